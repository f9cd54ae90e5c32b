"""`wgbstools init_genome` / `set_default_ref` without a GPU: the restatement and the library's host walk (csrc/fasta_core.h run serially:
the very functions the kernels run) against the goldens made from the reference's own functions, the refusals with their offsets, the
chromosome filter and order, the command line's refusals, the directory rules, and the constants the tests mirror."""
import hashlib
import json
import os
import os.path as op
import re

import numpy as np
import pytest

import init_genome_cases as GC
import init_genome_ref as GR
from wgbs_tools_amd import _lib, genome, init_genome, set_default_ref, wgbs_tools

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
with open(op.join(ROOT, 'tests', 'golden', 'init_genome_cases.json')) as f:
    GOLDEN = json.load(f)
TEXTS = ('cpg_bed', 'chrome_size', 'cpg_chrome_size')


def sha1(text):
    return hashlib.sha1(text.encode()).hexdigest()


def test_goldens_cover_the_cases():
    assert sorted(GOLDEN) == sorted(GC.CASES)
    for name, (text, no_sort) in GC.CASES.items():
        g = GOLDEN[name]
        assert g['text_sha1'] == hashlib.sha1(text).hexdigest() and g['no_sort'] == no_sort, name
        assert all(sha1(g[k]) == g[k + '_sha1'] for k in TEXTS), name
    assert GOLDEN['issue_example']['loci'] == [2, 5, 9]
    assert GOLDEN['across_sequences']['loci'] == [2] and GOLDEN['no_cpg']['cpg_chrome_size'] == 'chr1\t0\nchr2\t1\nchr3\t0\n'


@pytest.mark.parametrize('name', sorted(GC.CASES))
def test_restatement_gives_the_goldens(name):
    text, no_sort = GC.CASES[name]
    got, g = GR.init_genome(text, no_sort), GOLDEN[name]
    for k in TEXTS:
        assert got[k] == g[k], k
    assert got['loci'].tolist() == g['loci']


@pytest.mark.parametrize('name', sorted(GC.CASES))
def test_host_walk_gives_the_goldens(name):
    text, no_sort = GC.CASES[name]
    table, loci, refusal = _lib.debug_fasta_walk(text)
    assert refusal is None
    names = [s['name'].decode() for s in table]
    assert names == [n for n, _, _ in GR.table(text)]
    got, g = GR.assemble(table, loci, init_genome.kept_order(names, no_sort)), GOLDEN[name]
    for k in TEXTS:
        assert got[k] == g[k], k
    assert got['loci'].tolist() == g['loci']


def test_host_walk_and_restatement_agree_on_random_worlds():
    rng = np.random.default_rng(20261021)
    for _ in range(200):
        text = GC.random_world(rng, max_len=400)
        table, loci, refusal = _lib.debug_fasta_walk(text)
        assert refusal is None, text
        want = GR.table(text)
        assert [(s['name'].decode(), s['bases'], s['sites']) for s in table] == [(n, b, len(l)) for n, b, l in want], text
        assert loci.tolist() == [x for _, _, l in want for x in l], text


def test_header_offsets_and_names():
    text = b'\n>a b\nC\n>bb\tx\r\n>ccc\r\nG\n>d'
    table, loci, refusal = _lib.debug_fasta_walk(text)
    assert refusal is None and loci.size == 0
    assert [(s['name'], s['offset'], s['bases']) for s in table] == [(b'a', 1, 1), (b'bb', 8, 0), (b'ccc', 15, 1), (b'd', 23, 0)]


LONG = b'N' * GC.MAX_NAME


@pytest.mark.parametrize('text, want', [
    (b'ACGT\n>chr1\nA\n', (0, 'before_header')),
    (b'\n\r\n x\n>chr1\nA\n', (3, 'before_header')),
    (b'>chr1\nA\n>\nC\n', (8, 'empty_name')),
    (b'>chr1\nA\n> chr2\nC\n', (8, 'empty_name')),
    (b'>chr1\nA\n>', (8, 'empty_name')),
    (b'>chr1\nA\n>' + LONG + b'\nC\n', None),
    (b'>chr1\nA\n>' + LONG + b'N\nC\n', (8, 'long_name')),
    (b'>chr1\nAC GT\n', (8, 'bad_byte')),
    (b'>chr1\nACGT\nA\tC\n', (12, 'bad_byte')),
    (b'>chr1\nAC\x80GT\n', (8, 'bad_byte')),
    (b'>chr1\nAC\x7fGT\nx y\n', (8, 'bad_byte')),
    (b'>chr1 a b\x01\nAC~!GT\n', None),
    (b'x>\n>chr1\nA C\n', (0, 'before_header')),
])
def test_host_walk_refusals(text, want):
    assert _lib.debug_fasta_walk(text)[2] == want


def test_chromosome_filter_and_order():
    names = GC.NAMES
    assert [n for n in names if init_genome.is_valid_chrome(n)] == ['chrM', 'chr10', 'chr2', 'chrX', 'chr1', 'MT', '7', 'chr01']
    assert [names[i] for i in init_genome.kept_order(names)] == ['chr1', 'chr01', 'chr2', '7', 'chr10', 'chrX', 'chrM', 'MT']
    assert [names[i] for i in init_genome.kept_order(names, no_sort=True)] == ['chrM', 'chr10', 'chr2', 'chrX', 'chr1', 'MT', '7', 'chr01']
    for n in names + ['chrY', 'Y', 'chrMT', 'chr', '', 'chr1 ', 'CHR1', 'chrx']:
        assert init_genome.is_valid_chrome(n) == GR.is_valid_chrome(n) and init_genome.chromosome_order(n) == GR.chromosome_order(n), n
    assert GOLDEN['names_sorted']['chrome_size'].split('\n')[0] == 'chr1\t4' and GOLDEN['names_fasta_order']['chrome_size'].split('\n')[0] == 'chrM\t5'


def test_dispatcher_lists_the_commands(capsys):
    for cmd in ('init_genome', 'set_default_ref'):
        assert cmd in wgbs_tools.COMMANDS and cmd in wgbs_tools.REFERENCE_ONLY
    assert wgbs_tools.main(['wgbstools', 'init_genome', 'x']) == 1
    assert 'downloading a FASTA is not part of this build' in capsys.readouterr().err
    assert wgbs_tools.main(['wgbstools', 'init_genome', 'x', '--fasta_path', 'x.fa', '-d']) == 1
    assert 'init_genome -d / --debug is not part of this build' in capsys.readouterr().err
    assert wgbs_tools.main(['wgbstools', 'init_genome', 'x', '--fasta_path', '/nonexistent/x.fa', '-@', '4']) == 1
    assert 'No such file: /nonexistent/x.fa' in capsys.readouterr().err
    assert wgbs_tools.main(['wgbstools', 'init_genome', 'default', '--fasta_path', 'x.fa']) == 1
    assert 'invalid genome name' in capsys.readouterr().err


@pytest.fixture
def refs(tmp_path, monkeypatch):
    root = tmp_path / 'references'
    root.mkdir()
    monkeypatch.setenv('WGBSTOOLS_REFERENCES', str(root))
    return root


def test_existing_directory_needs_force(refs, tmp_path, capsys):
    fa = tmp_path / 'x.fa'
    fa.write_bytes(b'>chr1\nACG\n')
    (refs / 'hgX').mkdir()
    (refs / 'hgX' / 'keep.txt').write_text('mine')
    (refs / 'hgXY').mkdir()
    (refs / 'other.txt').write_text('other')
    assert wgbs_tools.main(['wgbstools', 'init_genome', 'hgX', '--fasta_path', str(fa)]) == 1
    err = capsys.readouterr().err
    assert 'genome hgX already exists' in err and 'Use -f to overwrite it.' in err
    assert (refs / 'hgX' / 'keep.txt').read_text() == 'mine'
    out = init_genome.setup_dir('hgX', True)                        # -f: that directory goes, and nothing else
    assert out == str(refs / 'hgX') and os.listdir(out) == []
    assert sorted(os.listdir(refs)) == ['hgX', 'hgXY', 'other.txt']
    assert init_genome.setup_dir('fresh', False) == str(refs / 'fresh')


def test_set_default_ref(refs, capsys):
    from wgbs_tools_amd import synth
    loci = np.array([5, 9, 20, 3], dtype=np.uint32)
    synth.write_genome(str(refs / 'gA'), ['chr1', 'chr2'], [3, 1], loci)
    synth.write_genome(str(refs / 'gB'), ['chr1'], [4], np.array([1, 4, 7, 9], dtype=np.uint32))
    with pytest.raises(genome.IllegalArgumentError, match='no default genome is set'):
        genome.GenomeRefPaths('default')
    cwd = os.getcwd()
    assert wgbs_tools.main(['wgbstools', 'set_default_ref', '--name', 'gA']) == 0
    assert os.getcwd() == cwd and os.readlink(refs / 'default') == 'gA'
    assert '[wt def] changed default genome to gA' in capsys.readouterr().err
    g = genome.GenomeRefPaths('default')
    assert g.genome == 'gA' and g.get_nr_sites() == 4 and genome.GenomeRefPaths().refdir == op.realpath(refs / 'gA')
    assert wgbs_tools.main(['wgbstools', 'set_default_ref', '--name', 'gB', '-ls']) == 0
    assert capsys.readouterr().out.split('\n')[:2] == ['Existing references:', '=====']
    assert os.readlink(refs / 'default') == 'gB'
    assert wgbs_tools.main(['wgbstools', 'set_default_ref', '-ls']) == 0
    assert sorted(capsys.readouterr().out.strip().split('\n')[2:]) == ['gA', 'gB (default)']
    assert wgbs_tools.main(['wgbstools', 'set_default_ref', '--name', 'nope']) == 1
    assert 'Invalid reference: nope' in capsys.readouterr().err
    assert wgbs_tools.main(['wgbstools', 'set_default_ref']) == 0
    assert 'you must specify either --name or -ls' in capsys.readouterr().err


def test_no_references_at_all(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv('WGBSTOOLS_REFERENCES', str(tmp_path / 'nothing_here'))
    assert wgbs_tools.main(['wgbstools', 'set_default_ref', '-ls']) == 0
    assert capsys.readouterr().out == 'No references found.\n'


def test_constants_mirror_the_headers():
    plan = open(op.join(ROOT, 'wgbs_tools_amd', 'csrc', 'fasta_plan.h')).read()
    core = open(op.join(ROOT, 'wgbs_tools_amd', 'csrc', 'fasta_core.h')).read()
    num = lambda src, name: int(re.search(r'#define %s (\d+)' % name, src).group(1))
    assert num(plan, 'WG_FA_TILE') == GC.TILE and num(plan, 'WG_FA_THREAD_BYTES') == GC.THREAD_BYTES
    assert num(plan, 'WG_FA_BLOCK') * GC.THREAD_BYTES == GC.TILE
    assert num(core, 'WG_FA_MAX_NAME') == GC.MAX_NAME == _lib.FA_MAX_NAME
    reasons = re.findall(r'#define WG_FA_BAD_([A-Z_]+) (\d+)', core)
    assert [(n.lower(), int(v)) for n, v in reasons[:5]] == [('before', 1), ('empty_name', 2), ('long_name', 3), ('byte', 4), ('long_seq', 5)]
    assert len(_lib.FA_REASONS) == int(dict(reasons)['REASONS'])


def test_layout_round_trips_on_the_host():
    """the round-trip input of the GPU suite: CG exactly at the loci"""
    from wgbs_tools_amd import synth
    import frag_cases
    sizes = [s for _, s in frag_cases.GENOME_CHROMS]
    names = [c for c, _ in frag_cases.GENOME_CHROMS]
    loci = synth.synth_loci(frag_cases.GENOME_SEED, sizes)
    at = np.concatenate([[0], np.cumsum(sizes)])
    assert all((np.diff(loci[at[k]:at[k + 1]].astype(np.int64)) >= 2).all() for k in range(len(sizes))), 'frag_cases has adjacent loci: use another generator'
    text = GC.layout_fasta(names, sizes, loci)
    got = GR.init_genome(text)
    assert got['loci'].tolist() == loci.tolist() and got['chroms'] == names


# ---- the shared headers under the sanitizers ----
def _have_sanitizers():
    import shutil
    import subprocess
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null', '-fsanitize=address,undefined'], input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason='no g++ with sanitizer runtimes')
def test_chunks_through_the_headers_under_sanitizers(tmp_path):
    """tests/native/san_fasta.cpp — the engine's way on the host (chunks cut anywhere, 16-byte stretches counted per entry state, composed,
    then walked from where the composition stands) by the functions the kernels call, every chunk a heap array of exactly its size — built
    plain and with ASan + UBSan: both give the restatement's table and loci whatever the cuts; exit status 0 says that the chunks and one
    serial walk agree and that no read left its array"""
    import subprocess
    rng = np.random.default_rng(5)
    jobs = [(name, text) for name, (text, _) in sorted(GC.CASES.items())] + [('world%d' % k, GC.random_world(rng, max_len=600)) for k in range(6)]
    for kind, flags in (('plain', []), ('asan_ubsan', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exe = str(tmp_path / ('san_fasta_' + kind))
        subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-I', op.join(ROOT, 'wgbs_tools_amd', 'csrc'), op.join(ROOT, 'tests', 'native', 'san_fasta.cpp'), '-o', exe] + flags)
        env = {'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'}
        for name, text in jobs:
            path = str(tmp_path / (name + '.fa'))
            with open(path, 'wb') as f:
                f.write(text)
            want = GR.table(text)
            lines = ['%s\t%d\t%d\t%d' % (s['name'].decode(), s['offset'], s['bases'], s['sites']) for s in _lib.debug_fasta_walk(text)[0]]
            assert [ln.split('\t')[0::2] for ln in lines] == [[n, str(b)] for n, b, _ in want]
            lines.append(' '.join(['loci'] + [str(x) for _, _, l in want for x in l]))
            lines.append('refused %d' % (2 ** 64 - 1))
            cut_sets = [[], [1], [len(text) - 1], sorted(int(x) for x in rng.integers(0, len(text) + 1, 5))]
            if name == 'every_case' and kind == 'asan_ubsan':
                cut_sets += [[at] for at in range(0, len(text) + 1, 3)]
            for cut in cut_sets:
                r = subprocess.run([exe, path] + [str(c) for c in cut], capture_output=True, timeout=120, env=env)
                assert r.returncode == 0, (kind, name, cut, r.stderr[-3000:])
                assert r.stdout.decode().split('\n')[:-1] == lines, (kind, name, cut)
        bad = str(tmp_path / 'bad.fa')
        with open(bad, 'wb') as f:
            f.write(b'>chr1\nAC\n>' + b'n' * 300 + b'\nA C\n>chr1\n')
        r = subprocess.run([exe, bad, '7', '200'], capture_output=True, timeout=120, env=env)
        assert r.returncode == 0 and r.stdout.decode().split('\n')[-2] == 'Invalid FASTA: a sequence name of more than 255 bytes at byte offset 9 of the text', (kind, r.stdout[-500:], r.stderr[-2000:])
