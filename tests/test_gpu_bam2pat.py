"""`wgbstools bam2pat` on the GPU (the kernels of csrc/sam_kernels.h behind wgbsseg_patview_set_sam): every golden case of the reference's own
`patter | sort | uniq -c` through the engine — whole, one feed per line, and as BGZF members of about 100 bytes inflated on the device, so
that members end inside lines and between mates —; the shapes of the text against the restatement tests/bam2pat_ref.py: a first mate in
the last bytes of a tile, a line longer than tile + spill, 300 filtered lines between two mates, a tile of more than 256 lines, a first
mate above 300 sites and one below --min_cpg carried over a cut; a seeded random world under several cuts; the command line end to end;
and what the engine refuses."""
import gzip
import json
import os.path as op

import numpy as np
import pytest

import bam2pat_cases as SC
import bam2pat_ref as BR
import frag_cases as FC
from wgbs_tools_amd import _lib, homog, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))
NAMES, SIZES = [c for c, _ in SC.CHROMS], [s for _, s in SC.CHROMS]
TILE, OVER = 4096, 1024                            # csrc/pat_kernels.h WG_PAT_TILE, WG_PAT_OVER


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'bam2pat_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def genome(tmp_path_factory):
    return FC.genome_dir(str(tmp_path_factory.mktemp('sam_genome')))[0]


def bgzf_bytes(text, member=100):
    return b''.join(homog._bgzf_member(text[p:p + member]) for p in range(0, len(text), member)) + homog._bgzf_member(b'')


def inflate(data):
    return gzip.decompress(data)


def engine(a, initial_records=0):
    v = _lib.PatView(1, SC.N_SITES + 1, sort=True, initial_records=initial_records)
    try:
        v.set_sam(SC.LOCI, NAMES, SIZES, paired=a['paired'], exclude_flags=a['exclude'], include_flags=a['include'], mapq=a['mapq'], strand=a['strand'], clip=a['clip'],
                  min_cpg=a['min_cpg'])
    except Exception:
        v.close()
        raise
    return v


def run(text, a, how='whole', cuts=None, deflate=False, initial_records=0, member=100):
    """the engine's (text, counters) for the SAM text; how: whole | lines (one feed per line) | cuts (at the byte offsets given) | bgzf (two
    feed_bgzf calls over members of `member` bytes)"""
    with engine(a, initial_records) as v:
        if how == 'bgzf':
            data = bgzf_bytes(text, member)
            used = v.feed_bgzf(data[:len(data) // 2])
            assert used + v.feed_bgzf(data[used:]) == len(data)
        else:
            if not text.endswith(b'\n'):
                text += b'\n'
            if how == 'lines':
                cuts = [i + 1 for i in range(len(text)) if text[i:i + 1] == b'\n']
            pos = 0
            for cut in list(cuts or []) + [len(text)]:
                v.feed(text[pos:cut])
                pos = cut
        v.finish(deflate=deflate)
        out = v.read()
        return (inflate(out) if deflate else out), v.sam_info()


def ref(text, a):
    return BR.bam2pat(text, SC.LOCI, SC.CHROMS, **a)


def line_ends(text):
    return [i + 1 for i in range(len(text)) if text[i:i + 1] == b'\n']


PE = dict(SC.DEFAULTS, paired=True, include=3)
SE = dict(SC.DEFAULTS)


# ---- the reference's bytes ----
@pytest.mark.parametrize('how', ['whole', 'lines', 'bgzf'])
def test_goldens_through_the_engine(how, golden):
    for name, case in SC.CASES.items():
        text, a = SC.case_text(case), SC.case_args(case)
        got, st = run(text, a, how, deflate=(how == 'bgzf'))
        assert got.decode() == golden[name]['stdout'], (how, name)
        assert st == ref(text, a)[1], (how, name)


def test_goldens_in_one_file_and_a_growing_table(golden):
    """the paired-end goldens one after the other as ONE file (names made distinct), a record table that begins with room for two records"""
    parts = []
    for k, (name, case) in enumerate(SC.CASES.items()):
        if SC.case_args(case) == PE:
            parts.append(b''.join((b'c%d_' % k + ln + b'\n') if ln and not ln.startswith(b'@') else ln + b'\n' for ln in SC.case_text(case).split(b'\n')[:-1]))
    text = b''.join(parts)
    want = ref(text, PE)
    assert len(parts) >= 8 and want[0].count(b'\n') > 20
    assert run(text, PE, initial_records=2) == want and run(text, PE, 'lines', initial_records=2) == want and run(text, PE, 'bgzf', deflate=True) == want


# ---- the shapes of the text ----
def _pairs(n, at=0, step=9, name=b'p'):
    out = []
    for k in range(n):
        at = SC._dense('chr1', 5, at + step)
        out.append((SC.pair('%s%d' % (name.decode(), k), 'chr1', at, 'CTC', at + 1, 'TCT', seed=k).encode()))
    return out


def filtered_line(n):
    """an unmapped read's line of exactly n >= 64 bytes"""
    base = len(SC.sam('pad', 4, '*', 0, 'A', cigar='*', tags=False))
    k = (n - base) // 2
    line = SC.sam('pad' + 'x' * ((n - base) % 2), 4, '*', 0, 'A' * (1 + k), cigar='*', tags=False).encode()
    assert len(line) == n
    return line


def test_first_mate_in_the_last_bytes_of_a_tile():
    pairs = _pairs(32)
    assert 15000 < sum(len(p) for p in pairs) < 30000
    for tail in (1, 2, 7, 40):                                          # the first mate of pair 9 begins `tail` bytes before a tile's end
        head = b''.join(pairs[:9])
        pad = (-(len(head) + tail)) % TILE
        text = head + filtered_line(pad if pad >= 64 else pad + TILE) + b''.join(pairs[9:])
        first = len(text) - sum(len(p) for p in pairs[9:])
        assert first % TILE == TILE - tail and text[first - 1:first] == b'\n'
        want = ref(text, PE)
        assert want[1]['pairs'] == 32 and run(text, PE) == want and run(text, PE, 'bgzf', deflate=True, member=3000) == want, tail
        mid = first + len(pairs[9]) // 2                                # a cut between the two mates
        assert run(text, PE, cuts=[text.index(b'\n', first) + 1]) == want and mid > first, tail


def test_line_longer_than_tile_and_spill():
    a = SC._dense('chr1', 4, 40)
    pos, seq = SC.adjusted('chr1', a, 'CTCT')
    for extra in (OVER + 50, TILE + OVER + 300, 3 * TILE):
        long_seq = seq + 'A' * extra                                    # the bases behind the CpGs: SEQ alone is longer than tile + spill
        m1 = SC.sam('long', 99, 'chr1', pos, long_seq).encode()
        m2 = SC.read('long', 147, 'chr1', a + 1, 'TCC', paired=True).encode()
        soft = SC.sam('soft', 99, 'chr1', pos, 'G' * extra + seq, cigar='%dS%dM' % (extra, len(seq))).encode() + SC.read('soft', 147, 'chr1', a + 2, 'CC', paired=True).encode()
        text = b''.join(_pairs(6)) + m1 + m2 + b''.join(_pairs(5, at=600, name=b'q')) + soft + b''.join(_pairs(3, at=900, name=b'r'))
        assert len(m1) > extra + 200
        want = ref(text, PE)
        assert want[1]['pairs'] == 16 and want[1]['invalid'] == 0
        assert run(text, PE) == want and run(text, PE, 'lines') == want and run(text, PE, 'bgzf', deflate=True, member=777) == want, extra


def test_300_filtered_lines_between_two_mates():
    a = SC._dense('chr1', 4, 1200)
    m1, m2 = SC.read('m', 99, 'chr1', a, 'CT', paired=True).encode(), SC.read('m', 147, 'chr1', a + 1, 'TC', paired=True).encode()
    filtered = b''.join(SC.sam('u%d' % k, 77 if k % 2 else 141, '*', 0, 'ACGTACGTAC', cigar='*', tags=False).encode() for k in range(300))
    text = b''.join(_pairs(3)) + m1 + filtered + m2 + b''.join(_pairs(3, at=500, name=b'q'))
    want = ref(text, PE)
    assert want[1]['pairs'] == 7 and want[1]['filtered'] == 300 and want[1]['left_single'] == 0
    ends = line_ends(text)
    at_m1 = ends[6]                                                     # behind the first mate
    assert run(text, PE) == want and run(text, PE, 'bgzf', deflate=True) == want
    assert run(text, PE, cuts=[at_m1]) == want and run(text, PE, cuts=[at_m1, ends[100], ends[200], ends[6 + 300]]) == want
    assert run(text, PE, cuts=ends[6:6 + 301:7]) == want


def test_tile_of_more_than_256_lines():
    """two-byte lines: 2,048 of them begin in one 4 KB tile; they name no chromosome, so they are dropped; three-field lines that name one
    are invalid and keep their place among the mates"""
    a = SC._dense('chr2', 4, 200)
    m1, m2 = SC.read('m', 99, 'chr2', a, 'CT', paired=True).encode(), SC.read('m', 147, 'chr2', a + 1, 'TC', paired=True).encode()
    text = b'x\n' * 700 + m1 + b'y\n' * 2500 + m2 + b'z\n' * 300
    want = ref(text, PE)
    assert want[1]['unknown_chrom'] == 3500 and want[1]['pairs'] == 1 and want[0].count(b'\n') == 1
    assert run(text, PE) == want and run(text, PE, cuts=[1400 + len(m1) + 2000]) == want
    short = b''.join(b'%d\t9\tchr2\n' % (k % 7) for k in range(900))     # runs of equal names among 900 invalid lines of chr2
    text = m1 + short + m2
    want = ref(text, PE)
    assert want[1]['invalid'] == 900 and want[1]['pairs'] == 0 and want[0].count(b'\n') == 2
    assert run(text, PE) == want and run(text, PE, 'bgzf', deflate=True) == want
    same = m1 + b'm\t9\tchr2\n' * 301 + m2                             # 303 lines of one name: place 302 is the last mate's, single
    want = ref(same, PE)
    assert want[1]['pairs'] == 151 and want[1]['left_single'] == 1 and want[0].count(b'\n') == 2
    assert run(same, PE) == want and run(same, PE, cuts=line_ends(same)[::50]) == want


def test_carried_first_mate_above_300_sites_and_below_min_cpg():
    L = SC.CHROM_LOCI['chr2']
    a = 300
    gap = int(L[a + 350] - L[a]) - 2
    long1 = SC.sam('far', 99, 'chr2', int(L[a]), 'CGCG', cigar='2M%dN2M' % gap).encode()       # C, 349 dots, C: 351 sites
    empty2 = SC.read('far', 147, 'chr2', a + 5, ['AG'], paired=True).encode()
    called2 = SC.read('far', 147, 'chr2', a + 5, 'T', paired=True).encode()
    for second, lines, too_long in ((empty2, 1, 0), (called2, 0, 1), (b'', 1, 0)):
        text = b''.join(_pairs(2)) + long1 + second + b''.join(_pairs(2, at=400, name=b'q'))
        want = ref(text, PE)
        assert want[1]['too_long'] == too_long and want[0].count(b'\tchr2\t') == 0 and want[0].count(b'chr2\t') == lines
        assert lines == 0 or b'C' + b'.' * 349 + b'C' in want[0]
        assert run(text, PE) == want and run(text, PE, 'lines') == want and run(text, PE, 'bgzf', deflate=True) == want, lines
    short = dict(PE, min_cpg=3)
    b = SC._dense('chr1', 6, 1700)
    one, far = SC.read('s', 99, 'chr1', b, 'C', paired=True).encode(), SC.read('s', 147, 'chr1', b + 2, 'T', paired=True).encode()
    near = SC.read('s', 147, 'chr1', b + 1, 'T', paired=True).encode()
    for second, lines in ((far, 1), (near, 0), (b'', 0)):                # C.T is long enough, CT and C alone are not
        text = b''.join(_pairs(2)) + one + second + b''.join(_pairs(1, at=500, name=b'q'))
        want = ref(text, short)
        assert want[0].count(b'\n') == 3 + lines
        assert run(text, short) == want and run(text, short, 'lines') == want and run(text, short, 'bgzf', deflate=True) == want, lines


def test_seeded_world_under_several_cuts():
    rng = np.random.default_rng(20261021)
    for k in range(2):
        text, a = SC.random_world(rng, 2000)
        if k == 0:
            a = dict(a, paired=True, include=3)
        alive = [BR.tokens_of(ln) for ln in text.split(b'\n') if ln and not ln.startswith(b'@')]
        assert not SC.names_split_by_other_chromosomes([(t[0], t[2]) for t in alive if len(t) >= 3 and t[2] in (b'chr1', b'chr2')])
        want = ref(text, a)
        assert len(text) > 100 * TILE and want[0].count(b'\n') > 300
        ends = line_ends(text)
        cuts = sorted(set(rng.choice(ends[:-1], size=40, replace=False).tolist()))
        assert run(text, a) == want, k
        assert run(text, a, cuts=cuts, initial_records=64) == want, k
        assert run(text, a, 'bgzf', deflate=True, member=100) == want and run(text, a, 'bgzf', deflate=True, member=65280) == want, k


# ---- end to end ----
@pytest.mark.parametrize('how', ['plain', 'gzip', 'bgzf_device'])
def test_cli_end_to_end(how, genome, tmp_path, capsys):
    rng = np.random.default_rng(5)
    text, a = SC.random_world(rng, 600)
    while not a['paired']:                                             # the command looks at the first alignment's FLAG
        text, a = SC.random_world(rng, 600)
    a = dict(a, include=3, min_cpg=2, clip=1)
    path = str(tmp_path / ('s.x.sam' if how == 'plain' else 's.x.sam.gz'))
    if how == 'plain':
        with open(path, 'wb') as f:
            f.write(text)
    elif how == 'gzip':
        with gzip.open(path, 'wb') as f:
            f.write(text)
    else:
        with open(path, 'wb') as f:
            f.write(bgzf_bytes(text, 100))
    out = tmp_path / 'out'
    out.mkdir()
    argv = ['wgbstools', 'bam2pat', path, '-o', str(out), '--genome', genome, '--min_cpg', '2', '--clip', '1', '-T', str(tmp_path), '-@', '4']
    assert wgbs_tools.main(argv + (['--inflate', 'device'] if how == 'bgzf_device' else [])) == 0
    err = capsys.readouterr().err
    want, n = ref(text, a)
    assert 'no .csi index is written' in err and 'is not BGZF' not in err and ('%d pairs' % n['pairs']) in err and 'paired-end' in err
    data = (out / 's.x.pat.gz').read_bytes()
    assert data[:4] == b'\x1f\x8b\x08\x04' and data.endswith(homog._bgzf_member(b'')) and inflate(data) == want
    ref_dir = tmp_path / 'ref'
    ref_dir.mkdir()
    with gzip.open(str(ref_dir / 's.x.pat.gz'), 'wb') as f:
        f.write(want)
    assert wgbs_tools.main(['wgbstools', 'pat2beta', str(ref_dir / 's.x.pat.gz'), '-o', str(ref_dir), '--genome', genome]) == 0
    beta = (out / 's.x.beta').read_bytes()
    assert len(beta) == 2 * SC.N_SITES and beta == (ref_dir / 's.x.beta').read_bytes() and any(beta)
    # -f, -l, --no_beta and the strand filter
    assert wgbs_tools.main(argv + ['-f', '--no_beta', '--top_strand']) == 0
    top = ref(text, dict(a, strand=1))[0]
    assert inflate((out / 's.x.pat.gz').read_bytes()) == top and top != want and (out / 's.x.beta').read_bytes() == beta
    assert wgbs_tools.main(argv + ['-f', '-l']) == 0 and (out / 's.x.lbeta').stat().st_size == 4 * SC.N_SITES
    capsys.readouterr()


def test_cli_standard_input_and_nothing_left(genome, tmp_path, capsys, monkeypatch):
    import io
    text = SC.case_text(SC.CASES['mates'])
    monkeypatch.setattr('sys.stdin', io.TextIOWrapper(io.BytesIO(text)))
    assert wgbs_tools.main(['wgbstools', 'bam2pat', '-', '--name', 'piped', '-o', str(tmp_path), '--genome', genome, '--no_beta']) == 0
    assert inflate((tmp_path / 'piped.pat.gz').read_bytes()) == ref(text, PE)[0] and not (tmp_path / 'piped.beta').exists()
    nothing = tmp_path / 'none.sam'
    nothing.write_bytes(SC.case_text(SC.CASES['clip_0']))
    capsys.readouterr()
    assert wgbs_tools.main(['wgbstools', 'bam2pat', str(nothing), '-o', str(tmp_path), '--genome', genome, '--clip', '5000']) == 0
    assert 'No reads found. No pat file is generated' in capsys.readouterr().err and not (tmp_path / 'none.pat.gz').exists()


# ---- what the engine refuses ----
def test_engine_state_refusals():
    text = SC.case_text(SC.CASES['mates'])
    with engine(PE) as v:
        for call, what in ((lambda: v.set_sam(SC.LOCI, NAMES, SIZES), 'patview_set_sam: called twice'), (lambda: v.set_mask([1], [5]), 'the engine takes SAM text: a mask'),
                           (lambda: v.set_labels(['a']), 'the engine takes SAM text: labels'), (v.next_file, 'an engine that takes SAM text takes one file')):
            with pytest.raises(_lib.SegmentorError, match=what) as e:
                call()
            assert e.value.code == _lib.E_STATE
        v.feed(text)
        with pytest.raises(_lib.SegmentorError, match='feed and feed_bgzf cannot be mixed'):
            v.feed_bgzf(bgzf_bytes(text))
        with pytest.raises(_lib.SegmentorError, match='a chunk must end with a complete line'):
            v.feed(text.rstrip(b'\n'))
        assert v.finish()[0] == ref(text, PE)[0].count(b'\n') and v.kernel_ms() > 0
        with pytest.raises(_lib.SegmentorError, match='finish\\(\\) has been called'):
            v.feed(text)
    with _lib.PatView(1, SC.N_SITES + 1, sort=True) as v:
        v.feed(b'chr1\t5\tC\t1\n')
        with pytest.raises(_lib.SegmentorError, match='patview_set_sam: called after the first feed'):
            v.set_sam(SC.LOCI, NAMES, SIZES)
    for kw, what in ((dict(sort=False), 'must be created with WGBSSEG_VIEW_SORT and no other flag \\(got 0\\)'), (dict(sort=True, strip=True), 'no other flag \\(got 10\\)')):
        with _lib.PatView(1, SC.N_SITES + 1, **kw) as v:
            with pytest.raises(_lib.SegmentorError, match=what):
                v.set_sam(SC.LOCI, NAMES, SIZES)
    with _lib.PatView(1, SC.N_SITES + 1, sort=True, mask=([3], [9])) as v:
        with pytest.raises(_lib.SegmentorError, match='the engine has a mask: SAM text does not go with it'):
            v.set_sam(SC.LOCI, NAMES, SIZES)
    with _lib.PatView(1, SC.N_SITES + 1, sort=True) as v:
        v.set_labels(['a', 'b'])
        with pytest.raises(_lib.SegmentorError, match='the engine has labels: SAM text does not go with it'):
            v.set_sam(SC.LOCI, NAMES, SIZES)
    with _lib.PatView(1, 100, sort=True) as v:
        with pytest.raises(_lib.SegmentorError, match='bedbeta: chromosomes 0 and 1 have the same name'):
            v.set_sam(SC.LOCI, ['a', 'a'], SIZES)
    with _lib.PatView(1, SC.N_SITES + 1, sort=True) as v:
        with pytest.raises(_lib.SegmentorError, match='patview_set_sam: mapq 300'):
            v.set_sam(SC.LOCI, NAMES, SIZES, mapq=300)
        v.set_sam(SC.LOCI, NAMES, SIZES)                                 # a refused call leaves the engine as it was
        assert v.finish() == (0, 0) and v.sam_info()['lines'] == 0
