"""`wgbstools bed2beta` on the GPU (k_bedbeta_scan / k_bedbeta_unpack behind wgbsseg_bedbeta_*): every golden case of the reference's own
functions through the command line as plain text, as gzip and as BGZF inflated on the device; through the engine the edges of the text —
a tile of more than 256 lines, a line across a tile edge, a line longer than tile + spill, a last line without its newline —, duplicates
inside one wavefront, across tiles and across feeds under every cut of the same text, next_file, every refusal with its byte offset, the
counters; and a time-boxed random comparison against the restatement tests/bed2beta_ref.py."""
import gzip
import hashlib
import json
import os.path as op
import time

import numpy as np
import pytest

import bed2beta_cases as BC
import bed2beta_ref as BR
import frag_cases as FC
from wgbs_tools_amd import _lib, homog, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))
LOCI = BC.loci().astype(np.uint32)
CHROMS = BC.CHROMS
NAMES, SIZES = [c for c, _ in CHROMS], [s for _, s in CHROMS]
TILE, OVER = 4096, 1024                            # csrc/pat_kernels.h WG_PAT_TILE, WG_PAT_OVER


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'bed2beta_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def genome(tmp_path_factory):
    return FC.genome_dir(str(tmp_path_factory.mktemp('bed_genome')))[0]


@pytest.fixture(scope='module')
def engine():
    """one engine for the module, as the command uses one for all files: every use begins with next_file"""
    with _lib.BedBeta(LOCI, NAMES, SIZES) as b:
        yield b


def bgzf_bytes(text, member=3000):
    return b''.join(homog._bgzf_member(text[p:p + member]) for p in range(0, len(text), member)) + homog._bgzf_member(b'')


def run(b, text, add_one=False, cuts=None, bgzf=False):
    """the engine's (rows, counters) for `text` as the next file; cuts: byte offsets (line ends) at which the text is cut into feeds;
    bgzf: fed as BGZF bytes in two calls (a text without its last newline must go this way)"""
    b.next_file(add_one=add_one, header=BR.is_header(text))
    if bgzf:
        data = bgzf_bytes(text)
        used = b.feed_bgzf(data[:len(data) // 2])
        assert used + b.feed_bgzf(data[used:]) == len(data)
    else:
        pos = 0
        for cut in list(cuts or []) + [len(text)]:
            b.feed(text[pos:cut])
            pos = cut
    return b.finish()


def same(got, want):
    return np.array_equal(got[0], want[0]) and got[1] == want[1]


def ref(text, add_one=False):
    return BR.bed2beta(text, LOCI, CHROMS, add_one=add_one)


def site_line(site, meth, total, mid=b'.'):
    chrom, p = (b'chr1', BC.L1[site]) if site < BC.N1 else (b'chr2', BC.L2[site - BC.N1])
    return b'%s\t%d\t%s\t%d\t%d\n' % (chrom, p, mid, meth, total)


# ---- the reference's bytes through the command line ----
@pytest.mark.parametrize('how', ['plain', 'gzip', 'bgzf_device'])
def test_cli_matches_reference(how, golden, genome, tmp_path, capsys):
    """every golden case, all of them in ONE call: the dictionary goes up once, next_file between two files"""
    paths = []
    for name, case in BC.CASES.items():
        text = BC.case_text(case)
        path = str(tmp_path / (name + ('.bed' if how == 'plain' else '.bed.gz')))
        if how == 'plain':
            with open(path, 'wb') as f:
                f.write(text)
        elif how == 'gzip':
            with gzip.open(path, 'wb') as f:
                f.write(text)
        else:
            homog.write_bgzf(path, text, 2)
        paths.append((name, path))
    out = tmp_path / 'out'
    out.mkdir()
    for flag in ([], ['--add_one']):                                    # --add_one is the call's: the cases that ask for it go together
        mine = [p for n, p in paths if BC.case_flags(BC.CASES[n]) == flag]
        argv = ['wgbstools', 'bed2beta'] + mine + flag + ['-o', str(out), '--genome', genome] + (['--inflate', 'device'] if how == 'bgzf_device' else [])
        assert wgbs_tools.main(argv) == 0
    err = capsys.readouterr().err
    assert 'is not BGZF' not in err
    for name, _ in paths:
        data = (out / (name + '.beta')).read_bytes()
        assert len(data) == 2 * BC.N_SITES and hashlib.sha1(data).hexdigest() == golden[name]['out_sha1'], (how, name)
        assert BC.sparse(np.frombuffer(data, dtype=np.uint8).reshape(-1, 2)) == golden[name]['rows'], (how, name)
    assert '[wt bed] big_mixed.bed' in err and '406 duplicates dropped' in err


def test_cli_refusal_and_overwrite(genome, tmp_path, capsys):
    bed = tmp_path / 'a.bed'
    good = site_line(5, 1, 2)
    bed.write_bytes(good + b'chr1\t5\t6\t3\t2\n')
    (tmp_path / 'a.beta').write_bytes(b'old')
    assert wgbs_tools.main(['wgbstools', 'bed2beta', str(bed), '-o', str(tmp_path), '--genome', genome, '-f']) == 1
    assert 'failed in bed2beta: the line at byte offset %d of the input has #meth above #total' % len(good) in capsys.readouterr().err
    assert not (tmp_path / 'a.beta').exists()                            # -f removed the old file, the refusal wrote none
    bed.write_bytes(good)
    assert wgbs_tools.main(['wgbstools', 'bed2beta', str(bed), '-o', str(tmp_path), '--genome', genome]) == 0
    assert BC.sparse(np.fromfile(str(tmp_path / 'a.beta'), dtype=np.uint8).reshape(-1, 2)) == [[5, 1, 2]]
    gz = tmp_path / 'plain.bed.gz'
    with gzip.open(str(gz), 'wb') as f:
        f.write(good)
    assert wgbs_tools.main(['wgbstools', 'bed2beta', str(gz), '-o', str(tmp_path), '--genome', genome, '--inflate', 'device']) == 0
    assert 'is not BGZF' in capsys.readouterr().err                      # plain gzip: inflated on the host, and said so
    assert (tmp_path / 'plain.beta').read_bytes() == (tmp_path / 'a.beta').read_bytes()


# ---- the edges of the text ----
def test_second_round_of_a_tile(engine):
    """ten-byte lines: 409 of them begin in one 4 KB tile, more than the 256 threads of a workgroup"""
    lines = [b'c\t%02d\t\t1\t2\n' % (i % 100) for i in range(1200)]
    assert all(len(ln) == 10 for ln in lines) and len(lines) * 10 < 3 * TILE
    got = run(engine, b''.join(lines))
    assert not got[0].any() and got[1] == dict(lines=1200, matched=0, unknown_chrom=1200, not_cpg=0, duplicates=0, sites_set=0)
    engine.next_file()
    engine.feed(b''.join(lines[:300]) + b'c\t07\t\t\t1\t\n' + b''.join(lines[300:]))      # line 300 of the first tile: a thread's second line
    with pytest.raises(_lib.SegmentorError, match='byte offset 3000 of the input has a start, #meth or #total that is not'):
        engine.finish()
    text = b''.join(b'chr1\t%05d\t\t1\t%d\n' % (p, 1 + p % 9) for p in range(10000, 11500))      # every position of a range, 256 lines a tile
    got, want = run(engine, text), ref(text)
    assert same(got, want) and want[1]['lines'] == 1500 and 0 < want[1]['matched'] < 1500


def test_lines_across_tile_edges_and_long_lines(engine):
    rows = [site_line(i, i % 7, 7 + i % 300) for i in range(0, 600)]
    for pad in range(0, 40, 3):                                         # the line that crosses the first tile edge crosses it at every field in turn
        text = b'chr9\t1\t' + b'x' * pad + b'\t0\t0\n' + b''.join(rows)
        assert len(text) > 2 * TILE
        assert same(run(engine, text), ref(text)), pad
    for mid in (OVER - 30, OVER + 7, TILE + OVER + 500, 3 * TILE):     # field 3 runs into the spill, past it, past tile + spill
        long_line = site_line(700, 3, 400, mid=b'y' * mid)
        text = b''.join(rows[:150]) + long_line + b''.join(rows[150:]) + site_line(701, 1, 1, mid=b'z' * mid)
        got, want = run(engine, text), ref(text)
        assert same(got, want) and got[0][700].tolist() == [1, 255] and got[0][701].tolist() == [1, 1], mid
        assert same(run(engine, text.rstrip(b'\n'), bgzf=True), want), mid


def test_last_line_without_newline(engine):
    text = site_line(9, 1, 3) + b'\n\n' + site_line(BC.N_SITES - 1, 2, 2) + site_line(0, 5, 600)
    want = ref(text)
    assert BC.sparse(want[0]) == [[0, 2, 255], [9, 1, 3], [BC.N_SITES - 1, 2, 2]]
    assert same(run(engine, text.rstrip(b'\n'), bgzf=True), want) and same(run(engine, text, bgzf=True), want) and same(run(engine, text), want)
    engine.next_file()
    with pytest.raises(_lib.SegmentorError, match='a chunk must end with a complete line'):
        engine.feed(text.rstrip(b'\n'))


# ---- duplicates: the first line wins under every cut ----
def _dup_text():
    """duplicates of one site inside one wavefront, in two tiles and far apart, the first never the largest; and a site whose first line
    is 0, 0: it is set, and stays 0, 0 whatever follows"""
    rows = [site_line(i, 1 + i % 5, 9 + i % 500) for i in range(900)]
    rows[3:3] = [site_line(1000, 2, 9), site_line(1000, 9, 9), site_line(1001, 0, 0), site_line(1000, 1, 9)]     # neighbours: one wavefront
    rows.insert(400, site_line(1000, 8, 9))                             # the same site two tiles on
    rows.insert(401, site_line(1001, 4, 4))
    rows.insert(250, site_line(2000, 3, 1000))
    rows.append(site_line(2000, 999, 1000))                             # ... and at the far end
    rows.append(site_line(1001, 7, 7))
    return rows


def test_first_line_wins_under_every_cut(engine):
    rows = _dup_text()
    text = b''.join(rows)
    want = ref(text)
    assert want[0][1000].tolist() == [2, 9] and want[0][1001].tolist() == [0, 0] and want[0][2000].tolist() == [0, 255] and want[1]['duplicates'] == 6
    assert len(text) > 3 * TILE
    ends = np.cumsum([len(r) for r in rows]).tolist()
    for cuts in ([], ends[:8], [ends[4]], [ends[5], ends[401]], ends[100::100], [ends[250], ends[402], ends[-3], ends[-2]]):
        assert same(run(engine, text, cuts=cuts), want), cuts
    assert same(run(engine, text, bgzf=True), want)
    back = b''.join(reversed(rows))                                     # the same lines in the other order: other winners
    want_back = ref(back)
    assert want_back[0][1000].tolist() == [8, 9] and want_back[0][1001].tolist() == [7, 7] and want_back[0][2000].tolist() == [254, 255]
    back_ends = np.cumsum([len(r) for r in reversed(rows)]).tolist()
    assert same(run(engine, back), want_back) and same(run(engine, back, cuts=back_ends[:3] + back_ends[500:502]), want_back)


def test_next_file_leaves_nothing_behind(engine):
    a, b = BC.case_text(BC.CASES['big_mixed']), BC.case_text(BC.CASES['totals'])
    first = run(engine, a)
    assert first[1]['sites_set'] == BC.N_SITES
    assert same(run(engine, b), ref(b))                                  # the table, the counters and the header flag of the file before are gone
    engine.next_file()
    engine.feed(b'chr1\tx\n' + b)
    with pytest.raises(_lib.SegmentorError, match='byte offset 0 of the input has fewer than five'):
        engine.finish()
    assert same(run(engine, b), ref(b))                                  # ... and so is its refusal
    got = run(engine, a[:len(BC.HEADER)] + b'\n', add_one=True)
    assert not got[0].any() and got[1] == dict(lines=0, matched=0, unknown_chrom=0, not_cpg=0, duplicates=0, sites_set=0)
    with _lib.BedBeta(LOCI, NAMES, SIZES, add_one=True, header=True) as fresh:      # the flags of create(); text and BGZF on one engine, file by file
        text = BC.case_text(BC.CASES['add_one_header'])
        fresh.feed(text)
        want = ref(text, add_one=True)
        assert same(fresh.finish(), want) and same(fresh.finish(), want)             # finish() may be asked twice
        assert fresh.kernel_ms() > 0 and fresh.inflate_ms() == 0
        assert same(run(fresh, text, add_one=True, bgzf=True), want) and fresh.inflate_ms() > 0
        with pytest.raises(_lib.SegmentorError, match='feed and feed_bgzf cannot be mixed'):
            fresh.feed(text)


# ---- refusals and counters ----
def test_every_refusal_with_its_offset(engine):
    rows = [site_line(i, 1, 2) for i in range(700)]
    bads = ((b'chr1\t5\t6\t1\n', 'has fewer than five tab-separated fields'), (b'chr1\n', 'has fewer than five'), (b'chr1\t+5\t6\t1\t2\n', 'that is not 1 to 18 decimal digits'),
            (b'chr1\t5\t6\t1.5\t2\n', 'that is not 1 to 18'), (b'chr1\t5\t6\t1\t2e1\n', 'that is not 1 to 18'), (b'chr1\t5\t6\t1\t2\r\n', 'that is not 1 to 18'),
            (b'chr1\t%s\t6\t1\t2\n' % (b'1' * 19), 'that is not 1 to 18'), (b'chrQ\t5\t6\t3\t2\n', 'has #meth above #total'),
            (b'chrQ\t5\t6\t3\t2147483648\n', 'has a #total above 2^31 - 1'))
    starts = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    edge = int(np.searchsorted(starts, TILE)) - 1                      # the line that holds the first tile's last byte
    assert starts[edge] < TILE < starts[edge + 1]
    for at in (0, 1, edge, edge + 1, 699):                              # in the first tile, across the tile edge and behind it, at the end
        off = int(starts[at])
        for bad, what in bads:
            engine.next_file()
            engine.feed(b''.join(rows[:at]) + bad + b''.join(rows[at:]) + b'late\n')      # a later refused line does not show
            with pytest.raises(_lib.SegmentorError) as e:
                engine.finish()
            assert e.value.code == _lib.E_ARG and e.value.msg.startswith('failed in bed2beta: the line at byte offset %d of the input ' % off) and what in e.value.msg, (at, bad)
    engine.next_file()
    engine.feed(b''.join(rows[:300]))
    engine.feed(b''.join(rows[300:]) + b'chr1\t5\n')                     # the offset counts over the feeds
    with pytest.raises(_lib.SegmentorError, match='byte offset %d of the input has fewer' % sum(len(r) for r in rows)):
        engine.finish()


def test_counters_and_other_genomes():
    """a genome of its own: names that are prefixes of each other, an empty chromosome, ranges not in the order of the names, sites that
    belong to no chromosome"""
    names = ['chr10', 'chr1', 'chr', 'chr1_random', 'chrEmpty']
    ranges = [(0, 4), (4, 8), (8, 10), (12, 16), (10, 10)]
    loci = np.array([5, 7, 9, 11, 5, 7, 9, 11, 5, 9, 1, 2, 5, 7, 9, 4000000000], dtype=np.uint32)
    text = b''.join(b'%s\t%d\t0\t%d\t%d\n' % (c, p, m, t) for c, p, m, t in (
        (b'chr1', 5, 1, 1), (b'chr10', 5, 2, 2), (b'chr', 5, 3, 3), (b'chr1_random', 5, 4, 4), (b'chrEmpty', 5, 5, 5), (b'chr1_rando', 5, 6, 6),
        (b'chr1', 11, 7, 7), (b'chr1', 12, 8, 8), (b'chr', 7, 9, 9), (b'chr1_random', 4000000000, 10, 10), (b'chr1_random', 4000000001, 1, 1),
        (b'chr10', 5, 9, 9), (b'chr100', 5, 9, 9), (b'chr1', 11, 1, 7)))
    with _lib.BedBeta(loci, names, chrom_ranges=([r[0] for r in ranges], [r[1] for r in ranges])) as b:
        b.feed(text)
        rows, st = b.finish()
    assert BC.sparse(rows) == [[0, 2, 2], [4, 1, 1], [7, 7, 7], [8, 3, 3], [12, 4, 4], [15, 10, 10]]
    assert st == dict(lines=14, matched=8, unknown_chrom=2, not_cpg=4, duplicates=2, sites_set=6)
    with pytest.raises(_lib.SegmentorError, match='bedbeta: chromosomes 0 and 1 have the same name'):
        _lib.BedBeta(loci, ['a', 'a'], [8, 8])
    with pytest.raises(_lib.SegmentorError, match='do not ascend at site 4 '):
        _lib.BedBeta(loci, ['a'], [16])


def test_golden_cases_through_the_engine(engine, golden):
    for name, case in BC.CASES.items():
        text = BC.case_text(case)
        got = run(engine, text, add_one=bool(case.get('add_one')))
        assert hashlib.sha1(got[0].tobytes()).hexdigest() == golden[name]['out_sha1'] and got[1] == ref(text, bool(case.get('add_one')))[1], name


def test_random_worlds_match_the_restatement(engine):
    seed = int(time.time()) & 0xffffff
    print('seed', seed)
    rng = np.random.default_rng(seed)
    t0, n = time.time(), 0
    while time.time() - t0 < 3.0 or n < 3:
        text, add_one = BC.random_world(rng)
        want = ref(text, add_one)
        ends = [i + 1 for i in range(len(text)) if text[i:i + 1] == b'\n']
        if text.endswith(b'\n'):
            cuts = sorted(set(rng.choice(ends[:-1], size=min(len(ends) - 1, int(rng.integers(0, 4))), replace=False).tolist())) if len(ends) > 1 else []
            assert same(run(engine, text, add_one=add_one, cuts=cuts), want), (seed, n, 'text')
        assert same(run(engine, text, add_one=add_one, bgzf=True), want), (seed, n, 'bgzf')
        n += 1
