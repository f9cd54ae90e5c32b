"""`wgbstools test_bimodal` on the GPU (k_bim_em and the streaming read table behind wgbsseg_bimodal_*): every golden case of the
reference through the command line, byte for byte; the device's raw per-block numbers bit for bit against the restatement
tests/bimodal_ref.py (every case, the hand-built corner cases of tests/bimodal_corners.py on both table paths and three chunk
sizes, a sweep over fixed seeds, then a time-boxed random sweep); the kernel's column-count arithmetic through
wgbsseg_debug_bimodal_terms against its host twin on the whole lattice of tests/bimodal_lattice.py; chunk sizes from a few hundred
bytes to the whole file; the LDS and the global-memory table paths; the refusals with their byte offsets."""
import gzip
import json
import os
import os.path as op
import time

import numpy as np
import pytest

import bimodal_cases as BC
import bimodal_corners as BK
import bimodal_lattice as BL
import bimodal_ref as BR
from wgbs_tools_amd import _lib, test_bimodal, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))
with open(op.join(ROOT, 'tests', 'golden', 'bimodal_cases.json')) as _f:
    GOLDEN = json.load(_f)['cases']


@pytest.fixture(scope='module')
def genome(tmp_path_factory):
    d = str(tmp_path_factory.mktemp('genome') / 'synth')
    BC.write_genome(d)
    return d


def _opts(args):
    strict = '--strict' in args
    min_len = int(args[args.index('--min_len') + 1]) if '--min_len' in args else 1
    return strict, min_len


def _blocks_of(case):
    """the blocks the command tests, in the reference's (genome) order"""
    if 'sites' in case:
        return np.array([case['sites'][0]]), np.array([case['sites'][1]])
    return BC.case_blocks(case['blocks'])


def _want(text, s, e, strict, min_len):
    starts, reads = BR.parse_pat(text)
    return [BR.block_result(starts, reads, a, b, strict, min_len) for a, b in zip(s.tolist(), e.tolist())]


def _same_bits(ll, cnt, want):
    for j, w in enumerate(want):
        got = (ll[j, 0], ll[j, 1], ll[j, 2], int(cnt[j, 0]), int(cnt[j, 1]), int(cnt[j, 2]))
        if w[4] == 0:                                             # no rows: the columns, nothing else
            assert got[3:5] == (w[3], 0), (j, got, w)
            continue
        assert np.float64(got[0]).tobytes() == np.float64(w[0]).tobytes(), (j, 'll0', got, w)
        assert np.float64(got[1]).tobytes() == np.float64(w[1]).tobytes(), (j, 'll_em', got, w)
        assert np.float64(got[2]).tobytes() == np.float64(w[2]).tobytes(), (j, 'sum_n', got, w)
        assert got[3:] == (w[3], w[4], w[5]), (j, got, w)


@pytest.mark.parametrize('name', sorted(GOLDEN))
def test_cli_matches_reference(name, genome, tmp_path, capsys):
    case = BC.CASES[name]
    pat_text, bed_text, args = BC.case_inputs(case)
    pat = str(tmp_path / 'smp.pat.gz')
    with gzip.open(pat, 'wb') as f:
        f.write(pat_text)
    argv = ['wgbstools', 'test_bimodal', pat, '--genome', genome] + args
    if bed_text is None:
        argv += ['-s', '%d-%d' % tuple(case['sites'])]
    else:
        bed = tmp_path / 'blocks.bed'
        bed.write_text(bed_text)
        argv += ['-L', str(bed)]
    capsys.readouterr()
    assert wgbs_tools.main(argv) == 0
    assert capsys.readouterr().out == GOLDEN[name]['text'], name


@pytest.mark.parametrize('name', sorted(BC.CASES))
def test_device_bits_match_restatement(name):
    case = BC.CASES[name]
    text, _, args = BC.case_inputs(case)
    strict, min_len = _opts(args)
    s, e = _blocks_of(case)
    with _lib.Bimodal(s, e, strict, min_len) as b:
        b.feed(text)
        ll, cnt = b.finish()
    _same_bits(ll, cnt, _want(text, s, e, strict, min_len))


def test_chunk_sizes_agree():
    """from a few hundred bytes per chunk (reads retire and drop between chunks) to the whole file in one"""
    case = BC.CASES['L_default']
    text, _, _ = BC.case_inputs(case)
    s, e = _blocks_of(case)
    results = []
    for size in (300, 1000, 4096, 20000, 150000, len(text)):
        with _lib.Bimodal(s, e) as b:
            pos = 0
            while pos < len(text):
                cut = text.find(b'\n', min(len(text) - 1, pos + size - 1)) + 1
                b.feed(text[pos:cut])
                pos = cut
            assert b.kernel_ms() >= 0
            results.append(b.finish())
    for ll, cnt in results[1:]:
        assert ll.tobytes() == results[0][0].tobytes() and np.array_equal(cnt, results[0][1])


def test_lds_and_global_paths_agree():
    """the wide blocks (more columns than the LDS tables hold) and every block forced onto global memory"""
    case = BC.CASES['L_strict']
    text, _, _ = BC.case_inputs(case)
    s, e = _blocks_of(case)
    out = []
    for cols in (-1, 0, 16):
        with _lib.Bimodal(s, e, True, 1, max_lds_cols=cols) as b:
            b.feed(text)
            out.append(b.finish())
    _, cnt = out[0]
    assert (cnt[:, 0] > 256).any() and (cnt[:, 0] <= 16).any()
    for ll, c in out[1:]:
        assert ll.tobytes() == out[0][0].tobytes() and np.array_equal(c, cnt)
    _same_bits(out[0][0], cnt, _want(text, s, e, True, 1))


def test_refusals(tmp_path):
    s, e = np.array([1, 10]), np.array([5, 20])
    good = b'chr1\t1\tCCCC\t1\nchr1\t3\tTTTT\t2\n'
    for bad in (b'chr1\t5\tCT\n', b'chr1\tx\tCT\t3\n', b'chr1\t5\tCT\t\n'):
        with _lib.Bimodal(s, e) as b:
            b.feed(good)
            b.feed(bad)
            with pytest.raises(_lib.SegmentorError, match='invalid line at byte offset %d' % len(good)):
                b.finish()
    with _lib.Bimodal(s, e) as b:
        b.feed(good + b'chr1\t4\tCC\t-2\n')
        with pytest.raises(_lib.SegmentorError, match='negative read count at byte offset %d' % len(good)):
            b.finish()
    # a descending read: inside a chunk, across tiles and across chunks
    with _lib.Bimodal(s, e) as b:
        b.feed(good + b'chr1\t2\tCCC\t1\n')
        with pytest.raises(_lib.SegmentorError, match='not sorted.*byte offset %d' % len(good)):
            b.finish()
    filler = b''.join(b'chr1\t%d\tCCCT\t1\n' % (3 + i // 1000) for i in range(3000))
    with _lib.Bimodal(s, e) as b:
        b.feed(good + filler + b'chr1\t4\tCCC\t1\n')
        with pytest.raises(_lib.SegmentorError, match='byte offset %d' % (len(good) + len(filler))):
            b.finish()
    with _lib.Bimodal(s, e) as b:
        b.feed(good)
        b.feed(b'\n\n')
        b.feed(b'chr1\t2\tCCC\t1\n')
        with pytest.raises(_lib.SegmentorError, match='byte offset %d' % (len(good) + 2)):
            b.finish()
    for a, z in ((0, 3), (5, 5), (7, 6)):
        with pytest.raises(_lib.SegmentorError, match='startCpG'):
            _lib.Bimodal(np.array([a]), np.array([z]))
    # through the command line
    pat = str(tmp_path / 'u.pat.gz')
    with gzip.open(pat, 'wb') as f:
        f.write(good + b'chr1\t2\tCCC\t1\n')
    bed = tmp_path / 'b.bed'
    bed.write_text('chr1\t10\t20\t1\t5\n')
    g = str(tmp_path / 'g')
    BC.write_genome(g)
    with pytest.raises(Exception, match='not sorted'):
        test_bimodal.main([pat, '-L', str(bed), '--genome', g])


def test_output_file_and_verbose(genome, tmp_path, capsys):
    case = BC.CASES['L_all_rejected_printed']
    pat_text, bed_text, args = BC.case_inputs(case)
    pat = str(tmp_path / 's.pat.gz')
    with gzip.open(pat, 'wb') as f:
        f.write(pat_text)
    bed = tmp_path / 'b.bed'
    bed.write_text(bed_text)
    out = tmp_path / 'o.txt'
    assert wgbs_tools.main(['wgbstools', 'test_bimodal', pat, '-L', str(bed), '--genome', genome, '-o', str(out), '-v'] + args) == 0
    cap = capsys.readouterr()
    assert cap.out == ''
    assert cap.err.count('[wt bimodal] finished processesing') == len(BC.CHROMS)
    assert out.read_text().count('\n') == 6


def _feed_in_chunks(b, text, size):
    pos = 0
    while pos < len(text):
        cut = text.find(b'\n', min(len(text) - 1, pos + size - 1)) + 1
        b.feed(text[pos:cut])
        pos = cut


def test_column_terms_match_the_host_twin():
    """wg_bim_pair / wg_bim_ll0_term as the device evaluates them (fp64 IEEE division, wg_log2 on full-mantissa quotients, both of
    its branches) against the host build of the same expressions, all six outputs bit for bit on every pair of the lattice.  The
    host twin, not this machine's libm, is the yardstick: tests/test_bimodal_arith_cpu.py ties the twin to libm."""
    host = BL.load_host()
    names = ('pa / n', 'pb / n', 'log2(pa / n)', 'log2(pb / n)', 'n', 'll0 term')
    bad = dict.fromkeys(names, 0)
    first = {}
    pairs = 0
    t_dev = 0.0
    for name, a, b in BL.batches():
        t0 = time.time()
        got = _lib.debug_bimodal_terms(a, b)
        t_dev += time.time() - t0
        want = BL.host_terms(host, a, b)
        pairs += a.size
        for k, nm in enumerate(names):
            d = np.flatnonzero(got[k] != want[k])
            bad[nm] += d.size
            if d.size:
                first.setdefault(nm, (name, int(a[d[0]]), int(b[d[0]]), hex(int(got[k][d[0]])), hex(int(want[k][d[0]]))))
    print('bimodal column terms: %d pairs, %.2f s in the hook, mismatches %s' % (pairs, t_dev, bad))
    assert pairs == 8394753 + BL.N_RANDOM + 5 * 2001
    assert not any(bad.values()), (bad, first)


@pytest.mark.parametrize('chunk', ['whole', 4096, 300, 1])
@pytest.mark.parametrize('cols', [-1, 0, 16])
@pytest.mark.parametrize('name', sorted(BK.cases()))
def test_corner_cases_match_restatement(name, cols, chunk):
    """each hand-built corner (tests/test_bimodal_cpu.py checks that the case reaches it), on the default tables, with every block
    on global memory and with LDS tables of 16 columns; the text fed whole, in chunks of about 4 KB and 300 B, and one line per
    call (chunk 1: a retire and a drop between every two reads)"""
    c = BK.cases()[name]
    s, e = np.array(c['s']), np.array(c['e'])
    with _lib.Bimodal(s, e, c['strict'], c['min_len'], max_lds_cols=cols) as b:
        _feed_in_chunks(b, c['text'], len(c['text']) if chunk == 'whole' else chunk)
        ll, cnt = b.finish()
    want = BK.want(name)
    _same_bits(ll, cnt, want)
    for j, w in enumerate(want):                                  # (without rows _same_bits looks at the columns only)
        if w[4] == 0:
            assert ll[j].tolist() == [0.0, 0.0, 0.0] and int(cnt[j, 2]) == 0, (j, ll[j], cnt[j])


FIXED_SEEDS = tuple(range(20261016, 20261016 + 24))


def _fixed_draw(seed):
    """the draw of test_random_against_restatement from a fixed seed; every third seed is deep: 30 - 200 sites, a few blocks,
    hundreds of reads with counts up to a few thousand"""
    rng = np.random.default_rng(seed)
    deep = seed % 3 == 0
    n_sites = int(rng.integers(30, 200 if deep else 1500))
    nb = int(rng.integers(1, 5 if deep else 60))
    s = rng.integers(1, n_sites, nb)
    e = s + rng.integers(1, rng.choice([4, 30, 400]), nb)
    nr = int(rng.integers(100, 400)) if deep else int(rng.integers(1, 1500))
    st = np.sort(rng.integers(1, n_sites + 5, nr))
    ln = rng.integers(0, rng.choice([6, 30, 200]), nr)
    max_count = int(rng.choice([300, 3000])) if deep else 12
    alphabet = np.array(list('CCTT.H'))
    lines = ['chr1\t%d\t%s\t%d\n' % (st[i], ''.join(rng.choice(alphabet, ln[i])), rng.integers(0, max_count)) for i in range(nr)]
    text = ''.join(lines).encode()
    strict, min_len = bool(rng.integers(0, 2)), int(rng.integers(1, 4))
    return text, s, e, strict, min_len, int(rng.choice([-1, 0, 8])), int(rng.choice([200, 5000, len(text)]))


@pytest.mark.parametrize('seed', FIXED_SEEDS)
def test_fixed_seeds_against_restatement(seed):
    """the random comparison below on inputs that are the same for every run of a commit"""
    text, s, e, strict, min_len, cols, step = _fixed_draw(seed)
    with _lib.Bimodal(s, e, strict, min_len, max_lds_cols=cols) as b:
        _feed_in_chunks(b, text, step)
        ll, cnt = b.finish()
    _same_bits(ll, cnt, _want(text, s, e, strict, min_len))


def test_random_against_restatement():
    """seeded random reads and blocks (both options, chunked feeds), bit for bit, for at most ~25 s"""
    seed0 = int.from_bytes(os.urandom(4), 'little')
    print('bimodal random comparison: seeds from', seed0)
    t_end = time.time() + 25
    k = 0
    while time.time() < t_end and k < 100:
        rng = np.random.default_rng(seed0 + k)
        n_sites = int(rng.integers(30, 1500))
        nb = int(rng.integers(1, 60))
        s = rng.integers(1, n_sites, nb)
        e = s + rng.integers(1, rng.choice([4, 30, 400]), nb)
        nr = int(rng.integers(1, 1500))
        st = np.sort(rng.integers(1, n_sites + 5, nr))
        ln = rng.integers(0, rng.choice([6, 30, 200]), nr)
        alphabet = np.array(list('CCTT.H'))
        lines = ['chr1\t%d\t%s\t%d\n' % (st[i], ''.join(rng.choice(alphabet, ln[i])), rng.integers(0, 12)) for i in range(nr)]
        text = ''.join(lines).encode()
        strict, min_len = bool(rng.integers(0, 2)), int(rng.integers(1, 4))
        with _lib.Bimodal(s, e, strict, min_len, max_lds_cols=int(rng.choice([-1, 0, 8]))) as b:
            step = int(rng.choice([200, 5000, len(text)]))
            pos = 0
            while pos < len(text):
                cut = text.find(b'\n', min(len(text) - 1, pos + step - 1)) + 1
                b.feed(text[pos:cut])
                pos = cut
            ll, cnt = b.finish()
        _same_bits(ll, cnt, _want(text, s, e, strict, min_len))
        k += 1
    assert k > 0
