"""Every call that reads the resident (meth, cov) rows, on BORROWED rows laid out the hostile way (tests/borrowed_rows.py): the
tightest pitch include/wgbsseg.h allows — 2 n rounded up to 16 bytes, so the last 16-byte vector of a row holds up to 7 sites that
are not the row's — and no zeros anywhere around a row: pads and guards hold a poison ('ff00': meth 255, cov 0; '00ff': meth 0,
cov 255; 'random').  The library's own rows (wgbsseg_set_betas_host) have 256 bytes of slack behind every row that read as zero,
so a tail mask that is dropped, shifted by a vector or applied to one of the two counts only changes nothing there.

For every call, every size and every poison: the result equals the yardstick the suite uses for that call (the oracle,
oracle.block_sums, numpy's cumsum, stats_ref, compare_ref, bed_ref, array_ref, the reference's stitching tree over the oracle),
it is byte-identical to that of a second context holding the same rows through set_betas, and not one byte of the borrowed
buffer has changed afterwards.  No tolerance anywhere.

Sizes: every residue of n mod 8, and the tile / pass edges of the kernel in question -1, 0, +1, read from the plan headers:
8 sites a vector, 512 a DPP pass, 1024 a scan iteration and a window tile (WG_WIN_TILE), 896 / 1024 the general block-sum tile and
what it stages (WG_BS_TILE / WG_BS_EXT), 1024 x 8 the streaming tile and run (WG_BSR_TILE, WG_BSR_RUN), 8192 sites a statistics
tile (WG_ST_TILE vectors), 32768 a pair run (WG_PH_RUN), 256 a BED block (WG_BED_BLOCK).  N = 1, 3, 5 samples: the last sample group
of a kernel that takes 2 or 4 samples per wavefront or workgroup is partly filled.

Then the share windows (multi.segment_regions_on_shares over ONE whole-world buffer, where what lies behind a share's window is the
next sites of the same sample) at the size of the driver's golden worlds, on a roomy buffer and on the helper's."""
import functools
import os

import numpy as np
import pytest

import array_ref as AR
import bed_ref as BR
import borrowed_rows as BW
import compare_ref as CR
import reftree
import stats_ref as SR
from oracle import block_sums as OB
from oracle import oracle
from wgbs_tools_amd import _lib, multi, synth
from test_gpu_compare import _check as _pair_check            # pass 1, the edges, pass 2 against tests/compare_ref.py -> (ranges, counts)
from test_gpu_compare import _edges_from_ranges               # pass 2's edges from pass 1's result, by the product's rule
from test_gpu_driver import driver_golden, world              # noqa: F401  (fixtures: the driver's golden cases and their world on disk)

pytestmark = pytest.mark.gpu

SEED = 20261020
DEV = 'cuda:0'
POISONS = BW.ROW_POISONS
SAMPLES = (1, 3, 5)
THREADS = min(16, os.cpu_count() or 1)
RESIDUES = [1, 2, 7, 8, 9, 12, 13, 14, 15, 17]                 # n mod 8 = 1, 2, 7, 0, 1, 4, 5, 6, 7, 1; 3 comes with 4099
SCAN_SIZES = RESIDUES + [16, 255, 257, 511, 513, 1023, 1024, 1025, 1030, 2049, 4099, 8193]
BLOCK_SIZES = RESIDUES + [255, 257, 511, 513, 895, 896, 897, 1023, 1024, 1025, 1919, 1921, 2049, 4099, 8191, 8193, 9217]
STATS_SIZES = RESIDUES + [255, 257, 1023, 1025, 2047, 2049, 8191, 8192, 8193, 8199, 16385]
PAIR_SIZES = RESIDUES + [255, 257, 2047, 2049, 4099, 32767, 32768, 32769, 32775]
BED_SIZES = RESIDUES + [255, 256, 257, 511, 513, 1025, 4099]


@functools.lru_cache(maxsize=None)
def _rows(n, N):
    """N samples of n sites: the synthetic rows of the other GPU modules, a few sites saturated at 255, and first and last sites that
    are not zero in either count (a tail that loses its last site must show)"""
    rows = []
    for s in range(N):
        r = synth.synth_betas(SEED, s, 0, n).copy()
        if n > 40:
            r[n // 3:n // 3 + 3, :] = 255
            r[n - 5:n - 3, :] = 255
        r[0] = (s, 9 + s)
        r[n - 1] = (17 * s + 1, 255 - s)
        rows.append(r)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def _loci(n, dense):
    if not dense:
        return synth.synth_loci(SEED, [n])
    return (np.cumsum(np.random.default_rng([SEED, n]).integers(1, 4, n)) + 5000).astype(np.uint32)      # ~2 bp apart: max_cpg bounds every window


_MEMO = {}


def _once(key, make):
    """yardsticks and the twin context's results: computed once, shared by the three poisons"""
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


@pytest.fixture(scope='module')
def seg():
    with _lib.Segmenter(0) as s:
        yield s


@pytest.fixture(scope='module')
def twin():
    """the second context: the same rows through set_betas, in the library's own roomy, zero-padded rows"""
    with _lib.Segmenter(0) as s:
        yield s


@pytest.fixture(scope='module')
def general_pair():
    """(borrowing context, twin) with WGBSSEG_BLOCK_SUMS_GENERAL = 0 and = 1 (read when a context is created)"""
    made = {}
    for flag in (0, 1):
        os.environ['WGBSSEG_BLOCK_SUMS_GENERAL'] = str(flag)
        try:
            made[flag] = (_lib.Segmenter(0), _lib.Segmenter(0))
        finally:
            del os.environ['WGBSSEG_BLOCK_SUMS_GENERAL']
    yield made
    for a, b in made.values():
        a.close()
        b.close()


def _borrow(sg, n, N, poison, pitch=None):
    b = BW.BorrowedRows(_rows(n, N), poison, DEV, pitch=pitch, seed=n)
    sg.set_betas_device(b.ptr, N, b.pitch, n, keepalive=b)
    return b


def _same_lists(got, want, what):
    assert len(got) == len(want), what
    for c, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)), (what, 'item', c, np.asarray(a)[:12], np.asarray(b)[:12])


# ---------------------------------------------------------------------------------------------------------
# the layout really is the hostile one, on the device too
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('poison', POISONS)
def test_helper_on_the_device(poison):
    n, N = 13, 3
    b = BW.BorrowedRows(_rows(n, N), poison, DEV)
    assert b.ptr % 16 == 0 and b.pitch == 32 and b.buf.is_cuda and b.buf.dim() == 1
    now = b.bytes_now()
    for s in range(N):
        assert np.array_equal(now[b.row0 + s * b.pitch:b.row0 + s * b.pitch + 2 * n], _rows(n, N)[s].reshape(-1))
    b.assert_untouched()
    b.buf[b.row0 + 2 * n] ^= 1                                    # the first pad byte
    with pytest.raises(AssertionError, match='pad behind row 0'):
        b.assert_untouched()


# ---------------------------------------------------------------------------------------------------------
# k_scan + k_prefix_materialise
# ---------------------------------------------------------------------------------------------------------
def _prefix_ranges(n):
    r = {(0, n), (n - 1, 1), (n - min(n, 9), min(n, 9)), (n - min(n, 700), min(n, 700)), (n // 3, n - n // 3), (min(3, n - 1), max(1, n // 2))}
    return sorted((a, l) for a, l in r if l >= 1 and a + l <= n)


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n', SCAN_SIZES + [8191])
def test_prefix_sums(seg, twin, n, poison):
    for N in SAMPLES:
        rows = _rows(n, N)
        b = _borrow(seg, n, N, poison)
        ranges = _prefix_ranges(n)
        assert (0, n) in ranges and any(a > 0 and a + l == n for a, l in ranges) or n == 1

        def reference():
            twin.set_betas(rows)
            return [twin.prefix_sums(a, l).tobytes() for a, l in ranges]
        same = _once(('prefix', n, N), reference)
        for (a, l), tw in zip(ranges, same):
            got = seg.prefix_sums(a, l)
            for s in range(N):
                want = np.zeros((l + 1, 2), dtype=np.uint32)
                want[1:] = np.cumsum(rows[s][a:a + l].astype(np.uint32), axis=0)
                assert np.array_equal(got[s], want), (n, N, poison, a, l, 'sample', s)
            assert got.tobytes() == tw, (n, N, poison, a, l)
        b.assert_untouched()


# ---------------------------------------------------------------------------------------------------------
# k_validate / k_scan, k_window, the three row stagings of k_cost (narrow, medium, wide tiles), recurrence, trace
# ---------------------------------------------------------------------------------------------------------
# (pcount, max_cpg, max_bp, dense loci): default parameters on the synthetic genome (narrow tiles), and on loci ~2 bp apart windows
# of 40 (narrow: windows <= 60), 200 (medium: 61 .. 252) and 300 sites (wide: scored from the carries of k_scan)
SEG_PARAMS = [(15.0, 1000, 2000, False), (15.0, 40, 10 ** 6, True), (1.0, 200, 10 ** 6, True), (0.5, 300, 10 ** 6, True)]


def _chunks(n):
    """[0, n), chunks that end on the last resident site, and a ragged set (one starts on site 0)"""
    c = [(0, n)] + [(n - k, k) for k in (1, 2, 9, 64, 65, 100, 301, 1000) if k < n]
    c += [(0, max(1, n // 2)), (n // 5, max(1, n // 2)), (min(7, n - 1), max(1, (n - min(7, n - 1)) // 3)), (n // 2, n - n // 2)]
    return [a for a, _ in c], [l for _, l in c]


def _segment_chunks_case(seg, twin, n, poison, set_loci, tag):
    starts, lens = _chunks(n)
    for N in SAMPLES:
        rows = _rows(n, N)
        b = _borrow(seg, n, N, poison)
        for pcount, max_cpg, max_bp, dense in SEG_PARAMS:
            loci = _loci(n, dense)
            held = set_loci(seg, loci)

            def reference():
                twin.set_betas(rows)
                twin.set_loci(loci)
                return (oracle.segment_chunks(rows, loci, starts, lens, pcount, max_cpg, max_bp, threads=THREADS),
                        twin.segment_chunks(starts, lens, pcount, max_cpg, max_bp))
            want, same = _once(('chunks', n, N, max_cpg, dense), reference)
            got = seg.segment_chunks(starts, lens, pcount, max_cpg, max_bp)
            _same_lists(got, want, (tag, n, N, poison, max_cpg, 'oracle'))
            _same_lists(got, same, (tag, n, N, poison, max_cpg, 'twin'))
            if held is not None:
                held.assert_untouched()
        b.assert_untouched()


def _host_loci(sg, loci):
    sg.set_loci(loci)


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n', SCAN_SIZES)
def test_segment_chunks(seg, twin, n, poison):
    _segment_chunks_case(seg, twin, n, poison, _host_loci, 'host loci')


def _region_chunk(n):
    """a chunk size that leaves a short last chunk"""
    return 60 if n < 200 else (100 if n < 1000 else 2 * n // 5 + 1)


def _segment_regions_case(seg, twin, n, poison, set_loci, tag):
    chunk = _region_chunk(n)
    assert n % chunk != 0 or n < chunk
    for N in SAMPLES:
        rows = _rows(n, N)
        b = _borrow(seg, n, N, poison)
        for pcount, max_cpg, max_bp, dense in SEG_PARAMS[:1] + SEG_PARAMS[2:3]:
            max_cpg = min(max_cpg, chunk)
            loci = _loci(n, dense)
            held = set_loci(seg, loci)

            def reference():
                def many(sites):             # 1-based half-open site ranges -> absolute border lists
                    return [oracle.segment_chunk([r[a - 1:e - 1] for r in rows], loci[a - 1:e - 1], pcount, max_cpg, max_bp).astype(np.int64) + a for a, e in sites]
                grid = [(a, min(a + chunk, n + 1)) for a in range(1, n + 1, chunk)]
                twin.set_betas(rows)
                twin.set_loci(loci)
                return reftree.tree(many(grid), many), twin.segment_regions([1], [n + 1], chunk, pcount, max_cpg, max_bp)[0][0]
            want, same = _once(('regions', n, N, max_cpg, dense), reference)
            got = seg.segment_regions([1], [n + 1], chunk, pcount, max_cpg, max_bp)[0][0]
            assert got[0] == 1 and got[-1] == n + 1
            assert np.array_equal(got, want), (tag, n, N, poison, max_cpg, 'reference tree over the oracle')
            assert np.array_equal(got, same), (tag, n, N, poison, max_cpg, 'twin')
            if held is not None:
                held.assert_untouched()
        b.assert_untouched()


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n', SCAN_SIZES)
def test_segment_regions(seg, twin, n, poison):
    _segment_regions_case(seg, twin, n, poison, _host_loci, 'host loci')


# ---- the same two with the loci borrowed as well: k_window's 16-byte loads of the loci ----
LOCI_SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 13, 1023, 1024, 1025, 1027, 2049, 4099]      # every residue mod 4 (a loci vector), WG_WIN_TILE -1, 0, +1, +3


def _borrowed_loci(poison, phase):
    def set_loci(sg, loci):
        held = BW.BorrowedLoci(loci, poison, DEV, phase_words=phase)
        sg.set_loci_device(held.ptr, held.n, keepalive=held)
        return held
    return set_loci


@pytest.mark.parametrize('loci_poison', BW.LOCI_POISONS)
@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n', LOCI_SIZES)
def test_segment_chunks_with_borrowed_loci(seg, twin, n, poison, loci_poison):
    """every 4-byte phase of the loci's address against the 16-byte grid: what include/wgbsseg.h allows"""
    for phase in range(4):
        _segment_chunks_case(seg, twin, n, poison, _borrowed_loci(loci_poison, phase), 'borrowed loci, phase %d' % phase)


@pytest.mark.parametrize('loci_poison', BW.LOCI_POISONS)
@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n', LOCI_SIZES)
def test_segment_regions_with_borrowed_loci(seg, twin, n, poison, loci_poison):
    _segment_regions_case(seg, twin, n, poison, _borrowed_loci(loci_poison, (n + len(poison)) % 4), 'borrowed loci')


# ---------------------------------------------------------------------------------------------------------
# the block reduction: k_block_sums (general), k_block_sums_prep / _run / _direct (streaming)
# ---------------------------------------------------------------------------------------------------------
def _block_tables(n):
    """block_plan.h: a table ordered by first AND last site (after the host's stable sort by first site) takes the streaming kernels
    (prep, run; direct for a block that begins more than a tile before the tile it ends in, or before its run); any other the
    general one.  WGBSSEG_BLOCK_SUMS_GENERAL=1 sends every table through the general kernel."""
    rng = np.random.default_rng([SEED, n, 7])
    edges = [m + d for tile in (896, 1024) for m in range(tile, n, tile) for d in (-1, 0, 1)]
    cuts = np.unique(np.concatenate([[0, n], rng.integers(0, n + 1, min(n, 60)), [e for e in edges if 0 < e < n]])).astype(np.int64)
    t = {}
    t['tiling'] = (cuts[:-1], cuts[1:])                                            # ordered: streaming; the last block ends on the last site
    t['ends'] = (np.array([n - 1, 0]), np.array([n, 1]))                           # one-site blocks at n - 1 and 0, in that order (sorted by the host: streaming)
    t['whole'] = (np.array([0]), np.array([n]))                                    # streaming: the ring up to a tile, k_block_sums_direct beyond
    st = np.arange(0, n, max(1, n // 50))
    t['ordered_overlaps'] = (np.concatenate([st, [n - 1, n]]), np.concatenate([np.minimum(st + n // 2 + 1, n), [n, n]]))   # ordered by both, long overlapping blocks that end on n
    un = [(n // 2, n), (0, n), (min(3, n - 1), max(n - 3, min(3, n - 1))), (min(5, n - 1), n), (n - 1, n), (0, 0), (n, n), (0, 1), (n // 3, n - n // 5)]
    un += [(int(a), int(min(a + l, n))) for a, l in zip(rng.integers(0, n, 20), rng.integers(0, n + 1, 20))]
    o = rng.permutation(len(un))
    t['unsorted'] = (np.array([un[i][0] for i in o]), np.array([un[i][1] for i in o]))      # nested, overlapping, unordered: the general kernel, tails from memory
    return {k: (np.asarray(a, dtype=np.int64), np.asarray(e, dtype=np.int64)) for k, (a, e) in t.items()}


def _all_modes(sg, s0, e0):
    return [sg.block_sums(s0, e0, mode=0), sg.block_sums(s0, e0, mode=1), sg.block_sums(s0, e0, mode=2), sg.block_sums(s0, e0, mode=3, min_cov=1),
            sg.block_sums(s0, e0, mode=3, min_cov=3)]


@pytest.mark.parametrize('general', [0, 1])
@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n', BLOCK_SIZES)
def test_block_sums(general_pair, n, poison, general):
    sg, tw = general_pair[general]
    tables = _block_tables(n)
    assert (np.diff(tables['tiling'][0]) >= 0).all() and (np.diff(tables['tiling'][1]) >= 0).all() and tables['tiling'][1][-1] == n and tables['tiling'][0][0] == 0
    assert (np.diff(tables['ordered_overlaps'][0]) >= 0).all() and (np.diff(tables['ordered_overlaps'][1]) >= 0).all()
    assert (np.diff(tables['unsorted'][0]) < 0).any()
    for N in SAMPLES:
        rows = _rows(n, N)
        b = _borrow(sg, n, N, poison)
        for name, (s0, e0) in tables.items():
            def reference():
                tw.set_betas(rows)
                return [OB.block_sums(r, s0, e0) for r in rows], [g.tobytes() for g in _all_modes(tw, s0, e0)]
            want, same = _once(('blocks', n, N, general, name), reference)
            got = _all_modes(sg, s0, e0)
            what = (name, n, N, poison, general)
            for s, w in enumerate(want):
                bad = np.flatnonzero((got[0][s].astype(np.int64) != w).any(1))
                assert bad.size == 0, '%s sample %d: block %d = [%d, %d): got %s want %s' % (what, s, bad[0], s0[bad[0]], e0[bad[0]], got[0][s][bad[0]], w[bad[0]])
                assert np.array_equal(got[1][s], OB.trim(w, False)) and np.array_equal(got[2][s], OB.trim(w, True)), (what, s)
                for g3, mc in ((got[3], 1), (got[4], 3)):
                    w3 = OB.beta2vec(w, mc)
                    assert np.array_equal(np.isnan(g3[s]), np.isnan(w3)), (what, s, mc)
                    assert np.array_equal(g3[s][~np.isnan(w3)].view(np.uint64), w3[~np.isnan(w3)].view(np.uint64)), (what, s, mc)
            assert [g.tobytes() for g in got] == same, what
        b.assert_untouched()


# ---------------------------------------------------------------------------------------------------------
# k_sample_stats
# ---------------------------------------------------------------------------------------------------------
def _stat_ranges(n):
    sets = {'whole': [(0, n)], 'last_site': [(n - 1, n)], 'first_site': [(0, 1)]}
    cuts = sorted({0, 1, n // 3, n // 3 + 1, n // 2, max(0, n - 9), n - 1, n})
    sets['pieces'] = [(a, e) for a, e in zip(cuts[:-1], cuts[1:])][::2] + ([(cuts[-2], n)] if len(cuts) % 2 == 1 else [])
    sets['pieces'] = sorted(set(sets['pieces']))
    sets['tail'] = [(max(0, n - 9), n)]
    return sets


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n', STATS_SIZES)
def test_sample_stats(seg, twin, n, poison):
    sets = _stat_ranges(n)
    assert all(r[-1][1] == n for k, r in sets.items() if k != 'first_site')
    for N in SAMPLES:
        rows = _rows(n, N)
        b = _borrow(seg, n, N, poison)
        for name, ranges in sets.items():
            def reference():
                twin.set_betas(rows)
                return [SR.expect(r, ranges, 10) for r in rows], twin.sample_stats(ranges).tobytes()
            want, same = _once(('stats', n, N, name), reference)
            got = seg.sample_stats(ranges)
            assert [SR.as_dict(g) for g in got] == want, (name, n, N, poison)
            assert got.tobytes() == same, (name, n, N, poison)
        b.assert_untouched()


# ---------------------------------------------------------------------------------------------------------
# k_pair_ranges, k_pair_hist
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('corners', ['0', '1'])
@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n', PAIR_SIZES)
def test_pair_ranges_and_hist(seg, twin, n, poison, corners, monkeypatch):
    monkeypatch.setenv('WGBSSEG_PAIR_CORNERS', corners)
    N = 3
    rows = list(_rows(n, N))
    pairs = CR.all_pairs(N)
    b = _borrow(seg, n, N, poison)
    for min_cov, bins in ((1, 7), (3, 101)):
        got, counts = _pair_check(seg, rows, pairs, min_cov, bins, (n, poison, corners, min_cov, bins))       # against tests/compare_ref.py

        def reference():
            twin.set_betas(rows)
            r = twin.pair_ranges(pairs, min_cov)
            return r.tobytes(), twin.pair_hist(pairs, min_cov, bins, _edges_from_ranges(r, bins)).tobytes()
        same = _once(('pairs', n, corners, min_cov, bins), reference)
        assert (got.tobytes(), counts.tobytes()) == same, (n, poison, corners, min_cov, bins)
    b.assert_untouched()


# ---------------------------------------------------------------------------------------------------------
# beta2bed, site_counts, site_table
# ---------------------------------------------------------------------------------------------------------
def _to_file(tmp_path, call):
    path = str(tmp_path / 'out.txt')
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        counted = call(fd)
    finally:
        os.close(fd)
    with open(path, 'rb') as f:
        return f.read(), counted


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n', BED_SIZES)
def test_beta2bed(seg, twin, n, poison, tmp_path):
    names, sizes = (['chrA', 'chrB'], [n // 2, n - n // 2]) if n > 1 else (['chrA'], [1])
    loci = synth.synth_loci(SEED, sizes)
    a0 = max(0, n - 700)                                              # the last site is among those asked for
    for N in SAMPLES:
        rows = _rows(n, N)
        b = _borrow(seg, n, N, poison)
        seg.set_loci(loci)
        for sample in sorted({0, N - 1}):
            for o in (dict(), dict(mean=True, keep_na=True), dict(min_cov=5, slab_sites=256)):
                ref_o = {k: v for k, v in o.items() if k != 'slab_sites'}

                def reference():
                    twin.set_betas(rows)
                    twin.set_loci(loci)
                    return (BR.text_of(names, sizes, loci, rows[sample], a0, n, **ref_o),
                            _to_file(tmp_path, lambda fd: twin.beta2bed(fd, sample, names, np.cumsum(sizes), start0=a0, end0=n, **o)))
                want, same = _once(('bed', n, N, sample, tuple(sorted(o.items()))), reference)
                got = _to_file(tmp_path, lambda fd: seg.beta2bed(fd, sample, names, np.cumsum(sizes), start0=a0, end0=n, **o))
                assert got[0] == want and got[1] == (want.count(b'\n'), len(want)), (n, N, poison, sample, o)
                assert got == same, (n, N, poison, sample, o)
        b.assert_untouched()


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n', BED_SIZES)
def test_site_counts_and_table(seg, twin, n, poison, tmp_path):
    rng = np.random.default_rng([SEED, n, 11])
    site0 = np.concatenate([[n - 1, 0, n // 2, n - 1], rng.integers(0, n, 40), np.arange(max(0, n - 9), n)]).astype(np.int64)
    labels = [b'cg%07d' % i for i in range(site0.size)]
    for N in SAMPLES:
        rows = _rows(n, N)
        cols = list(range(N))[::-1]
        b = _borrow(seg, n, N, poison)

        def reference():
            twin.set_betas(rows)
            return (twin.site_counts(site0, cols).tobytes(), _to_file(tmp_path, lambda fd: twin.site_table(fd, site0, cols, labels, min_cov=3, slab_rows=16)))
        same = _once(('sites', n, N), reference)
        got = seg.site_counts(site0, cols)
        assert got.dtype == np.uint16 and np.array_equal(got, np.stack([rows[s][site0] for s in cols], axis=1)), (n, N, poison)
        want = AR.table_body([x.decode() for x in labels], site0, [rows[s] for s in cols], 3)
        text = _to_file(tmp_path, lambda fd: seg.site_table(fd, site0, cols, labels, min_cov=3, slab_rows=16))
        assert text == (want, (site0.size, len(want))), (n, N, poison)
        assert (got.tobytes(), text) == same, (n, N, poison)
        b.assert_untouched()


# ---------------------------------------------------------------------------------------------------------
# what the two borrowing calls refuse, and that a refusal leaves the context as it was
# ---------------------------------------------------------------------------------------------------------
def test_set_betas_device_refusals(seg):
    n, N = 1025, 3
    rows = _rows(n, N)
    loci = _loci(n, False)
    good = BW.BorrowedRows(rows, 'ff00', DEV)
    roomy = BW.BorrowedRows(rows, 'ff00', DEV, pitch=good.pitch + 32)
    seg.set_betas_device(good.ptr, N, good.pitch, n, keepalive=good)
    seg.set_loci(loci)
    want = seg.segment_chunks([0], [n], 15.0, 1000, 2000)[0].tolist()
    sums = seg.block_sums([0], [n]).tobytes()
    refused = [('base not a multiple of 16', (roomy.ptr + 8, N, roomy.pitch, n)), ('base not a multiple of 16', (roomy.ptr + 1, N, roomy.pitch, n)),
               ('pitch not a multiple of 16', (roomy.ptr, N, roomy.pitch - 8, n)), ('pitch not a multiple of 16', (roomy.ptr, N, roomy.pitch - 31, n)),
               ('pitch < 2 n', (good.ptr, N, good.pitch - 16, n)), ('pitch < 2 n', (good.ptr, N, 0, n)),
               ('n_samples < 1', (good.ptr, 0, good.pitch, n)), ('n_samples < 1', (good.ptr, -1, good.pitch, n))]
    assert roomy.pitch - 8 >= 2 * n and roomy.pitch - 31 >= 2 * n and good.pitch - 16 < 2 * n
    for why, (ptr, ns, pitch, sites) in refused:
        with pytest.raises(_lib.SegmentorError) as e:
            seg.set_betas_device(ptr, ns, pitch, sites)
        assert e.value.code == _lib.E_ARG, why
        # the context still holds the rows it had, and works
        assert seg.segment_chunks([0], [n], 15.0, 1000, 2000)[0].tolist() == want, why
        assert seg.block_sums([0], [n]).tobytes() == sums, why
    good.assert_untouched()
    roomy.assert_untouched()


def test_set_loci_device_takes_any_whole_entry_and_refuses_the_rest(seg):
    """include/wgbsseg.h: the loci must be a multiple of 4 bytes, nothing more; anything else is WGBSSEG_E_ARG and the context keeps
    the loci it had"""
    n, N = 1027, 3
    rows = _rows(n, N)
    loci = _loci(n, False)
    b = _borrow(seg, n, N, 'random')
    seg.set_loci(loci)
    want = oracle.segment_chunks(rows, loci, [0, n - 100], [n, 100], 15.0, 1000, 2000)
    _same_lists(seg.segment_chunks([0, n - 100], [n, 100], 15.0, 1000, 2000), want, 'host loci')
    for phase in range(4):
        held = BW.BorrowedLoci(loci, 'ffffffff', DEV, phase_words=phase)
        assert held.ptr % 16 == 4 * phase
        seg.set_loci_device(held.ptr, n, keepalive=held)
        _same_lists(seg.segment_chunks([0, n - 100], [n, 100], 15.0, 1000, 2000), want, ('phase', phase))
        for off in (1, 2, 3):
            with pytest.raises(_lib.SegmentorError) as e:
                seg.set_loci_device(held.ptr + off, n - 1)
            assert e.value.code == _lib.E_ARG and '4 bytes' in e.value.msg
            _same_lists(seg.segment_chunks([0, n - 100], [n, 100], 15.0, 1000, 2000), want, ('after a refusal', phase, off))
        for bad_n in (0, -1):
            with pytest.raises(_lib.SegmentorError) as e:
                seg.set_loci_device(held.ptr, bad_n)
            assert e.value.code == _lib.E_ARG
        held.assert_untouched()
    with pytest.raises(_lib.SegmentorError) as e:
        seg.set_loci_device(0, n)
    assert e.value.code == _lib.E_ARG
    b.assert_untouched()


# ---------------------------------------------------------------------------------------------------------
# share windows: what lies behind a share's rows is the next sites of the same sample
# ---------------------------------------------------------------------------------------------------------
SHARE_CASES = ['wg_c20000', 'tiny_chunks', 'bed_regions']


def _share_world(driver_golden, world, name):
    """rows, loci, regions, parameters and the reference driver's (start, end) columns of a golden case.  tiny_chunks segments the
    sites 20000 .. 20999 only: its world is cut behind them (regions never interact, segment.py:129-134), so that its last chunk
    ends on the last resident site like the other two's."""
    g = driver_golden['cases'][name]
    total = int(sum(world['sizes']))
    rows = [np.fromfile(p, dtype=np.uint8).reshape(-1, 2) for p in world['paths']]
    loci = world['loci']
    seen, regions = set(), []
    for tag in g['chunks']['tags']:
        if tag not in seen:
            seen.add(tag)
            regions.append(tuple(int(x) for x in tag.split('-')))
    n = total
    if name == 'tiny_chunks':
        n = regions[-1][1] - 1
        rows, loci = [r[:n] for r in rows], loci[:n]
    assert regions[-1][1] - 1 == n or name == 'bed_regions'
    a = g['args']
    p = dict(chunk_size=a['chunk_size'], pcount=float(a.get('pcount', 15)), max_cpg=a.get('max_cpg', 1000), max_bp=a.get('max_bp', 2000))
    assert a.get('min_cpg', 1) == 1
    return rows, loci, n, regions, p, np.array(g['start_cpg'], dtype=np.int64), np.array(g['end_cpg'], dtype=np.int64)


def _columns(borders):
    """the (start, end) columns of the blocks of every region's border list (segment.py:154)"""
    return np.concatenate([np.asarray(b)[:-1] for b in borders]), np.concatenate([np.asarray(b)[1:] for b in borders])


def _shares_case(driver_golden, world, name, n_shares, make_buffer):
    rows, loci, n, regions, p, want_s, want_e = _share_world(driver_golden, world, name)
    N = len(rows)
    held, ptr, pitch, check = make_buffer(rows, n)
    st, en = np.array([r[0] for r in regions]), np.array([r[1] for r in regions])
    with _lib.Segmenter(0) as one:                                                   # one context over the whole buffer
        one.set_betas_device(ptr, N, pitch, n, keepalive=held)
        one.set_loci(loci)
        whole, _ = one.segment_regions(st, en, p['chunk_size'], p['pcount'], p['max_cpg'], p['max_bp'])
    got, stats, grp = multi.segment_regions_on_shares(ptr, N, pitch, n, loci, regions, p['chunk_size'], p['pcount'], p['max_cpg'], p['max_bp'],
                                                      [0] * n_shares, keepalive=held, want_group=True)
    try:
        w = grp.windows
        busy = w['chunks'] > 0                                                        # (a share may be left without chunks: it borrows nothing)
        assert busy.sum() >= 2 and int(w['chunks'].sum()) == len(driver_golden['cases'][name]['chunks']['starts'])
        assert (w['win_lo'][busy] % 128 == 0).all() and int(w['win_hi'][busy].max()) == n, 'no share window ends on the last site of the world'
        # ... and around the other windows lie real sites of the same sample (tiny_chunks: in front only, its halo reaches the end from every share)
        assert (w['win_lo'][busy] > 0).any() and ((w['win_hi'][busy] < n).any() or name == 'tiny_chunks')
    finally:
        grp.close()
    _same_lists(got, whole, (name, n_shares, 'one context'))
    s, e = _columns(got)
    assert np.array_equal(s, want_s) and np.array_equal(e, want_e), (name, n_shares, 'the reference driver')
    check()


def _roomy(rows, n):
    import torch
    pitch = ((2 * n + 255) // 256) * 256 + 256
    host = np.zeros((len(rows), pitch), dtype=np.uint8)
    for s, r in enumerate(rows):
        host[s, :2 * n] = r.reshape(-1)
    buf = torch.from_numpy(host).to(DEV)
    return buf, buf.data_ptr(), pitch, lambda: None


@pytest.mark.parametrize('n_shares', [3, 5])
@pytest.mark.parametrize('name', SHARE_CASES)
def test_share_windows_over_one_buffer(driver_golden, world, name, n_shares):
    _shares_case(driver_golden, world, name, n_shares, _roomy)


@pytest.mark.parametrize('poison', POISONS)
@pytest.mark.parametrize('n_shares', [3, 5])
@pytest.mark.parametrize('name', SHARE_CASES)
def test_share_windows_over_a_tight_poisoned_buffer(driver_golden, world, name, n_shares, poison):
    def tight(rows, n):
        b = BW.BorrowedRows(rows, poison, DEV, seed=n_shares)
        assert b.pitch - 2 * n < 16
        return b, b.ptr, b.pitch, b.assert_untouched
    _shares_case(driver_golden, world, name, n_shares, tight)
