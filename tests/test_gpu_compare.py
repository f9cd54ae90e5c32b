"""Pairwise 2-D histograms on the GPU (k_pair_ranges and k_pair_hist behind wgbsseg_pair_ranges / wgbsseg_pair_hist): everything
against the numpy restatement tests/compare_ref.py as integers and exact doubles, over the sizes, sample counts, row widths,
bins and thresholds of tests/compare_cases.py; the worlds that take the kernels' special paths; bit-identical repeats and the
two forms of corner handling; the refusals; `compare_betas.pair_histograms` and the command's .npz end to end against
np.histogram2d per pair."""
import os.path as op

import numpy as np
import pytest

import compare_cases as CC
import compare_ref as CR
from wgbs_tools_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def seg():
    with _lib.Segmenter(0) as s:
        yield s


@pytest.fixture(scope='module')
def limits():
    return _lib.pair_hist_limits()


def _load(seg, rows, elem):
    (seg.set_betas if elem == 1 else seg.set_lbetas)(CC.flat(rows))


def _edges(rows, pairs, min_cov, bins):
    """[n_pairs, 2, bins + 1] from the restatement"""
    e = np.empty((len(pairs), 2, bins + 1))
    for k, (a, b) in enumerate(pairs):
        x, y = CR.values(rows[a], rows[b], min_cov)
        e[k, 0], e[k, 1] = CR.axis_edges(x, bins), CR.axis_edges(y, bins)
    return e


def _edges_from_ranges(got, bins):
    """[n_pairs, 2, bins + 1] from pass 1's result, by the rule the product's host code follows"""
    e = np.empty((len(got), 2, bins + 1))
    for k, g in enumerate(got):
        for ax, (lo, hi) in enumerate(((g['b_min'], g['b_max']), (g['a_min'], g['a_max']))):
            lo, hi = (0.0, 1.0) if g['n'] == 0 else (float(lo), float(hi))
            if lo == hi:
                lo, hi = lo - 0.5, hi + 0.5
            e[k, ax] = np.linspace(lo, hi, bins + 1)
    return e


def _check(seg, rows, pairs, min_cov, bins, what):
    got = seg.pair_ranges(pairs, min_cov)
    assert len(got) == len(pairs)
    for k, (a, b) in enumerate(pairs):
        want = CR.pair_range(rows[a], rows[b], min_cov)
        assert {f: (int(got[k][f]) if f == 'n' else float(got[k][f])) for f in want} == want, (what, 'pair', (a, b))
    edges = _edges_from_ranges(got, bins)
    assert edges.tobytes() == _edges(rows, pairs, min_cov, bins).tobytes(), what
    counts = seg.pair_hist(pairs, min_cov, bins, edges)
    assert counts.dtype == np.uint64 and counts.shape == (len(pairs), bins, bins)
    for k, (a, b) in enumerate(pairs):
        want, xe, ye = CR.hist(rows[a], rows[b], min_cov, bins)
        assert np.array_equal(counts[k], want), (what, 'pair', (a, b))
        assert int(counts[k].sum()) == int(got[k]['n'])
    return got, counts


def _sizes(limits):
    return CC.SIZES + (2 * limits[1] + 3,)


@pytest.mark.parametrize('elem', [1, 2])
@pytest.mark.parametrize('n_index', range(5))
def test_all_pairs_match_restatement(seg, limits, n_index, elem):
    n = _sizes(limits)[n_index]
    rows = CC.world(n, 5, elem)
    for n_samples in CC.SAMPLES:
        _load(seg, rows[:n_samples], elem)
        _check(seg, rows, CR.all_pairs(n_samples), 10, 7, (n, n_samples, elem))


@pytest.mark.parametrize('elem', [1, 2])
def test_explicit_pair_list(seg, elem):
    """a pair twice, a pair and its reverse, the diagonal"""
    rows = CC.world(4097, 5, elem, seed=1)
    _load(seg, rows, elem)
    pairs = [(1, 0), (0, 1), (1, 0), (4, 4), (3, 1), (1, 3), (2, 0)]
    got, counts = _check(seg, rows, pairs, 5, 7, elem)
    assert np.array_equal(counts[0], counts[2]) and np.array_equal(counts[0], counts[1].T)
    assert got[0] == got[2]


@pytest.mark.parametrize('elem', [1, 2])
@pytest.mark.parametrize('bins_index', range(5))
def test_bins(seg, limits, bins_index, elem):
    bins = (CC.BINS + (limits[0],))[bins_index]
    rows = CC.world(70001, 3, elem, seed=2)
    _load(seg, rows, elem)
    _check(seg, rows, CR.all_pairs(3), 10, bins, (bins, elem))


def test_bins_limit_is_what_lds_holds(limits):
    max_bins, run = limits
    assert max_bins >= 101 and run >= 1
    lds = lambda b: 4 * b * b + 2 * 8 * (b + 1)
    assert lds(max_bins) <= 65536 < lds(max_bins + 1)


@pytest.mark.parametrize('elem, min_cov', [(1, 1), (1, 10), (1, 255), (1, 256), (2, 1), (2, 10), (2, 255), (2, 256), (2, 1001), (2, 70000)])
def test_min_cov(seg, elem, min_cov):
    """(1, 256) and (2, 1001), (2, 70000) lie above every coverage of the world: every pair is empty"""
    rows = CC.world(4097, 5, elem, seed=3)
    _load(seg, rows, elem)
    got, _ = _check(seg, rows, CR.all_pairs(5), min_cov, 7, (elem, min_cov))
    if (elem, min_cov) in ((1, 256), (2, 1001), (2, 70000)):
        assert not got['n'].any()
    if (elem, min_cov) in ((1, 255), (2, 256)):
        assert got['n'][0] > 0                      # (some sites of sample 0 are that deep: the case is not empty)


@pytest.mark.parametrize('elem', [1, 2])
def test_bimodal_world_takes_the_corner_path(seg, elem):
    rows = CC.bimodal(70001, elem)
    _load(seg, rows, elem)
    _, counts = _check(seg, rows, CR.all_pairs(2), 10, 101, elem)
    c = counts[1]
    assert int(c[0, 0]) + int(c[-1, -1]) >= 0.9 * int(c.sum())


@pytest.mark.parametrize('elem', [1, 2])
def test_constant_identical_and_uncovered_samples(seg, elem):
    rows = CC.world(4097, 5, elem, seed=4)
    _load(seg, rows, elem)
    pairs = CR.all_pairs(5)
    got, counts = _check(seg, rows, pairs, 4, 7, elem)
    edges = _edges_from_ranges(got, 7)
    for k, (a, b) in enumerate(pairs):
        if 2 in (a, b):                              # the sample without coverage: range (0, 1), nothing counted
            assert got[k]['n'] == 0 and not counts[k].any()
            assert edges[k, 0, 0] == 0.0 and edges[k, 0, -1] == 1.0 and edges[k, 1, 0] == 0.0 and edges[k, 1, -1] == 1.0
        elif a == 3:                                 # the constant sample on y: the +-0.5 range
            assert got[k]['a_min'] == got[k]['a_max'] == 0.25 and edges[k, 1, 0] == -0.25 and edges[k, 1, -1] == 0.75
    k = pairs.index((4, 0))                          # two identical samples: everything on the diagonal
    assert int(np.trace(counts[k])) == int(got[k]['n']) > 0


@pytest.mark.parametrize('elem', [1, 2])
def test_meth_above_cov(seg, elem):
    rows = CC.over(4097, elem)
    _load(seg, rows, elem)
    got, _ = _check(seg, rows, CR.all_pairs(2), 2, 7, elem)
    assert got[1]['b_max'] == 3.0


@pytest.mark.parametrize('elem', [1, 2])
def test_extremes_at_the_ends_of_a_run(seg, limits, elem):
    run = limits[1]
    rows = CC.extremes(2 * run + 3, elem, run)
    _load(seg, rows, elem)
    got, _ = _check(seg, rows, CR.all_pairs(2), 10, 7, elem)
    assert (got['a_min'] == 0.0).all() and (got['a_max'] == 1.0).all()


def test_repeat_and_corner_forms_give_identical_bytes(seg, monkeypatch):
    for elem, rows in ((1, CC.bimodal(70001, 1, seed=1)), (2, CC.world(70001, 3, 2, seed=5))):
        _load(seg, rows, elem)
        pairs = CR.all_pairs(len(rows))
        r = seg.pair_ranges(pairs, 10)
        assert r.tobytes() == seg.pair_ranges(pairs, 10).tobytes()
        edges = _edges_from_ranges(r, 101)
        first = seg.pair_hist(pairs, 10, 101, edges)
        assert first.tobytes() == seg.pair_hist(pairs, 10, 101, edges).tobytes()
        monkeypatch.setenv('WGBSSEG_PAIR_CORNERS', '0')
        assert first.tobytes() == seg.pair_hist(pairs, 10, 101, edges).tobytes()
        monkeypatch.setenv('WGBSSEG_PAIR_CORNERS', '1')
        assert first.tobytes() == seg.pair_hist(pairs, 10, 101, edges).tobytes()
        monkeypatch.delenv('WGBSSEG_PAIR_CORNERS')
    assert seg.last_block_sums_ms() > 0.0


def test_values_outside_the_edges_are_dropped(seg):
    """the ABI takes any ascending edges: uneven ones, and ones that leave values out on either side"""
    rows = CC.world(4097, 2, 1, seed=6)
    _load(seg, rows, 1)
    xe = np.array([0.1, 0.11, 0.5, 0.500001, 0.9])
    ye = np.array([-3.0, 0.0, 0.25, 1.0, 1e300])
    counts = seg.pair_hist([(1, 0)], 3, 4, np.stack([xe, ye])[None])
    x, y = CR.values(rows[1], rows[0], 3)
    assert np.array_equal(counts[0], CR.count(x, y, xe, ye))
    want, _, _ = np.histogram2d(x, y, bins=[xe, ye])
    assert np.array_equal(counts[0], want.astype(np.uint64)) and 0 < counts[0].sum() < x.size


# ---- refusals ----
def _refused(call, code, *words):
    with pytest.raises(_lib.SegmentorError) as e:
        call()
    assert e.value.code == code, e.value.msg
    for w in words:
        assert w in e.value.msg, e.value.msg


def test_refusals(seg, limits):
    rows = CC.world(100, 3, 1)
    _load(seg, rows, 1)
    ok_edges = np.tile(np.linspace(0, 1, 8), (1, 2, 1))
    for call in (seg.pair_ranges, lambda p, c: seg.pair_hist(p, c, 7, np.tile(ok_edges, (max(len(p), 1), 1, 1)))):
        _refused(lambda: call([(0, 1)], 0), _lib.E_ARG, 'min_cov = 0')
        _refused(lambda: call([(0, 1)], -3), _lib.E_ARG, 'min_cov = -3')
        _refused(lambda: call([(0, 1), (1, 3)], 1), _lib.E_ARG, 'pair 1 = (1, 3)')
        _refused(lambda: call([(-1, 0)], 1), _lib.E_ARG, 'pair 0 = (-1, 0)')
        _refused(lambda: call([], 1), _lib.E_ARG, 'n_pairs = 0')
    _refused(lambda: seg.pair_hist([(0, 1)], 1, 0, np.zeros((1, 2, 1))), _lib.E_ARG, 'bins = 0')
    big = limits[0] + 1
    _refused(lambda: seg.pair_hist([(0, 1)], 1, big, np.tile(np.linspace(0, 1, big + 1), (1, 2, 1))), _lib.E_ARG, 'bins = %d' % big)
    for bad, word in ((np.nan, 'not finite'), (np.inf, 'not finite'), (ok_edges[0, 1, 2], 'strictly ascending'), (0.0, 'strictly ascending')):
        e = np.tile(ok_edges, (2, 1, 1))
        e[1, 1, 3] = bad
        _refused(lambda: seg.pair_hist([(0, 1), (1, 0)], 1, 7, e), _lib.E_ARG, word, 'edge 3 of axis 1 of pair 1')
    L, err = seg._L, seg._err
    one = np.zeros(1, dtype=np.int32)
    out = np.zeros(1, dtype=_lib.PAIR_RANGE_DTYPE)
    cnt = np.zeros((1, 7, 7), dtype=np.uint64)
    e = np.ascontiguousarray(ok_edges)
    p = one.ctypes.data
    for args in ((None, p, 1, 1, out.ctypes.data), (p, None, 1, 1, out.ctypes.data), (p, p, 1, 1, None)):
        assert L.wgbsseg_pair_ranges(seg._h, *args, err, _lib.ERRLEN) == _lib.E_ARG and b'NULL' in err.value
    for args in ((None, p, 1, 1, 7, e.ctypes.data, cnt.ctypes.data), (p, None, 1, 1, 7, e.ctypes.data, cnt.ctypes.data),
                 (p, p, 1, 1, 7, None, cnt.ctypes.data), (p, p, 1, 1, 7, e.ctypes.data, None)):
        assert L.wgbsseg_pair_hist(seg._h, *args, err, _lib.ERRLEN) == _lib.E_ARG and b'NULL' in err.value
    assert L.wgbsseg_pair_ranges(None, p, p, 1, 1, out.ctypes.data, err, _lib.ERRLEN) == _lib.E_ARG
    assert L.wgbsseg_pair_hist(None, p, p, 1, 1, 7, e.ctypes.data, cnt.ctypes.data, err, _lib.ERRLEN) == _lib.E_ARG


def test_needs_rows():
    with _lib.Segmenter(0) as s:
        _refused(lambda: s.pair_ranges([(0, 0)], 1), _lib.E_STATE)
        _refused(lambda: s.pair_hist([(0, 0)], 1, 2, np.tile(np.linspace(0, 1, 3), (1, 2, 1))), _lib.E_STATE)


# ---- the Python layer and the command end to end ----
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    td = str(tmp_path_factory.mktemp('compare_world'))
    rows = CC.world(70001, 5, 1, seed=8)
    rows[2] = CC.mixed(np.random.default_rng(20261104), 70001, 1)          # (a covered sample in place of the empty one)
    paths = []
    for s, r in enumerate(rows):
        paths.append(op.join(td, 'smp%d.beta' % s))
        r.tofile(paths[-1])
    wide = CC.world(70001, 2, 2, seed=8)
    lpaths = []
    for s, r in enumerate(wide):
        lpaths.append(op.join(td, 'wide%d.lbeta' % s))
        r.tofile(lpaths[-1])
    from wgbs_tools_amd import synth
    ref = synth.write_genome(op.join(td, 'references', 'synth'), ['chr1'], [70001], synth.synth_loci(20261105, [70001]))
    return (td, ref), paths, rows, lpaths, wide


def _against_numpy(rows, result, min_cov, bins):
    pairs, counts, xedges, yedges = result
    assert [tuple(p) for p in pairs] == CR.all_pairs(len(rows))
    for k, (i, j) in enumerate(pairs):
        x, y = CR.values(rows[i], rows[j], min_cov)
        h, xe, ye = np.histogram2d(x, y, bins)
        assert np.array_equal(counts[k], h.astype(np.uint64)), (i, j)
        assert xedges[k].tobytes() == xe.tobytes() and yedges[k].tobytes() == ye.tobytes(), (i, j)


def test_pair_histograms_end_to_end(files):
    from wgbs_tools_amd import compare_betas
    td, paths, rows, lpaths, wide = files
    _against_numpy(rows, compare_betas.pair_histograms(paths), 10, 101)
    _against_numpy(rows, compare_betas.pair_histograms(paths, min_cov=3, bins=20), 3, 20)
    # through -s: 1-based [start, end)
    cut = [r[1000:30001] for r in rows]
    _against_numpy(cut, compare_betas.pair_histograms(paths, sites=(1001, 30002)), 10, 101)
    # .beta and .lbeta together: widened on the host
    both = [rows[0].astype(np.uint16), wide[0], wide[1]]
    _against_numpy(both, compare_betas.pair_histograms([paths[0]] + lpaths, min_cov=12, bins=9), 12, 9)


def test_command_writes_npz(files, tmp_path):
    from wgbs_tools_amd import wgbs_tools
    (td, ref), paths, rows, lpaths, wide = files
    out = str(tmp_path / 'cmp.npz')
    assert wgbs_tools.main(['wgbstools', 'compare_betas'] + paths[:3] + ['-o', out, '--bins', '31', '-c', '5', '-s', '11-60001', '--genome', ref]) == 0
    z = np.load(out)
    assert list(z['names']) == ['smp0', 'smp1', 'smp2']
    _against_numpy([r[10:60000] for r in rows[:3]], (z['pairs'], z['counts'], z['xedges'], z['yedges']), 5, 31)
