"""The planner of the share groups (csrc/share_plan.h behind wgbsseg_plan_shares[_weighted]) against a numpy restatement written here: the
chunk grid, the work of a chunk, the cut into contiguous runs by cumulative work, the shares that get nothing, the windows and their
128-site alignment, the halo's default - all six arrays exactly; and its refusals by message.  Host arithmetic only: no device."""
import numpy as np
import pytest

from wgbs_tools_amd import _lib, parallel, synth

SIZES = [24900, 100000, 3700, 50000, 1]
MAX_CPG, MAX_BP = 1000, 2000


@pytest.fixture(scope='module')
def world():
    return synth.synth_loci(5, SIZES), parallel.regions_of_sizes(SIZES)


def _chunk_work(seg):
    """Scored blocks of a chunk whose positions ascend: site k opens blocks up to the first site that is max_cpg sites or more than
    max_bp bases away, or the chunk's end - at least the block of k alone."""
    assert (np.diff(seg) >= 0).all()
    k = np.arange(seg.size)
    end = np.minimum(np.minimum(np.searchsorted(seg, seg + MAX_BP, side='right'), k + MAX_CPG), seg.size)
    return int((np.maximum(end, k + 1) - k).sum())


def _restate(loci, regions, chunk, n_shares, halo, weights, work_of):
    cks = [(s - 1, min(s + chunk, b) - 1) for a, b in regions for s in range(a, b, chunk)]
    if n_shares == 1:
        w = [hi - lo for lo, hi in cks]
    else:
        w = [work_of[c] + 4 * (c[1] - c[0]) for c in cks]
    total = sum(w)
    if weights is None:
        upto = [(d + 1) / n_shares for d in range(n_shares)]
    else:
        run = np.cumsum(np.asarray(weights, dtype=np.float64))
        upto = (run / run[-1]).tolist()
    out = {k: np.zeros(n_shares, dtype=np.int64) for k in ('own_lo', 'own_hi', 'win_lo', 'win_hi', 'chunks', 'work')}
    d, acc = 0, 0
    for (lo, hi), wk in zip(cks, w):
        while d < n_shares - 1 and float(acc) >= float(total) * upto[d]:
            d += 1
        if not out['chunks'][d]:
            out['own_lo'][d] = lo
        out['own_hi'][d] = hi
        out['chunks'][d] += 1
        out['work'][d] += wk
        acc += wk
    if halo < 0:
        halo = max(chunk, 4096)
    for q in range(n_shares):
        if not out['chunks'][q]:
            out['own_lo'][q] = out['own_hi'][q] = out['own_hi'][q - 1] if q else cks[0][0]
        else:
            out['win_lo'][q] = max(0, out['own_lo'][q] - halo) // 128 * 128
            out['win_hi'][q] = min(loci.size, out['own_hi'][q] + halo)
    return out


@pytest.mark.parametrize('chunk', [1000, 7000, 60000])
def test_plan_equals_restatement(world, chunk):
    loci, regions = world
    lo64 = loci.astype(np.int64)
    work_of = {(s - 1, e - 1): _chunk_work(lo64[s - 1:e - 1]) for _, s, e in parallel.chunk_grid(regions, chunk)}
    idle = 0
    for n_shares in (1, 2, 3, 8, 40):
        with_zero = [[1.0, 0.0, 2.0, 1.5][d % 4] for d in range(n_shares)]
        for weights in (None, [0.6] + [1.0] * (n_shares - 1), with_zero):
            if n_shares == 1 and weights is with_zero:
                weights = [1.0]                                    # (a single zero is "all weights are zero": among the refusals below)
            for halo in (-1, 10, 5000):
                got = _lib.plan_shares(loci, regions, chunk, 15.0, MAX_CPG, MAX_BP, n_shares, halo=halo, weights=weights)
                want = _restate(loci, regions, chunk, n_shares, halo, weights, work_of)
                for key in want:
                    assert np.array_equal(got[key], want[key]), (n_shares, weights, halo, key, got[key], want[key])
                assert got['chunks'].sum() == len(work_of)
                idle += int((got['chunks'] == 0).sum())
    assert idle > 0                                                # a zero weight or 40 shares: somebody got nothing
    if chunk == 60000:                                             # 6 chunks over 40 shares
        assert (_lib.plan_shares(loci, regions, chunk, 15.0, MAX_CPG, MAX_BP, 40)['chunks'] == 0).sum() >= 34


def test_plan_refusals(world):
    loci, regions = world
    n = int(loci.size)

    def refused(msg, regions=regions, max_bp=MAX_BP, n_shares=3, weights=None):
        with pytest.raises(_lib.SegmentorError) as e:
            _lib.plan_shares(loci, regions, 7000, 15.0, MAX_CPG, max_bp, n_shares, weights=weights)
        assert e.value.code == _lib.E_ARG and e.value.msg == msg, e.value.msg

    refused('plan_shares: weights must be >= 0', weights=[1.0, -0.5, 1.0])
    refused('plan_shares: weights must be >= 0', weights=[1.0, float('nan'), 1.0])
    refused('plan_shares: all weights are zero', weights=[0.0, 0.0, 0.0])
    refused('plan_shares: all weights are zero', n_shares=1, weights=[0.0])
    refused('plan_shares: regions must be ascending and disjoint', regions=[regions[1], regions[0]])
    refused('plan_shares: regions must be ascending and disjoint', regions=[(1, 500), (499, 900)])
    refused('region 1 = [500, 500) is empty or outside the %d sites' % n, regions=[(1, 500), (500, 500)])
    refused('region 0 = [1, %d) is empty or outside the %d sites' % (n + 3, n), regions=[(1, n + 3)])
    refused('max_bp and max_cpg must be >= 1', max_bp=0)
