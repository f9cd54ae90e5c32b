"""Seeded inputs of the pairwise-histogram tests (tests/test_compare_cpu.py, tests/test_gpu_compare.py).  Everything is
regenerated from the seed, nothing stored.  Rows are [n, 2] (meth, cov) arrays of uint8 (elem 1) or uint16 (elem 2)."""
import numpy as np

SIZES = (1, 9, 4097, 70001)              # the GPU test adds twice a workgroup's run of sites plus 3
SAMPLES = (1, 2, 3, 5)
BINS = (1, 2, 7, 101)                    # the GPU test adds the library's limit


def _dt(elem):
    return np.uint8 if elem == 1 else np.uint16


def mixed(rng, n, elem, like=None):
    """shallow and deep sites, some without reads; with `like` the methylation follows that sample's (a concordant pair)"""
    top = 255 if elem == 1 else 1000
    cov = np.where(rng.random(n) < 0.4, rng.integers(0, 12, n), rng.integers(0, top + 1, n))
    if like is None:
        frac = rng.random(n)
    else:
        frac = np.clip(like[:, 0] / np.maximum(like[:, 1], 1) + rng.normal(0, 0.08, n), 0, 1)
    meth = np.minimum(np.rint(frac * cov), cov)
    return np.stack([meth, cov], axis=1).astype(_dt(elem))


def world(n, n_samples, elem, seed=0):
    """up to five samples: 0 mixed, 1 concordant with 0, 2 without any coverage, 3 with one ratio everywhere (1 / 4, at
    coverages 4, 8, 12, ... so that the division is exact), 4 a copy of 0"""
    rng = np.random.default_rng([20261101, n, elem, seed])
    s0 = mixed(rng, n, elem)
    s1 = mixed(rng, n, elem, like=s0)
    s2 = np.zeros((n, 2), dtype=_dt(elem))
    q = rng.integers(1, 60 if elem == 1 else 200, n)
    s3 = np.stack([q, 4 * q], axis=1).astype(_dt(elem))
    return [s0, s1, s2, s3, s0.copy()][:n_samples]


def bimodal(n, elem, seed=0):
    """two concordant samples, well covered, >= 90 % of the sites at ratio 0 or 1 in both: the corner cells take almost all"""
    rng = np.random.default_rng([20261102, n, elem, seed])
    state = rng.random(n)
    rows = []
    for _ in range(2):
        cov = rng.integers(10, 200 if elem == 1 else 600, n)
        meth = np.where(state < 0.47, 0, np.where(state < 0.94, cov, rng.integers(0, cov + 1)))
        rows.append(np.stack([meth, cov], axis=1).astype(_dt(elem)))
    return rows


def over(n, elem, seed=0):
    """two mixed samples; one site of the first has meth > cov (a ratio of 3)"""
    rng = np.random.default_rng([20261103, n, elem, seed])
    rows = [mixed(rng, n, elem), mixed(rng, n, elem)]
    k = n // 2
    rows[0][k] = (90, 30)
    rows[1][k] = (20, 40)
    return rows


def extremes(n, elem, run):
    """sample 0: ratio 1 / 2 everywhere but its smallest value (0) at the first site of the second run of `run` sites and its
    largest (1) at the last site of that run; sample 1: the same with the two at the first and the last site of the row"""
    rows = []
    for lo_at, hi_at in ((run, 2 * run - 1), (0, n - 1)):
        r = np.empty((n, 2), dtype=_dt(elem))
        r[:, 0], r[:, 1] = 20, 40
        r[lo_at] = (0, 40)
        r[hi_at] = (40, 40)
        rows.append(r)
    return rows


def flat(rows):
    """rows as Segmenter.set_betas / set_lbetas take them"""
    return [np.ascontiguousarray(r).reshape(-1) for r in rows]


def golden_cases():
    """the small cases tests/golden/make_golden_compare.py hands to the reference's comp2: name -> (a, b, min_cov, bins)"""
    out = {}
    for elem in (1, 2):
        w = world(200, 5, elem, seed=7)
        tag = 'u8' if elem == 1 else 'u16'
        out['mixed_' + tag] = (w[0], w[1], 3, 7)
        out['identical_' + tag] = (w[0], w[4], 10, 5)
        out['constant_x_' + tag] = (w[0], w[3], 1, 4)
        out['constant_y_' + tag] = (w[3], w[1], 5, 3)
        out['both_constant_' + tag] = (w[3], w[3], 1, 2)
        b = bimodal(150, elem, seed=7)
        out['bimodal_' + tag] = (b[0], b[1], 10, 7)
        o = over(120, elem, seed=7)
        out['meth_above_cov_' + tag] = (o[0], o[1], 2, 6)
        out['one_bin_' + tag] = (w[1], w[0], 8, 1)
        out['no_common_site_' + tag] = (w[0], w[2], 1, 3)
    return out
