"""numpy restatement of wgbsseg_sample_stats (include/wgbsseg.h): what the per-sample statistics kernel must return, field by
field, as Python integers.  Used by the CPU suite (against plain numpy) and the GPU suite (against the library)."""
import numpy as np

FIELDS = ('n_sites', 'meth_sum', 'cov_sum', 'covered', 'covered_at', 'orphans', 'ratio_lo', 'ratio_hi', 'max_cov')
UNIT_BITS = 62                                         # the ratio sum counts units of 2^-62


def term_units(m, c):
    """fl(fl(m / c) * 100.0) as an integer number of 2^-62 (exact: the double is a multiple of 2^-62 for uint8 / uint16 counts)"""
    t = float(np.float64(m) / np.float64(c) * 100.0)
    num, den = t.as_integer_ratio()
    scaled = num << UNIT_BITS
    assert scaled % den == 0, (m, c)
    return scaled // den


def ratio_units(rows):
    """exact sum of the terms over the sites with cov > 0 of an [n, 2] (meth, cov) array, as a Python int"""
    rows = np.asarray(rows)
    rows = rows[rows[:, 1] > 0]
    if not rows.size:
        return 0
    wide = rows.dtype.itemsize > 1                             # (a narrow key sorts fast: the 5 M-site case)
    key = rows[:, 0].astype(np.uint32) << 16 | rows[:, 1] if wide else rows[:, 0].astype(np.uint16) << 8 | rows[:, 1]
    pairs, counts = np.unique(key, return_counts=True)
    sh, mask = (16, 0xffff) if wide else (8, 0xff)
    return sum(term_units(k >> sh, k & mask) * n for k, n in zip(pairs.tolist(), counts.tolist()))


def select(rows, ranges):
    """the rows of the union of the 0-based half-open `ranges` (ascending, disjoint), concatenated"""
    rows = np.asarray(rows)
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    if not len(r):
        return rows[:0]
    return np.concatenate([rows[a:b] for a, b in r.tolist()])


def expect(rows, ranges, depth_at=10):
    """dict of FIELDS for one sample's [n, 2] rows over the union of `ranges`"""
    d = select(rows, ranges)
    assert d.dtype in (np.uint8, np.uint16)
    ratio = ratio_units(d)
    m, c = d[:, 0].astype(np.int64), d[:, 1].astype(np.int64)
    return {'n_sites': int(len(d)), 'meth_sum': int(m.sum()), 'cov_sum': int(c.sum()), 'covered': int((c > 0).sum()),
            'covered_at': int((c >= depth_at).sum()), 'orphans': int(((c == 0) & (m > 0)).sum()),
            'ratio_lo': ratio & (2 ** 64 - 1), 'ratio_hi': ratio >> 64, 'max_cov': int(c.max()) if len(d) else 0}


def as_dict(stat):
    """one element of Segmenter.sample_stats' structured array -> dict of FIELDS as Python ints"""
    return {k: int(stat[k]) for k in FIELDS}
