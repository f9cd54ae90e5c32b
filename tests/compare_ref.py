"""TEST INFRASTRUCTURE: a numpy restatement of what `wgbstools compare_betas` computes per pair of files (the reference's comp2:
the mask, the ratios, np.histogram2d with no range given), spelled out step by step so that the kernels' rules (k_pair_ranges,
k_pair_hist) can be checked one by one.  tests/test_compare_cpu.py pins it to np.histogram2d itself and to what the reference's
own comp2 drew (tests/golden/compare_cases.json).  Not imported by the product.

Rows are [n, 2] (meth, cov) arrays of uint8 or uint16.  x is sample b, y is sample a, as comp2(a, b) draws them."""
import numpy as np


def mask(ra, rb, min_cov):
    return np.minimum(ra[:, 1], rb[:, 1]) >= min_cov


def values(ra, rb, min_cov):
    """(x, y): meth / cov of b and of a over the sites both cover — numpy divides uint8 / uint16 columns in float64"""
    keep = mask(ra, rb, min_cov)
    a, b = ra[keep], rb[keep]
    return b[:, 0] / b[:, 1], a[:, 0] / a[:, 1]


def value_range(v):
    """what np.histogram2d takes as the range of an axis when none is given"""
    if v.size == 0:
        return 0.0, 1.0
    lo, hi = float(v.min()), float(v.max())
    if lo == hi:
        return lo - 0.5, hi + 0.5
    return lo, hi


def axis_edges(v, bins):
    lo, hi = value_range(v)
    return np.linspace(lo, hi, bins + 1)


def cells(edges, v):
    """cell of every value, -1 for a value outside the edges"""
    c = np.searchsorted(edges, v, side='right') - 1
    c[v == edges[-1]] -= 1
    c[(c < 0) | (c >= edges.size - 1)] = -1
    return c


def count(x, y, xedges, yedges):
    """counts [x_cell, y_cell] (uint64) of the values against given edges"""
    nx, ny = xedges.size - 1, yedges.size - 1
    cx, cy = cells(xedges, x), cells(yedges, y)
    ok = (cx >= 0) & (cy >= 0)
    flat = np.bincount(cx[ok] * ny + cy[ok], minlength=nx * ny)
    return flat.reshape(nx, ny).astype(np.uint64)


def hist(ra, rb, min_cov, bins):
    """-> counts [bins, bins] uint64, xedges, yedges"""
    x, y = values(ra, rb, min_cov)
    xe, ye = axis_edges(x, bins), axis_edges(y, bins)
    return count(x, y, xe, ye), xe, ye


def pair_range(ra, rb, min_cov):
    """what wgbsseg_pair_ranges returns for the pair (a, b)"""
    x, y = values(ra, rb, min_cov)
    if x.size == 0:
        return dict(n=0, a_min=0.0, a_max=0.0, b_min=0.0, b_max=0.0)
    return dict(n=int(x.size), a_min=float(y.min()), a_max=float(y.max()), b_min=float(x.min()), b_max=float(x.max()))


def all_pairs(n):
    """the reference's pairs: (i, j) with j <= i, row by row"""
    return [(i, j) for i in range(n) for j in range(i + 1)]
