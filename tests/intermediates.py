"""Expected intermediates of the segment path, and their comparison with what wgbsseg_debug_fetch returns.

For a world (beta slices per sample + loci) and a list of chunks (start0, len) `expected()` gives, per chunk, what the device
must hold bit for bit: the window extents F_k, their exclusive prefix (chunk-relative), the scored blocks as uint64 bit patterns
in start-major rows (row k = ends k .. k + F_k - 1) and the back-pointers k + 1 - T[k + 1].  Every chunk is scored on its own
slice by oracle.segment_chunk(..., debug=True), as the reference does (`-s start0 -n len`).

The hook's layout (include/wgbsseg.h) is dense: chunk after chunk in the caller's order, no padding.  `diff_sites` and
`diff_cost` compare a dense array with the per-chunk expectation and name the first cell that differs: chunk, start site, end
site, got, want.  tests/test_intermediates_cpu.py plants faults to show that they are not blind.
"""
import collections
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle


def _numpy_windows(loci, max_cpg, max_bp):
    """forward window F_k: number of admissible ends i >= k of a block starting at k (segmentor.cpp:111-117)"""
    l = loci.astype(np.int64)
    k = np.arange(l.size)
    hi = np.searchsorted(l, l + max_bp, 'right') - 1
    hi = np.minimum(np.minimum(hi, k + max_cpg - 1), l.size - 1)
    return (hi - k + 1).astype(np.int64)


def _first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return 'shape %s vs %s' % (a.shape, b.shape)
    d = np.flatnonzero(a != b)
    if d.size == 0:
        return None
    i = int(d[0])
    return '%d mismatches, first at %d: got %r want %r' % (d.size, i, a.flat[i], b.flat[i])


# one chunk's expectation.  W, cum, back: int64 [len]; cost: uint64 [sum(W)] (fp64 bit patterns); borders: the oracle's list
Expected = collections.namedtuple('Expected', 'start0 length W cum cost back borders')

# the first cell that differs.  window / cum: `start` is the site, `end` None; back: `end` is the site (the block ending there),
# `start` None; cost: the block [start, end].  Sites are chunk-relative; `count` cells differ in all.
Mismatch = collections.namedtuple('Mismatch', 'what chunk start end got want count')


def describe(m):
    if m is None:
        return 'equal'
    if m.chunk is None:
        return '%s: %d entries fetched, %d expected' % (m.what, m.got, m.want)
    where = 'chunk %d' % m.chunk
    if m.start is not None: where += ', start site %d' % m.start
    if m.end is not None: where += ', end site %d' % m.end
    return '%s: %d cells differ, first in %s: got %r want %r' % (m.what, m.count, where, m.got, m.want)


def expected_chunk(slices, loci, start0, length, pcount, max_cpg, max_bp):
    """One chunk, scored on its own slice.  max_cpg is cut to the chunk's length (a window never exceeds its chunk,
    segmentor.cpp:110), which keeps the oracle's [len, max_cpg] debug band small."""
    sl = [np.ascontiguousarray(s[start0:start0 + length]) for s in slices]
    lo = np.ascontiguousarray(loci[start0:start0 + length])
    mc = int(min(max_cpg, length))
    W = _numpy_windows(lo, mc, max_bp)
    cum = np.concatenate([[0], np.cumsum(W)[:-1]]).astype(np.int64)
    b, M, T, band = oracle.segment_chunk(sl, lo, pcount, mc, max_bp, debug=True)
    inside = np.arange(mc, dtype=np.int64)[None, :] < W[:, None]
    cost = band[inside].view(np.uint64)                            # row-major over (k, j < F_k): start-major rows
    del band
    back = np.arange(1, length + 1, dtype=np.int64) - T[1:]
    return Expected(int(start0), int(length), W, cum, cost, back, b)


def expected(slices, loci, chunks, pcount, max_cpg, max_bp, threads=None):
    """-> [Expected] for chunks = [(start0, len), ...], in that order (the chunks in parallel: the oracle releases the GIL)"""
    chunks = [(int(a), int(l)) for a, l in chunks]
    threads = min(len(chunks), threads or min(16, os.cpu_count() or 1))
    work = lambda c: expected_chunk(slices, loci, c[0], c[1], pcount, max_cpg, max_bp)
    if threads <= 1:
        return [work(c) for c in chunks]
    with ThreadPoolExecutor(threads) as pool:
        return list(pool.map(work, chunks))


# ---------------------------------------------------------------------------------------------------------
# the dense layout
# ---------------------------------------------------------------------------------------------------------
def dense_offsets(sizes):
    """entries per chunk -> where each chunk begins in the dense array, and (last) the array's length"""
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def dense(exp, what):
    """the dense array the hook must return for `what` in 'window', 'cum', 'back', 'cost'"""
    field = {'window': 'W', 'cum': 'cum', 'back': 'back', 'cost': 'cost'}[what]
    return np.concatenate([getattr(e, field) for e in exp])


def locate_cost(exp, j):
    """entry j of the dense cost array -> (chunk, start site, end site)"""
    off = dense_offsets([e.cost.size for e in exp])
    assert 0 <= j < off[-1]
    c = int(np.searchsorted(off, j, 'right') - 1)
    r = int(j - off[c])
    k = int(np.searchsorted(exp[c].cum, r, 'right') - 1)
    return c, k, k + r - int(exp[c].cum[k])


def locate_site(exp, j):
    """entry j of a dense per-site array -> (chunk, site)"""
    off = dense_offsets([e.length for e in exp])
    assert 0 <= j < off[-1]
    c = int(np.searchsorted(off, j, 'right') - 1)
    return c, int(j - off[c])


def _diff(what, got, want, where):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return Mismatch(what, None, None, None, int(got.size), int(want.size), -1)
    d = np.flatnonzero(got != want)
    if d.size == 0:
        return None
    j = int(d[0])
    c, s, e = where(j)
    return Mismatch(what, c, s, e, got[j].item(), want[j].item(), int(d.size))


def diff_sites(what, got, exp):
    """dense 'window' / 'cum' / 'back' of a batch against the expectation -> None or the first Mismatch"""
    assert what in ('window', 'cum', 'back')
    want = dense(exp, what)

    def where(j):
        c, i = locate_site(exp, j)
        return (c, None, i) if what == 'back' else (c, i, None)
    return _diff(what, np.asarray(got).astype(np.int64), want, where)


def diff_cost(got, exp):
    """dense 'cost' of a batch (float64, or its uint64 bits) against the expectation, bit for bit -> None or the first Mismatch;
    got / want of a Mismatch are the bit patterns"""
    got = np.asarray(got)
    if got.dtype != np.uint64:
        got = np.ascontiguousarray(got, dtype=np.float64).view(np.uint64)
    return _diff('cost', got, dense(exp, 'cost'), lambda j: locate_cost(exp, j))


def describe_cost(m):
    """describe() with the doubles behind the bit patterns"""
    if m is None or m.chunk is None:
        return describe(m)
    f = lambda bits: float(np.array([bits], dtype=np.uint64).view(np.float64)[0])
    return describe(m) + ' (%r vs %r)' % (f(m.got), f(m.want))


# ---------------------------------------------------------------------------------------------------------
# a device call against the expectation (GPU tests)
# ---------------------------------------------------------------------------------------------------------
def fetch(sg, what, exp):
    """the last call's dense `what` from Segmenter `sg`, sized by the expectation"""
    if what == 'cost':
        return sg.debug_fetch('cost', np.float64, int(sum(e.cost.size for e in exp))).view(np.uint64)
    n = int(sum(e.length for e in exp))
    return sg.debug_fetch(what, np.uint32 if what == 'cum' else np.uint16, n)


def check_call(sg, exp, got_borders, whats, label=''):
    """After sg.segment_chunks(...) on the chunks of `exp`: every intermediate of `whats` equals the expectation exactly, and so do the
    border lists.  Raises AssertionError naming kernel output, chunk, start site, end site, got and want."""
    for what in whats:
        got = fetch(sg, what, exp)
        m = diff_cost(got, exp) if what == 'cost' else diff_sites(what, got, exp)
        assert m is None, '%s%s' % (label and label + ': ', describe_cost(m) if what == 'cost' else describe(m))
    for c, (e, b) in enumerate(zip(exp, got_borders)):
        assert np.asarray(b).tolist() == e.borders.tolist(), '%s%sborders of chunk %d: %s' % (label, label and ': ', c, _first_diff(b, e.borders))
