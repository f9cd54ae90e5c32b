"""The host plans of the pat engines and of sample_stats (csrc/bimodal_plan.h, homog_plan.h, stats_plan.h) through their host build
(tests/native/patplan_host.cpp), against numpy restatements written here; the retire / drop rules of test_bimodal walked the way
wgbsseg_bimodal_feed and _finish walk them, over reads cut into chunks at random lines: no block is retired before all its reads have
come, none of them has been dropped by then, every block is retired once; and every refusal text, as it read before the plans had
headers of their own."""
import ctypes as C
import os.path as op
import subprocess

import numpy as np
import pytest

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(HERE)
CSRC = op.join(ROOT, 'wgbs_tools_amd', 'csrc')
SRC = op.join(HERE, 'native', 'patplan_host.cpp')
LIB = op.join(HERE, 'native', 'libpatplan_host.so')
DEPS = [SRC, op.join(ROOT, 'include', 'wgbsseg.h')] + [op.join(CSRC, h) for h in ('bimodal_plan.h', 'homog_plan.h', 'stats_plan.h', 'block_plan.h', 'exact_log2.h')]
OK, E_ARG, E_CAPACITY = 0, -1, -6
I64_MAX, I64_MIN = 2 ** 63 - 1, -2 ** 63
CTX, LDS_COLS, COL_BYTES, ST_TILE = 150, 256, 48, 1024
P = C.c_void_p


@pytest.fixture(scope='module')
def L():
    """tests/native/libpatplan_host.so (built when missing or older than its sources)"""
    if not op.isfile(LIB) or op.getmtime(LIB) < max(op.getmtime(d) for d in DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', SRC, '-o', LIB])
    lib = C.CDLL(LIB)
    lib.patplan_constants.argtypes = [P]
    lib.patplan_bim_new.restype = P
    lib.patplan_bim_new.argtypes = [P, P, C.c_int64, C.c_int32, C.c_int32, P, C.c_char_p, C.c_size_t]
    lib.patplan_bim_free.argtypes = [P]
    lib.patplan_bim_tables.restype = C.c_int32
    lib.patplan_bim_tables.argtypes = [P] * 5
    lib.patplan_bim_retire_upto.restype = C.c_int64
    lib.patplan_bim_retire_upto.argtypes = [P, C.c_int64, C.c_int64]
    lib.patplan_bim_drop_below.restype = C.c_int64
    lib.patplan_bim_drop_below.argtypes = [P, C.c_int64]
    lib.patplan_bim_chunk_bound.argtypes = [C.c_int64, P]
    lib.patplan_bim_scratch.restype = C.c_int
    lib.patplan_bim_scratch.argtypes = [P, P, C.c_int64, C.c_int32, P, P, C.c_char_p, C.c_size_t]
    lib.patplan_homog.restype = C.c_int
    lib.patplan_homog.argtypes = [P, P, C.c_int64, P, C.c_int32, C.c_int32, P, P, P, P, C.c_char_p, C.c_size_t]
    lib.patplan_stats.restype = C.c_int
    lib.patplan_stats.argtypes = [P, P, C.c_int64, C.c_int64, C.c_int32, C.c_int32, P, P, P, P, C.c_char_p, C.c_size_t]
    k = np.zeros(10, dtype=np.int64)
    lib.patplan_constants(k.ctypes.data)
    assert k.tolist() == [CTX, LDS_COLS, COL_BYTES, 100000, I64_MIN, 8, I64_MIN, 256, 4, ST_TILE]
    return lib


def _i64(v):
    return np.ascontiguousarray(v, dtype=np.int64)


def _ptr(a, null=False):
    return None if null else a.ctypes.data


# ---------------------------------------------------------------------------------------------------------
# test_bimodal
# ---------------------------------------------------------------------------------------------------------
class BimPlan:
    def __init__(self, L, s, e, min_len=1, cols=-1, null=False):
        self.L = L
        s, e = _i64(s), _i64(e)
        n = s.size
        rc = C.c_int32(77)
        msg = C.create_string_buffer(600)
        self.h = L.patplan_bim_new(_ptr(s, null), _ptr(e, null), n, min_len, cols, C.addressof(rc), msg, 600)
        self.rc, self.msg = rc.value, msg.value.decode()
        if self.h:
            self.s1, self.s2, self.by_end = (np.full(n, -7, dtype=np.int32) for _ in range(3))
            self.lo_after = np.full(n + 1, -7, dtype=np.int64)
            self.lds_cols = L.patplan_bim_tables(self.h, self.s1.ctypes.data, self.s2.ctypes.data, self.by_end.ctypes.data, self.lo_after.ctypes.data)

    def retire_upto(self, pending, last_start):
        return int(self.L.patplan_bim_retire_upto(self.h, pending, I64_MIN if last_start is None else last_start))

    def drop_below(self, pending):
        return int(self.L.patplan_bim_drop_below(self.h, pending))

    def close(self):
        if self.h:
            self.L.patplan_bim_free(self.h)
            self.h = None


def _bim_restated(s, e):
    """by_end: the blocks in order of endCpG, equal ones as they came; lo_after[p]: the lowest first site any block of by_end[p:] asks for"""
    s, e = [int(v) for v in s], [int(v) for v in e]
    by_end = sorted(range(len(s)), key=lambda j: (e[j], j))
    lo_after = [min([max(1, s[j] - CTX) for j in by_end[p:]], default=I64_MAX) for p in range(len(s) + 1)]
    return by_end, lo_after


def _retire_restated(e, by_end, pending, last_start):
    """the blocks that end at or before the last start seen are complete (by_end is ordered by end: they are its first ones)"""
    if last_start is None:
        return pending
    return max(pending, sum(1 for j in by_end if int(e[j]) <= last_start))


def _drop_restated(s, by_end, pending):
    return min([max(1, int(s[j]) - CTX) for j in by_end[pending:]], default=2 ** 31)


BIM_TABLES = {
    'one block': ([400], [420]),
    'shared endCpG': ([300, 10, 250, 500], [320, 320, 320, 501]),
    'nested': ([100, 200, 210, 205, 900], [1000, 300, 220, 206, 901]),
    'startCpG within the context of site 1': ([1, 150, 151, 152, 700], [5, 160, 400, 153, 800]),
    'descending file order': ([900, 600, 300, 1], [950, 650, 350, 2]),
    'ends at 2^31 - 1': ([5, 2 ** 31 - 2], [9, 2 ** 31 - 1]),
}


def _random_blocks(rng):
    n_sites = int(rng.integers(30, 3000))
    nb = int(rng.integers(1, 40))
    s = rng.integers(1, n_sites, nb)
    e = s + rng.integers(1, rng.choice([2, 30, 1500]), nb)
    if nb > 2 and rng.random() < 0.5:
        e[rng.integers(0, nb, 2)] = e[0]                                      # shared ends
    return s, np.maximum(e, s + 1), n_sites


def _check_bim_plan(L, s, e):
    p = BimPlan(L, s, e)
    try:
        assert p.rc == OK and p.msg == '' and p.lds_cols == LDS_COLS
        by_end, lo_after = _bim_restated(s, e)
        assert p.s1.tolist() == [int(v) for v in s] and p.s2.tolist() == [int(v) for v in e]
        assert p.by_end.tolist() == by_end and p.lo_after.tolist() == lo_after
        n = len(by_end)
        lasts = sorted({None, 0, 1, 2 ** 31} | {int(v) + d for v in e for d in (-1, 0, 1)}, key=lambda v: -1 if v is None else v)
        for pending in sorted({0, n // 2, max(0, n - 1), n}):
            assert p.drop_below(pending) == _drop_restated(s, by_end, pending)
            for last in lasts:
                assert p.retire_upto(pending, last) == _retire_restated(e, by_end, pending, last), (pending, last)
    finally:
        p.close()


@pytest.mark.parametrize('name', sorted(BIM_TABLES))
def test_bimodal_plan_fixed_tables(L, name):
    _check_bim_plan(L, *BIM_TABLES[name])


def test_bimodal_plan_random_tables(L):
    rng = np.random.default_rng(20261019)
    for _ in range(300):
        s, e, _n = _random_blocks(rng)
        _check_bim_plan(L, s, e)


def test_bimodal_lds_cols_clamp(L):
    for cols, want in ((-1, LDS_COLS), (-5, LDS_COLS), (0, 0), (16, 16), (LDS_COLS, LDS_COLS), (LDS_COLS + 1, LDS_COLS), (2 ** 31 - 1, LDS_COLS)):
        p = BimPlan(L, [3], [9], cols=cols)
        assert p.rc == OK and p.lds_cols == want
        p.close()


def _scratch(L, meta, ids, lds_cols):
    meta = _i64(meta).reshape(-1, 6)
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    n = meta.shape[0]
    off = np.full(max(n, 1), -7, dtype=np.int64)
    used = C.c_uint64(77)
    msg = C.create_string_buffer(600)
    rc = L.patplan_bim_scratch(meta.ctypes.data, ids.ctypes.data, n, lds_cols, off.ctypes.data, C.addressof(used), msg, 600)
    return rc, msg.value.decode(), off[:n].tolist(), used.value


def test_bimodal_scratch_layout(L):
    """a block with rows and more columns than the LDS tables hold gets ncols x 48 bytes behind the blocks before it; every other one offset 0"""
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(1, 30))
        lds_cols = int(rng.choice([0, 16, LDS_COLS]))
        ncols = rng.choice([0, 1, 15, 16, 17, LDS_COLS - 1, LDS_COLS, LDS_COLS + 1, 5000], n)
        rows = rng.choice([0, 1, 7, 2 ** 31 - 1], n)
        meta = np.zeros((n, 6), dtype=np.int64)
        meta[:, 3], meta[:, 4] = ncols, rows
        rc, msg, off, used = _scratch(L, meta, np.arange(n), lds_cols)
        want, at = [], 0
        for g in range(n):
            wide = rows[g] > 0 and ncols[g] > lds_cols
            want.append(at if wide else 0)
            at += int(ncols[g]) * COL_BYTES if wide else 0
        assert (rc, msg, off, used) == (OK, '', want, at)
    assert _scratch(L, np.zeros((0, 6)), [], 16) == (OK, '', [], 0)
    # the refusal: more than 2^31 - 1 rows in one block; the message names the block's place in the retired group and its row of the blocks file
    meta = np.zeros((3, 6), dtype=np.int64)
    meta[:, 3] = 300
    meta[:, 4] = (5, 2 ** 31, 5)
    rc, msg, _off, _used = _scratch(L, meta, [11, 4, 6], 16)
    assert rc == E_CAPACITY and msg == 'test_bimodal: block 1 (row 5 of the blocks) has 2147483648 rows: more than 2^31 - 1'


# the walk ------------------------------------------------------------------------------------------------
def _pat_line(start, pattern, count, chrom='chr1'):
    return '%s\t%d\t%s\t%d\n' % (chrom, start, pattern, count)


def _true_counts(chunk):
    """lines and 16-site pattern words of a chunk of good pat lines, by splitting the text"""
    lines = chunk.split('\n')[:-1]
    return len(lines), sum(-(-len(l.split('\t')[2]) // 16) for l in lines)


def _bound(L, n_bytes):
    out = np.zeros(2, dtype=np.uint64)
    L.patplan_bim_chunk_bound(n_bytes, out.ctypes.data)
    return int(out[0]), int(out[1])


def _walk(L, s, e, starts, chunks_of):
    """feed() per chunk: retire what the reads before this chunk completed, drop below the pending blocks' lowest reach, append; finish():
    retire the rest.  `chunks_of`: the number of reads in each chunk.  Returns the number of feed() steps that retired something."""
    p = BimPlan(L, s, e)
    try:
        n = len(s)
        starts = [int(v) for v in starts]
        wanted = [[i for i, st in enumerate(starts) if max(1, int(s[j]) - CTX) <= st <= int(e[j]) - 1] for j in range(n)]
        table, appended, last_start, pending, retired, steps = [], 0, None, 0, [0] * n, 0

        def retire(p1):
            nonlocal pending, steps
            assert pending <= p1 <= n
            live = set(table)
            for j in p.by_end[pending:p1].tolist():
                retired[j] += 1
                assert all(i < appended for i in wanted[j]), ('block retired before its last read came', j)
                assert all(i in live for i in wanted[j]), ('a read of the block was dropped before it was retired', j)
            steps += p1 > pending
            pending = p1

        for k in chunks_of:
            retire(p.retire_upto(pending, last_start))
            if table:
                lo = p.drop_below(pending)
                table = [i for i in table if starts[i] >= lo]
            table += list(range(appended, appended + k))
            appended += k
            last_start = starts[appended - 1]
        assert appended == len(starts)
        between = steps
        retire(n)
        assert retired == [1] * n
        return between
    finally:
        p.close()


def _cuts(rng, n_reads, mode):
    if mode == 'one':
        return [1] * n_reads
    if mode == 'whole':
        return [n_reads]
    out, left = [], n_reads
    while left:
        k = int(min(left, rng.integers(1, max(2, n_reads // 3))))
        out.append(k)
        left -= k
    return out


def test_bimodal_walk_retires_complete_blocks_once(L):
    rng = np.random.default_rng(20261020)
    stepped = 0
    for trial in range(300):
        s, e, n_sites = _random_blocks(rng)
        starts = np.sort(rng.integers(1, n_sites + 200, int(rng.integers(1, 120))))
        if trial % 4 == 0:                                                     # reads exactly at the edges the rules compare with
            edges = np.concatenate([e, e - 1, np.maximum(1, s - CTX), np.maximum(1, s - CTX - 1)])
            starts = np.sort(np.concatenate([starts, edges]))
        for mode in ('one', 'random', 'whole'):
            stepped += _walk(L, s, e, starts, _cuts(rng, len(starts), mode))
    assert stepped > 1000                                                      # (blocks did retire between chunks, not only at the end)
    for name, (s, e) in BIM_TABLES.items():
        starts = sorted({max(1, v + d) for v in list(s) + list(e) for d in (-CTX - 1, -CTX, -1, 0, 1)})
        for mode in ('one', 'whole'):
            _walk(L, s, e, starts, _cuts(rng, len(starts), mode))


def test_bimodal_chunk_bound_covers_every_chunk(L):
    """{lines, words} is never below what a chunk holds: random chunks, chunks of the shortest legal line only (no chromosome, one digit
    of site and count, no pattern: 6 bytes), reads whose whole text is pattern, the longest pattern the reference writes (150) and longer"""
    rng = np.random.default_rng(3)
    chunks = ['\t1\t\t1\n' * k for k in (1, 2, 3, 7, 16, 17, 1000)]
    chunks += [_pat_line(1, 'C' * n, 1, chrom='') for n in (1, 15, 16, 17, CTX, 4096)]
    chunks += [_pat_line(1, 'C' * n, 1, chrom='') * 50 for n in (1, 16, 17)]
    chunks += [_pat_line(7, 'CT.' * 50, 3), _pat_line(7, 'T' * CTX, 3) * 9]
    for _ in range(300):
        k = int(rng.integers(1, 60))
        chunks.append(''.join(_pat_line(int(rng.integers(1, 10 ** int(rng.integers(1, 9)))), 'C' * int(rng.integers(0, rng.choice([3, 40, 400]))),
                                        int(rng.integers(0, 500)), chrom=str(rng.choice(['', 'chr1', 'chr22_random']))) for _ in range(k)))
    for ch in chunks:
        lines, words = _true_counts(ch)
        ub_lines, ub_words = _bound(L, len(ch))
        assert ub_lines == len(ch) // 6 + 1 and ub_words == len(ch) // 16 + ub_lines + 1
        assert lines <= ub_lines and words <= ub_words, (lines, words, ub_lines, ub_words, ch[:60])


def test_bimodal_refusals(L):
    def refused(s, e, min_len=1, null=False):
        p = BimPlan(L, s, e, min_len=min_len, null=null)
        assert p.h is None
        return p.rc, p.msg
    assert refused([], []) == (E_ARG, 'test_bimodal: no blocks')
    assert refused([1], [2], null=True) == (E_ARG, 'test_bimodal: no blocks')
    assert refused([1], [2], min_len=0) == (E_ARG, 'test_bimodal: min_len 0 < 1')
    assert refused([5, 0], [9, 4]) == (E_ARG, 'test_bimodal: block 2 has startCpG 0, endCpG 4 (1 <= startCpG < endCpG < 2^31)')
    assert refused([5], [5]) == (E_ARG, 'test_bimodal: block 1 has startCpG 5, endCpG 5 (1 <= startCpG < endCpG < 2^31)')
    assert refused([5, 6, 7], [9, 9, 2 ** 31]) == (E_ARG, 'test_bimodal: block 3 has startCpG 7, endCpG 2147483648 (1 <= startCpG < endCpG < 2^31)')
    assert refused([0], [4], min_len=-3) == (E_ARG, 'test_bimodal: min_len -3 < 1')           # (min_len is looked at before the blocks)


# ---------------------------------------------------------------------------------------------------------
# homog
# ---------------------------------------------------------------------------------------------------------
def _homog(L, s, e, edges=(0.0, 0.25, 0.75, 1.0), n_bins=None, min_cpgs=1, null=False, no_range=False):
    s, e = _i64(s), _i64(e)
    n = s.size
    r = np.ascontiguousarray(edges, dtype=np.float32)
    s32, e32, pm = (np.full(max(n, 1), -7, dtype=np.int32) for _ in range(3))
    last = C.c_int64(-7)
    msg = C.create_string_buffer(600)
    rc = L.patplan_homog(_ptr(s, null), _ptr(e, null), n, _ptr(r, no_range), len(edges) - 1 if n_bins is None else n_bins, min_cpgs,
                         s32.ctypes.data, e32.ctypes.data, pm.ctypes.data, C.addressof(last), msg, 600)
    return rc, msg.value.decode(), s32[:n].tolist(), e32[:n].tolist(), pm[:n].tolist(), last.value


def test_homog_plan_tables(L):
    """startCpG and endCpG as int32, the running maximum of endCpG (nested blocks keep it up), the last block's endCpG"""
    rng = np.random.default_rng(11)
    tables = [([7], [9]), ([1, 1, 1], [2, 2, 50]), ([10, 20, 30, 900], [1000, 25, 31, 901]), ([5, 2 ** 31 - 2], [9, 2 ** 31 - 1])]
    for _ in range(300):
        s, e, _n = _random_blocks(rng)
        order = sorted(range(len(s)), key=lambda j: (int(s[j]), int(e[j])))
        tables.append((s[order], e[order]))
    for s, e in tables:
        rc, msg, s32, e32, pm, last = _homog(L, s, e)
        want_pm = np.maximum.accumulate(_i64(e)).tolist()
        assert (rc, msg, s32, e32, pm, last) == (OK, '', [int(v) for v in s], [int(v) for v in e], want_pm, int(e[-1]))


def test_homog_refusals_in_order(L):
    def refused(*a, **k):
        rc, msg = _homog(L, *a, **k)[:2]
        return rc, msg
    assert refused([], []) == (E_ARG, 'homog: no blocks')
    assert refused([1], [2], null=True) == (E_ARG, 'homog: no blocks')
    assert refused([1], [2], no_range=True) == (E_ARG, 'homog: 3 bins (1..8)')
    assert refused([1], [2], n_bins=0) == (E_ARG, 'homog: 0 bins (1..8)')
    assert refused([1], [2], edges=np.linspace(0, 1, 10)) == (E_ARG, 'homog: 9 bins (1..8)')
    assert _homog(L, [1], [2], edges=np.linspace(0, 1, 9))[0] == OK
    assert refused([1], [2], edges=(0.0, 0.5, 0.5, 1.0)) == (E_ARG, 'homog: the range is not ascending')
    assert refused([1], [2], edges=(0.0, float('nan'), 1.0)) == (E_ARG, 'homog: the range is not ascending')
    assert refused([1], [2], min_cpgs=0) == (E_ARG, 'homog: min_cpgs 0 < 1')
    assert refused([3, 0], [9, 4]) == (E_ARG, 'homog: block 1 (in sorted order) has startCpG 0 < 1')
    assert refused([3], [3]) == (E_ARG, 'homog: block 0 (in sorted order) has endCpG 3 (startCpG 3)')
    assert refused([3, 4], [9, 2 ** 31]) == (E_ARG, 'homog: block 1 (in sorted order) has endCpG 2147483648 (startCpG 4)')
    assert refused([3, 2], [9, 9]) == (E_ARG, 'homog: blocks must be given sorted by (startCpG, endCpG) (block 1)')
    assert refused([3, 3], [9, 8]) == (E_ARG, 'homog: blocks must be given sorted by (startCpG, endCpG) (block 1)')
    # the order of the checks: blocks there at all, bins, edges, min_cpgs, then block by block
    assert refused([], [], n_bins=0, min_cpgs=0) == (E_ARG, 'homog: no blocks')
    assert refused([0], [0], edges=(1.0, 0.0), n_bins=0, min_cpgs=0) == (E_ARG, 'homog: 0 bins (1..8)')
    assert refused([0], [0], edges=(1.0, 0.0), min_cpgs=0) == (E_ARG, 'homog: the range is not ascending')
    assert refused([0], [0], min_cpgs=0) == (E_ARG, 'homog: min_cpgs 0 < 1')
    assert refused([0, 9], [0, 3]) == (E_ARG, 'homog: block 0 (in sorted order) has startCpG 0 < 1')


# ---------------------------------------------------------------------------------------------------------
# sample_stats
# ---------------------------------------------------------------------------------------------------------
def _stats(L, x0, x1, n_total, elem, n_samples=3, null=False, n_ranges=None):
    x0, x1 = _i64(x0), _i64(x1)
    n = x0.size if n_ranges is None else n_ranges
    o0, o1 = (np.full(max(n, 1), -7, dtype=np.int64) for _ in range(2))
    cum = np.full(max(n, 0) + 1, -7, dtype=np.int64)
    info = np.full(3, -7, dtype=np.int64)
    msg = C.create_string_buffer(600)
    rc = L.patplan_stats(_ptr(x0, null), _ptr(x1, null), n, n_total, elem, n_samples, o0.ctypes.data, o1.ctypes.data, cum.ctypes.data, info.ctypes.data, msg, 600)
    return rc, msg.value.decode(), o0[:max(n, 0)].tolist(), o1[:max(n, 0)].tolist(), cum.tolist(), info.tolist()


def _stats_restated(x0, x1, elem):
    """a range touches the aligned 16-byte vectors that hold any of its sites (8 sites of uint8 pairs, 4 of uint16 pairs), an empty one none"""
    S = 8 // elem
    per = [len({x // S for x in range(int(a), int(b))}) if b - a < 5000 else (int(b) + S - 1) // S - int(a) // S for a, b in zip(x0, x1)]
    cum = [0]
    for v in per:
        cum.append(cum[-1] + v)
    n_vec = cum[-1]
    return cum, [sum(int(b) - int(a) for a, b in zip(x0, x1)), n_vec, -(-n_vec // ST_TILE)]


def _check_stats(L, x0, x1, n_total, elem):
    rc, msg, o0, o1, cum, info = _stats(L, x0, x1, n_total, elem)
    want_cum, want_info = _stats_restated(x0, x1, elem)
    assert (rc, msg) == (OK, '')
    assert o0 == [int(v) for v in x0] and o1 == [int(v) for v in x1] and cum == want_cum and info == want_info
    return info


@pytest.mark.parametrize('elem', [1, 2])
def test_stats_plan_fixed_ranges(L, elem):
    S = 8 // elem
    assert _check_stats(L, [], [], 1000, elem) == [0, 0, 0]                                   # no ranges
    assert _check_stats(L, [0, 5, 5, 1000], [0, 5, 5, 1000], 1000, elem) == [0, 0, 0]          # empty ranges only
    for a in range(2 * S):                                                                     # edges on every residue of the vector
        for b in range(a, 4 * S + 1):
            _check_stats(L, [a], [b], 100, elem)
            _check_stats(L, [a, b, b], [b, b, 4 * S + 2], 100, elem)                           # ... with an empty range between two that meet
    # two ranges that meet inside one vector: the vector counts for each
    assert _check_stats(L, [0, S // 2], [S // 2, S], 100, elem) == [S, 2, 1]
    assert _check_stats(L, [1, S + 1], [S + 1, 3 * S], 100, elem)[1] == 2 + 2
    # exactly one tile of vectors; one tile and one vector (in one range, and with the extra vector from a range of one site)
    assert _check_stats(L, [0], [ST_TILE * S], 10 ** 6, elem) == [ST_TILE * S, ST_TILE, 1]
    assert _check_stats(L, [0], [ST_TILE * S + 1], 10 ** 6, elem) == [ST_TILE * S + 1, ST_TILE + 1, 2]
    assert _check_stats(L, [3, 90000], [3 + ST_TILE * S - S, 90001], 10 ** 6, elem) == [ST_TILE * S - S + 1, ST_TILE + 1, 2]
    assert _check_stats(L, [0, 90000], [ST_TILE * S - S, 90001], 10 ** 6, elem) == [ST_TILE * S - S + 1, ST_TILE, 1]
    assert _check_stats(L, [0], [2 ** 31 + 5], 2 ** 31 + 5, elem)[0] == 2 ** 31 + 5               # (sites are int64: no 2^31 limit here)


@pytest.mark.parametrize('elem', [1, 2])
def test_stats_plan_random_ranges(L, elem):
    rng = np.random.default_rng(20261021 + elem)
    for _ in range(300):
        n_total = int(rng.integers(1, rng.choice([40, 3000, 40000])))
        cuts = np.sort(rng.integers(0, n_total + 1, 2 * int(rng.integers(0, 25))))
        _check_stats(L, cuts[0::2], cuts[1::2], n_total, elem)


def test_stats_refusals(L):
    def refused(*a, **k):
        return _stats(L, *a, **k)[:2]
    assert refused([], [], 100, 1, n_ranges=-1) == (E_ARG, 'bad arguments to sample_stats')
    assert refused([1], [2], 100, 1, null=True) == (E_ARG, 'bad arguments to sample_stats')
    assert refused([0, -1], [4, 9], 100, 1) == (E_ARG, 'sample_stats: range 1 = sites [-1, 9) is outside the 100 resident sites or reversed')
    assert refused([9], [4], 100, 2) == (E_ARG, 'sample_stats: range 0 = sites [9, 4) is outside the 100 resident sites or reversed')
    assert refused([9], [101], 100, 1) == (E_ARG, 'sample_stats: range 0 = sites [9, 101) is outside the 100 resident sites or reversed')
    assert refused([0, 3], [4, 9], 100, 1) == (E_ARG, 'sample_stats: range 1 = sites [3, 9) begins before range 0 ends (4): ranges must be ascending and disjoint')
    assert refused([0], [8], 100, 1, n_samples=65536) == (E_ARG, 'too many sites / samples for one sample_stats call')
    assert _stats(L, [0], [8], 100, 1, n_samples=65535)[0] == OK
    # 2^31 tiles of 1024 vectors of 4 sites: one tile too many; one site less fits
    edge = 2 ** 31 * ST_TILE * 4
    assert refused([0], [edge - ST_TILE * 4 + 1], edge, 2) == (E_ARG, 'too many sites / samples for one sample_stats call')
    assert _stats(L, [0], [edge - ST_TILE * 4], edge, 2)[5] == [edge - ST_TILE * 4, 2 ** 31 * ST_TILE - ST_TILE, 2 ** 31 - 1]
