"""`wgbstools bed2beta` without a GPU: the restatement tests/bed2beta_ref.py (both of its forms) against every golden the reference's own
load_bed, left merge and trim_to_uint8 wrote (tests/golden/bed2beta_cases.json); csrc/bed2beta_plan.h and bed2beta_core.h (through
tests/native/bed2beta_host.cpp) — every refusal of the plan with its message, the line walk, the chromosome lookup, the locus search, the
packed word, and whole files through the functions the kernels call — against the restatement; the command line: help, flags, refusals,
output names, the skip without -f; and the goldens through a stand-alone program over the same headers (tests/native/san_bed2beta.cpp),
built plain and with ASan + UBSan."""
import ctypes as C
import hashlib
import json
import os.path as op
import shutil
import subprocess

import numpy as np
import pytest

import bed2beta_cases as BC
import bed2beta_ref as BR
import frag_cases as FC
from wgbs_tools_amd import bed2beta, wgbs_tools

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(HERE)
CSRC = op.join(ROOT, 'wgbs_tools_amd', 'csrc')
SRC = op.join(HERE, 'native', 'bed2beta_host.cpp')
LIB = op.join(HERE, 'native', 'libbed2beta_host.so')
DEPS = [SRC, op.join(HERE, 'native', 'bed2beta_run.h'), op.join(ROOT, 'include', 'wgbsseg.h')] + [
    op.join(CSRC, h) for h in ('bed2beta_plan.h', 'bed2beta_core.h', 'merge_plan.h', 'view_core.h', 'bed_fmt.h', 'block_plan.h')]
OK, E_ARG = 0, -1
P, I64, I32, U32, U64 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_uint64
EMPTY = 2 ** 64 - 1
LOCI = BC.loci().astype(np.uint32)
CHROMS = BC.CHROMS


@pytest.fixture(scope='module')
def L():
    """tests/native/libbed2beta_host.so (built when missing or older than its sources)"""
    if not op.isfile(LIB) or op.getmtime(LIB) < max(op.getmtime(d) for d in DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', SRC, '-o', LIB])
    lib = C.CDLL(LIB)
    lib.bb_plan.restype = C.c_int
    lib.bb_plan.argtypes = [P, I64, C.POINTER(C.c_char_p), P, P, I32, I32, P, C.POINTER(P), C.c_char_p, C.c_size_t]
    lib.bb_free.argtypes = [P]
    lib.bb_plan_table.argtypes = [P, P, P, P, C.c_char_p]
    lib.bb_find_chrom.restype = I32
    lib.bb_find_chrom.argtypes = [P, C.c_char_p, I64, I32]
    lib.bb_walk.restype = C.c_int
    lib.bb_walk.argtypes = [C.c_char_p, I64, I64, P]
    lib.bb_find_locus.restype = I64
    lib.bb_find_locus.argtypes = [P, I64, I64, I64]
    lib.bb_word.restype = U64
    lib.bb_word.argtypes = [U64, I64, I64]
    lib.bb_pair.restype = U32
    lib.bb_pair.argtypes = [U64]
    lib.bb_flags.restype = C.c_int
    lib.bb_flags.argtypes = [I32, C.c_char_p, C.c_size_t]
    lib.bb_chunk.restype = C.c_int
    lib.bb_chunk.argtypes = [U64, I64, C.c_char_p, C.c_size_t]
    lib.bb_report.restype = U64
    lib.bb_report.argtypes = [U64, C.c_int]
    lib.bb_refusal.restype = C.c_int
    lib.bb_refusal.argtypes = [U64, C.c_char_p, C.c_size_t]
    lib.bb_run.restype = U64
    lib.bb_run.argtypes = [P, P, C.c_char_p, I64, I32, P, P]
    return lib


@pytest.fixture(scope='module')
def golden():
    with open(op.join(HERE, 'golden', 'bed2beta_cases.json')) as f:
        return json.load(f)


class Plan:
    """a plan of tests/native/bed2beta_host.cpp"""

    def __init__(self, L, loci, names, ranges, flags=0):
        self.loci = np.ascontiguousarray(loci, dtype=np.uint32)
        lo = np.ascontiguousarray([r[0] for r in ranges], dtype=np.int64)
        hi = np.ascontiguousarray([r[1] for r in ranges], dtype=np.int64)
        raw = [n if isinstance(n, bytes) else n.encode() for n in names]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        info = np.full(5, -7, dtype=np.int64)
        msg = C.create_string_buffer(600)
        self.L, self.h, self.names = L, P(), raw
        self.rc = L.bb_plan(self.loci.ctypes.data, self.loci.size, arr, lo.ctypes.data if lo.size else None, hi.ctypes.data if hi.size else None, len(raw), flags,
                            info.ctypes.data, C.byref(self.h), msg, 600)
        self.msg = msg.value.decode()
        self.n, self.n_sites, self.n_words, self.arena, self.upload = info.tolist()

    def table(self):
        order, lo, hi = (np.zeros(self.n, dtype=np.int32) for _ in range(3))
        names = C.create_string_buffer(self.arena + self.n + 1)
        self.L.bb_plan_table(self.h, order.ctypes.data, lo.ctypes.data, hi.ctypes.data, names)
        return order.tolist(), lo.tolist(), hi.tolist(), names.raw[:self.arena + self.n].split(b'\0')[:self.n]

    def find(self, field, hint=-1):
        return self.L.bb_find_chrom(self.h, field, len(field), hint)

    def run(self, text, flags=0):
        out = np.full((self.n_sites, 2), 77, dtype=np.uint8)
        stats = np.zeros(6, dtype=np.int64)
        rep = self.L.bb_run(self.h, self.loci.ctypes.data, text, len(text), flags, out.ctypes.data, stats.ctypes.data)
        return out, dict(zip(('lines', 'matched', 'unknown_chrom', 'not_cpg', 'duplicates', 'sites_set'), stats.tolist())), rep

    def close(self):
        if self.h:
            self.L.bb_free(self.h)
            self.h = P()


def genome_plan(L):
    sizes = [s for _, s in CHROMS]
    hi = np.cumsum(sizes)
    return Plan(L, LOCI, [c for c, _ in CHROMS], list(zip((hi - sizes).tolist(), hi.tolist())))


def case_flag_bits(case, text):
    return (1 if case.get('add_one') else 0) | (2 if BR.is_header(text) else 0)


# ---- the restatement against the reference's own output ----
def test_every_case_has_a_golden(golden):
    assert sorted(golden) == sorted(BC.CASES)
    for name, case in BC.CASES.items():
        assert golden[name]['text_sha1'] == hashlib.sha1(BC.case_text(case)).hexdigest(), name
        assert golden[name]['flags'] == BC.case_flags(case) and golden[name]['n_sites'] == BC.N_SITES, name
        assert BR.is_header(BC.case_text(case)) == bool(case.get('header')), name


@pytest.mark.parametrize('name', sorted(BC.CASES))
def test_restatement_equals_golden(name, golden):
    rec, case = golden[name], BC.CASES[name]
    rows, st = BR.bed2beta(BC.case_text(case), LOCI, CHROMS, add_one=bool(case.get('add_one')))
    assert BC.sparse(rows) == rec['rows'], name
    assert hashlib.sha1(rows.tobytes()).hexdigest() == rec['out_sha1'], name
    assert st['lines'] == st['matched'] + st['unknown_chrom'] + st['not_cpg'] and st['sites_set'] == st['matched'] - st['duplicates']
    assert st['sites_set'] >= len(rec['rows'])                         # (a winning line of 0, 0 sets a site and shows nowhere)


def test_goldens_cover_what_the_issue_names(golden):
    g = {k: {r[0]: (r[1], r[2]) for r in v['rows']} for k, v in golden.items()}
    one = lambda chrom, p: int(np.searchsorted(BC.L1, p)) if chrom == 'chr1' else BC.N1 + int(np.searchsorted(BC.L2, p))
    assert g['header'] == g['no_header'] and len(g['header']) == 12
    assert len(g['add_one']) == 13 and one('chr1', BC.L1[200]) not in g['add_one'] and g['add_one'][one('chr2', BC.L2[9])] == (2, 2)
    assert g['dup_first_not_largest'] == {50: (3, 10), 51: (1, 1), BC.N1 + 50: (0, 255)}            # the first, not the largest
    assert g['dup_of_unmatched'] == {60: (2, 5)} and g['unknown_chrom'] == {5: (2, 3)}
    assert g['chr1_beside_chr10'] == {5: (2, 3), BC.N1 + 7: (5, 6)}
    s0, s1 = int(BC.COMMON[0]), int(BC.COMMON[1])
    assert g['same_position_two_chroms'] == {one('chr1', s0): (6, 7), one('chr2', s0): (1, 7), one('chr1', s1): (2, 9), one('chr2', s1): (8, 9)}
    assert g['first_and_last_cpg'] == {0: (1, 2), BC.N1 - 1: (3, 4), BC.N1: (5, 6), BC.N_SITES - 1: (7, 8)}
    assert g['one_off'] == {71: (4, 5)} and len(g['extra_columns']) == 9 and g['blank_lines'] == {90: (1, 2), 91: (2, 3), BC.N1 + 90: (3, 4)}
    t = g['totals']
    assert [t[100 + i] for i in range(4)] == [(255, 255)] * 4
    assert [t[BC.N1 + 100 + i] for i in range(12)] == [(254, 255), (99, 255), (254, 255), (254, 255), (0, 255), (0, 255), (254, 255), (0, 255), (127, 255),
                                                       (2, 255), (84, 255), (85, 255)]
    assert len(g['unsorted']) == 60 and len(g['big_mixed']) == BC.N_SITES and len(BC.case_text(BC.CASES['big_mixed'])) > 20 * 4096


def test_frames_restatement_equals_golden(golden, tmp_path):
    pytest.importorskip('pandas')
    frame = BR.dict_frame(LOCI, CHROMS)
    for name in ('header', 'add_one', 'dup_first_not_largest', 'totals', 'blank_lines', 'big_mixed'):
        case = BC.CASES[name]
        path = str(tmp_path / (name + '.bed'))
        with open(path, 'wb') as f:
            f.write(BC.case_text(case))
        rows = BR.bed2beta_frames(path, frame, add_one=bool(case.get('add_one')))
        assert hashlib.sha1(np.ascontiguousarray(rows).tobytes()).hexdigest() == golden[name]['out_sha1'], name


def test_restatement_refusals():
    good = b'chr1\t%d\t0\t1\t2\n' % BC.L1[3]
    for why, bad in ((BR.FEW_FIELDS, b'chr1\t5\t6\t1\n'), (BR.FEW_FIELDS, b'chr1\n'), (BR.NOT_NUMBER, b'chr1\t+5\t6\t1\t2\n'), (BR.NOT_NUMBER, b'chr1\t5\t6\t1.0\t2\n'),
                     (BR.NOT_NUMBER, b'chr1\t5\t6\t1\t2e3\n'), (BR.NOT_NUMBER, b'chr1\t5\t6\t1\t2\r\n'), (BR.NOT_NUMBER, b'chr1\t5\t6\t\t2\n'),
                     (BR.NOT_NUMBER, b'chr1\t%s\t6\t1\t2\n' % (b'1' * 19)), (BR.METH_GT_TOTAL, b'chr1\t5\t6\t3\t2\n'), (BR.TOTAL_RANGE, b'chr1\t5\t6\t3\t2147483648\n')):
        with pytest.raises(BR.Refused) as e:
            BR.bed2beta(good + bad + b'chrZ\tx\n', LOCI, CHROMS)
        assert (e.value.why, e.value.offset) == (why, len(good)), bad


# ---- bed2beta_plan.h ----
def test_plan_table_and_lookup(L):
    names = ['chr2', 'chr10', 'chr1', 'chrX', 'chr', 'chr1_gl000191_random', '1', 'chr19']
    ranges = [(10, 20), (0, 10), (20, 25), (25, 25), (30, 40), (40, 41), (41, 50), (25, 30)]
    p = Plan(L, np.arange(100, 150), names, ranges)
    try:
        assert (p.rc, p.msg, p.n, p.n_sites, p.n_words) == (OK, '', 8, 50, 56)
        order, lo, hi, sorted_names = p.table()
        assert sorted_names == sorted(n.encode() for n in names) and [names[k].encode() for k in order] == sorted_names
        assert [(lo[r], hi[r]) for r in range(8)] == [ranges[k] for k in order]
        assert p.upload == 9 * 4 + 8 * 8 + p.arena and p.arena == sum(len(n) for n in names)
        for k, n in enumerate(names):
            for hint in (-1, 0, 3, 7, 99):
                assert p.find(n.encode(), hint) == k, (n, hint)
        for miss in (b'', b'c', b'chr1 ', b'chr100', b'chr11', b'Chr1', b'chr1_gl000191_rando', b'chr1_gl000191_randomx', b'chrY', b'0', b'2', b'chr\0'):
            assert p.find(miss) == -1 and p.find(miss, 2) == -1, miss
    finally:
        p.close()
    one = Plan(L, [5, 9], ['a'], [(0, 2)])
    assert (one.rc, one.n_words, one.find(b'a'), one.find(b'b')) == (OK, 8, 0, -1)
    one.close()


def test_plan_refusals(L):
    loci = np.arange(100, 150)
    for names, ranges, what in (([], [], 'bedbeta: 0 chromosomes (1 .. 65535)'),
                                (['a', ''], [(0, 5), (5, 9)], 'bedbeta: chromosome 1 has an empty name'),
                                (['a', 'b\tc'], [(0, 5), (5, 9)], 'bedbeta: the name of chromosome 1 holds a tab or a newline'),
                                (['a\n'], [(0, 5)], 'bedbeta: the name of chromosome 0 holds a tab or a newline'),
                                (['a', 'b', 'a'], [(0, 5), (5, 9), (9, 12)], 'bedbeta: chromosomes 0 and 2 have the same name (a)'),
                                (['a', 'b'], [(0, 5), (4, 9)], 'bedbeta: the sites of chromosomes 0 and 1 overlap'),
                                (['a', 'b', 'c'], [(20, 30), (0, 5), (3, 21)], 'bedbeta: the sites of chromosomes 1 and 2 overlap'),
                                (['a', 'b'], [(0, 5), (5, 51)], 'bedbeta: chromosome 1 (b) has the sites [5, 51) (inside [0, 50))'),
                                (['a'], [(-1, 5)], 'bedbeta: chromosome 0 (a) has the sites [-1, 5) (inside [0, 50))'),
                                (['a'], [(6, 5)], 'bedbeta: chromosome 0 (a) has the sites [6, 5) (inside [0, 50))')):
        p = Plan(L, loci, names, ranges)
        assert (p.rc, p.msg) == (E_ARG, what) and not p.h, names
    many = Plan(L, loci, ['c%d' % k for k in range(65536)], [(0, 0)] * 65536)
    assert (many.rc, many.msg) == (E_ARG, 'bedbeta: 65536 chromosomes (1 .. 65535)')
    top = Plan(L, loci, ['c%d' % k for k in range(65535)], [(0, 0)] * 65535)
    assert top.rc == OK and top.find(b'c65534') == 65534 and top.find(b'c65535') == -1
    top.close()
    bad = loci.copy()
    bad[30] = bad[29]
    p = Plan(L, bad, ['a', 'b'], [(0, 30), (30, 50)])                   # the loci restart at a chromosome's first site: no refusal there
    assert p.rc == OK
    p.close()
    p = Plan(L, bad, ['a', 'b'], [(0, 25), (25, 50)])
    assert (p.rc, p.msg) == (E_ARG, 'bedbeta: the loci of chromosome 1 (b) do not ascend at site 30 (129 after 129)')
    p = Plan(L, loci, ['a'], [(0, 50)], flags=4)
    assert (p.rc, p.msg) == (E_ARG, 'bedbeta: unknown flags 4 (ADD_ONE = 1, HEADER = 2)')
    p = Plan(L, np.zeros(0), ['a'], [(0, 0)])
    assert (p.rc, p.msg) == (E_ARG, 'bedbeta: 0 sites (1 .. 2^31 - 1)')
    msg = C.create_string_buffer(300)
    assert L.bb_flags(3, msg, 300) == OK and L.bb_flags(-1, msg, 300) == E_ARG
    assert L.bb_chunk(0, 2 ** 47, msg, 300) == OK and L.bb_chunk(2 ** 47 - 5, 5, msg, 300) == OK
    assert L.bb_chunk(2 ** 47 - 5, 6, msg, 300) == E_ARG and msg.value == b'bedbeta_feed: more than 2^47 bytes of text in one file'


def test_refusal_messages(L):
    msg = C.create_string_buffer(400)
    assert L.bb_refusal(EMPTY, msg, 400) == 0
    for why, what in ((1, 'has fewer than five tab-separated fields'), (2, 'has a start, #meth or #total that is not 1 to 18 decimal digits and nothing else'),
                      (3, 'has a #total above 2^31 - 1'), (4, 'has #meth above #total')):
        for off in (0, 77, 2 ** 47 - 1):
            rep = L.bb_report(off, why)
            assert rep == off << 8 | why and rep < EMPTY and L.bb_refusal(rep, msg, 400) == 1
            assert msg.value.decode() == 'failed in bed2beta: the line at byte offset %d of the input %s' % (off, what)
    assert L.bb_report(5, 4) < L.bb_report(6, 1)                        # the lowest offset wins, whatever its reason


# ---- bed2beta_core.h ----
def walk(L, text, p=0):
    out = np.zeros(5, dtype=np.int64)
    return L.bb_walk(text, len(text), p, out.ctypes.data), out.tolist()


def test_line_walk(L):
    assert walk(L, b'chr1\t100\t102\t3\t7\n') == (0, [0, 4, 100, 3, 7])
    assert walk(L, b'chr1\t100\tanything at all, 1e5 +-\t3\t7\tmore\t\tstuff\n') == (0, [0, 4, 100, 3, 7])
    assert walk(L, b'chr1\t100\t\t3\t7') == (0, [0, 4, 100, 3, 7])                       # an empty field 3; no newline before n
    assert walk(L, b'\t0\t\t0\t0\n') == (0, [0, 0, 0, 0, 0])                            # an empty chromosome: no genome has it
    assert walk(L, b'x\nchr2\t5\t6\t1\t2\nchr1\tz\n', 2) == (0, [2, 4, 5, 1, 2])
    assert walk(L, b'c\t%s\t.\t%s\t2147483647\n' % (b'9' * 18, b'0' * 18)) == (0, [0, 1, 10 ** 18 - 1, 0, 2 ** 31 - 1])
    for text, why in ((b'chr1\t100\t102\t3\n', 1), (b'chr1\n', 1), (b'chr1 100 102 3 7\n', 1), (b'chr1\tx\ty\n7\t8\n', 1),
                      (b'chr1\t+100\t102\t3\t7\n', 2), (b'chr1\t100\t102\t-3\t7\n', 2), (b'chr1\t100\t102\t3\t7.0\n', 2), (b'chr1\t100\t102\t3\t7\r\n', 2),
                      (b'chr1\t1e2\t102\t3\t7\n', 2), (b'chr1\t\t102\t3\t7\n', 2), (b'chr1\t100\t102\t3\t\n', 2), (b'chr1\t100\t102\t3\t\t9\n', 2),
                      (b'chr1\t 100\t102\t3\t7\n', 2), (b'chr1\t%s\t102\t3\t7\n' % (b'1' * 19), 2), (b'chr1\t100\t102\t3\t%s\n' % (b'0' * 19), 2),
                      (b'chr1\t100\t102\t3\t2147483648\n', 3), (b'chr1\t100\t102\t9\t999999999999999999\n', 3),
                      (b'chr1\t100\t102\t8\t7\n', 4), (b'chr1\t100\t102\t2147483647\t2147483646\n', 4)):
        assert walk(L, text)[0] == why, text
    assert walk(L, b'chr1\tx\ty\tz\n')[0] == 1 and walk(L, b'chr1\tx\ty\tz\t\n')[0] == 2       # too few fields comes before what they hold


def test_locus_search_and_word(L):
    loci = np.array([5, 9, 9, 12, 4000000000, 4294967295, 3, 8], dtype=np.uint32)
    f = lambda lo, hi, p: L.bb_find_locus(loci.ctypes.data, lo, hi, p)
    assert [f(0, 2, p) for p in (4, 5, 6, 9, 10)] == [-1, 0, -1, 1, -1]
    assert [f(2, 6, p) for p in (9, 12, 13, 4000000000, 4294967295, 4294967296, 2 ** 32 + 9, -1, 10 ** 18)] == [2, 3, -1, 4, 5, -1, -1, -1, -1]
    assert [f(6, 8, p) for p in (3, 5, 8, 9)] == [6, -1, 7, -1] and f(3, 3, 12) == -1
    for off in (0, 1, 4095, 2 ** 31, 2 ** 47 - 1):
        for m, c in ((0, 0), (3, 7), (255, 255), (0, 256), (100, 256), (256, 256), (599, 600), (1, 2 ** 31 - 1), (2 ** 31 - 2, 2 ** 31 - 1), (2 ** 31 - 1, 2 ** 31 - 1)):
            w = L.bb_word(off, m, c)
            m8, c8 = BR.trim(m, c)
            assert w == off << 16 | m8 << 8 | c8 and w != EMPTY and L.bb_pair(w) == m8 | c8 << 8, (off, m, c)
    assert L.bb_pair(EMPTY) == 0
    assert L.bb_word(7, 9, 9) < L.bb_word(8, 0, 1) and L.bb_word(2 ** 47 - 1, 255, 255) < EMPTY      # the offset decides; no word is the empty marker


def test_whole_files_on_the_host(L, golden):
    p = genome_plan(L)
    try:
        for name, case in BC.CASES.items():
            text = BC.case_text(case)
            rows, st, rep = p.run(text, case_flag_bits(case, text))
            want, want_st = BR.bed2beta(text, LOCI, CHROMS, add_one=bool(case.get('add_one')))
            assert rep == EMPTY and hashlib.sha1(rows.tobytes()).hexdigest() == golden[name]['out_sha1'] and st == want_st, name
        rng = np.random.default_rng(20261021)
        for _ in range(40):
            text, add_one = BC.random_world(rng)
            rows, st, rep = p.run(text, (1 if add_one else 0) | (2 if BR.is_header(text) else 0))
            want, want_st = BR.bed2beta(text, LOCI, CHROMS, add_one=add_one)
            assert rep == EMPTY and np.array_equal(rows, want) and st == want_st
        good = b'chr1\t%d\t0\t1\t2\n' % BC.L1[3]
        for why, bad in ((1, b'chr1\t5\n'), (2, b'chr1\t5\t6\t1\tx\n'), (3, b'chrQ\t5\t6\t1\t4294967296\n'), (4, b'chrQ\t5\t6\t3\t2\n')):
            assert p.run(good + bad + good + b'zz\n')[2] == len(good) << 8 | why
        assert p.run(b'chr\tstart\n' + good, 2)[2] == EMPTY and p.run(b'chr\tstart\n' + good, 0)[2] == 1      # the header is dropped unread
    finally:
        p.close()


# ---- the command line ----
FLAGS = ('--add_one', '--outdir', '--force', '--genome', '--device', '--inflate', '--debug')


def test_cli_surface(capsys):
    assert 'bed2beta' in wgbs_tools.COMMANDS and 'bed2beta' in wgbs_tools.REFERENCE_ONLY
    with pytest.raises(SystemExit) as e:
        wgbs_tools.main(['wgbstools', 'bed2beta', '-h'])
    assert e.value.code == 0
    out = capsys.readouterr()
    assert 'not part of this build' not in out.err and 'Convert bed[.gz] file[s] to beta file[s].' in out.out
    for flag in FLAGS:
        assert flag in out.out, flag
    args = bed2beta.parse_args(['a.bed', 'b.bed.gz', '--add_one', '-o', 'out', '-f', '--genome', 'hg19', '--inflate', 'device', '--device', '1'])
    assert (args.bed_paths, args.add_one, args.outdir, args.force, args.genome, args.inflate, args.device, args.debug) == (
        ['a.bed', 'b.bed.gz'], True, 'out', True, 'hg19', 'device', 1, False)
    with pytest.raises(SystemExit):
        bed2beta.parse_args([])
    capsys.readouterr()
    for word in ('failed in bed2beta:', 'fewer than five fields', '18 digits', '#meth >', '2^31 - 1', '-d / --debug', 'tabix', 'duplicates', 'BGZF'):
        assert word in bed2beta.__doc__, word
    assert bed2beta.out_path_of('/x/y/a.bed.gz', 'o') == op.join('o', 'a.beta') and bed2beta.out_path_of('s.cov.bed', '.') == op.join('.', 's.cov.beta')


def test_header_peek(tmp_path):
    import gzip
    for text, want in ((b'chr\tstart\tend\n', True), (b'chr1\t100\t102\t1\t2\n', False), (b'chr1\n', True), (b'chr1\t+100\t102\n', True), (b'chr1\t1e3\t5\n', True),
                       (b'chr1\t\t5\n', True), (b'chr1\t007', False), (b'\nchr1\t5\t6\t1\t2\n', True), (b'chr1\t\xc2\xb2\t5\n', True)):
        for gz in (False, True):
            path = str(tmp_path / ('p.bed.gz' if gz else 'p.bed'))
            with (gzip.open if gz else open)(path, 'wb') as f:
                f.write(text)
            assert bed2beta.first_line_is_header(path) is want and BR.is_header(text) is want, text


def test_cli_refusals_names_and_skip(capsys, tmp_path):
    ref, _ = FC.genome_dir(str(tmp_path))
    bed = tmp_path / 'a.bed'
    bed.write_bytes(BC.case_text(BC.CASES['no_header']))
    empty = tmp_path / 'e.bed'
    empty.write_bytes(b'')
    out = tmp_path / 'out'
    out.mkdir()
    for argv, what in (([str(bed), '-d', '--genome', ref], 'bed2beta -d / --debug is not part of this build (it needs tabix)'),
                       ([str(tmp_path / 'missing.bed'), '--genome', ref], 'No such file'),
                       ([str(bed), '-o', str(tmp_path / 'nowhere'), '--genome', ref], 'Invalid output dir'),
                       ([str(empty), '-o', str(out), '--genome', ref], 'e.bed is empty')):
        assert wgbs_tools.main(['wgbstools', 'bed2beta'] + argv) == 1, argv
        err = capsys.readouterr().err
        assert 'Invalid input argument' in err and what in err, (argv, err)
    assert not list(out.iterdir())
    # an existing output without -f: skipped with the reference's line, nothing touched (and no device asked for)
    (out / 'a.beta').write_bytes(b'kept')
    gz = tmp_path / 'a.bed.gz'
    gz.write_bytes(b'')
    assert wgbs_tools.main(['wgbstools', 'bed2beta', str(bed), str(gz), '-o', str(out), '--genome', ref]) == 0
    err = capsys.readouterr().err
    assert err.count(f"File {out / 'a.beta'} already exists. Skipping it. Use [-f] flag to force overwrite.") == 2 and '[wt bed] Converting a.bed...' in err
    assert (out / 'a.beta').read_bytes() == b'kept'


# ---- the shared headers under the sanitizers ----
def _have_sanitizers():
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null', '-fsanitize=address,undefined'], input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason='no g++ with sanitizer runtimes')
def test_goldens_through_the_headers_under_sanitizers(golden, tmp_path):
    """tests/native/san_bed2beta.cpp — the whole of `bed2beta` on the host by the functions the kernels call, every array of exactly its
    size — built plain and with ASan + UBSan: both write every golden's bytes, and refuse a malformed line with the engine's message; exit
    status 0 says that no read or write left its array"""
    loci, chroms = str(tmp_path / 'loci.u32'), str(tmp_path / 'chroms.tsv')
    LOCI.tofile(loci)
    with open(chroms, 'w') as f:
        f.write(''.join('%s\t%d\n' % c for c in CHROMS))
    texts = {name: BC.case_text(case) for name, case in BC.CASES.items()}
    texts['no_last_newline'] = BC.case_text(BC.CASES['unsorted']).rstrip(b'\n')
    for kind, flags in (('plain', []), ('asan_ubsan', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exe = str(tmp_path / ('san_bed2beta_' + kind))
        subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-I', CSRC, op.join(HERE, 'native', 'san_bed2beta.cpp'), '-o', exe] + flags)
        env = {'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'}
        for name, text in texts.items():
            case = BC.CASES.get(name, BC.CASES['unsorted'])
            bed = str(tmp_path / (name + '.bed'))
            with open(bed, 'wb') as f:
                f.write(text)
            r = subprocess.run([exe, bed, loci, chroms, str(case_flag_bits(case, text))], capture_output=True, timeout=120, env=env)
            assert r.returncode == 0, (kind, name, r.stderr[-3000:])
            want = golden[name if name in golden else 'unsorted']
            assert hashlib.sha1(r.stdout).hexdigest() == want['out_sha1'], (kind, name)
            st = BR.bed2beta(text, LOCI, CHROMS, add_one=bool(case.get('add_one')))[1]
            assert r.stderr.decode() == 'stats %d %d %d %d %d %d\n' % tuple(st[k] for k in ('lines', 'matched', 'unknown_chrom', 'not_cpg', 'duplicates', 'sites_set')), (kind, name)
        bad = str(tmp_path / 'bad.bed')
        with open(bad, 'wb') as f:
            f.write(b'chr1\t5\t6\t1\t2\nchr1\t5\t6\t1')                   # the file ends inside a line of four fields
        r = subprocess.run([exe, bad, loci, chroms, '0'], capture_output=True, timeout=120, env=env)
        assert r.returncode == 4 and r.stdout == b'', (kind, r.stderr[-3000:])
        assert r.stderr.decode() == 'failed in bed2beta: the line at byte offset 13 of the input has fewer than five tab-separated fields\n', kind
