"""`wgbstools view` / `cview` without a GPU: the restatement tests/view_ref.py against every golden the reference's cview, sort and
collapse script wrote (tests/golden/view_cases.json); csrc/view_core.h and view_plan.h (through tests/native/view_host.cpp) against
the restatement — the cut rule on random reads and on the corners of the interval, the comparator against a live
`LC_ALL=C sort -k2,2n -k3,3`, the run-head test and the line length — and every refusal of the plan; the command line's refusals; the goldens
through a stand-alone program over the same two headers (tests/native/san_view.cpp), built plain and with ASan + UBSan."""
import ctypes as C
import hashlib
import json
import os
import os.path as op
import shutil
import subprocess

import numpy as np
import pytest

import view_cases as VC
import view_ref as VR
from wgbs_tools_amd import view, wgbs_tools

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(HERE)
CSRC = op.join(ROOT, 'wgbs_tools_amd', 'csrc')
SRC = op.join(HERE, 'native', 'view_host.cpp')
LIB = op.join(HERE, 'native', 'libview_host.so')
DEPS = [SRC, op.join(ROOT, 'include', 'wgbsseg.h')] + [op.join(CSRC, h) for h in ('view_core.h', 'view_plan.h', 'bed_fmt.h', 'block_plan.h')]
OK, E_ARG, E_CAPACITY = 0, -1, -6
P, I64, I32, U32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32
STRICT, STRIP, NO_GAPS, SORT = 1, 2, 4, 8
RUN = 512


@pytest.fixture(scope='module')
def L():
    """tests/native/libview_host.so (built when missing or older than its sources)"""
    if not op.isfile(LIB) or op.getmtime(LIB) < max(op.getmtime(d) for d in DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', SRC, '-o', LIB])
    lib = C.CDLL(LIB)
    lib.view_constants.argtypes = [P]
    lib.view_cut.argtypes = [I64, C.c_char_p, I64, I64, I64, I32, I64, P]
    lib.view_table.restype = P
    lib.view_table.argtypes = [I64, C.c_char_p, P, C.c_char_p, P, P, P]
    lib.view_table_free.argtypes = [P]
    for f in (lib.view_cmp, lib.view_less, lib.view_run_head):
        f.restype = C.c_int
        f.argtypes = [P, U32, U32]
    lib.view_line_len.restype = U32
    lib.view_line_len.argtypes = [P, U32, I64]
    lib.view_sort.argtypes = [P, P]
    lib.view_int_text.restype = C.c_int
    lib.view_int_text.argtypes = [I64, C.c_char_p]
    lib.view_plan.restype = C.c_int
    lib.view_plan.argtypes = [I64, I64, I32, I32, I64, P, C.c_char_p, C.c_size_t]
    lib.view_plan_chunk.restype = C.c_int
    lib.view_plan_chunk.argtypes = [I64, I64, C.c_char_p, C.c_size_t]
    lib.view_plan_read.restype = C.c_int
    lib.view_plan_read.argtypes = [I64, I64, I64, C.c_int, C.c_char_p, C.c_size_t]
    for f in (lib.view_chunk_records, lib.view_runs, lib.view_slabs):
        f.restype = I64
        f.argtypes = [I64]
    lib.view_grow.restype = I64
    lib.view_grow.argtypes = [I64, I64]
    lib.view_slab_len.restype = I64
    lib.view_slab_len.argtypes = [I64, I64]
    lib.view_merge_passes.restype = C.c_int
    lib.view_merge_passes.argtypes = [I64]
    return lib


@pytest.fixture(scope='module')
def golden():
    with open(op.join(HERE, 'golden', 'view_cases.json')) as f:
        return json.load(f)


class Table:
    """lines (chrom, rs, pattern, count) as view_host's record table"""

    def __init__(self, L, lines):
        self.L, self.n = L, len(lines)
        clen = np.array([len(x[0]) for x in lines], dtype=np.uint32)
        plen = np.array([len(x[2]) for x in lines], dtype=np.uint32)
        rs = np.array([x[1] for x in lines], dtype=np.int64)
        cnt = np.array([x[3] for x in lines], dtype=np.int32)
        self.h = L.view_table(self.n, b''.join(x[0] for x in lines), clen.ctypes.data, b''.join(x[2] for x in lines), plen.ctypes.data,
                              rs.ctypes.data, cnt.ctypes.data)

    def sort(self):
        perm = np.zeros(self.n, dtype=np.uint32)
        self.L.view_sort(self.h, perm.ctypes.data)
        return perm.tolist()

    def close(self):
        self.L.view_table_free(self.h)


def flags_of(strict=False, strip=False, no_gaps=False, **_):
    return (STRICT if strict else 0) | (STRIP if strip else 0) | (NO_GAPS if no_gaps else 0)


def host_cut(L, rs, pat, s, e, **kw):
    out = np.zeros(3, dtype=np.int64)
    L.view_cut(rs, pat, len(pat), s, e, flags_of(**kw), kw.get('min_len', 1), out.ctypes.data)
    rs2, first, ln = out.tolist()
    return (rs2, pat[first:first + ln]) if ln else None


# ---- the restatement against the reference's own output ----
def test_every_case_has_a_golden(golden):
    assert sorted(golden) == sorted(VC.CASES)
    for name, case in VC.CASES.items():
        assert golden[name]['pat_sha1'] == hashlib.sha1(VC.case_pat(case)).hexdigest(), name
        assert golden[name]['where'] == VC.case_where(case) and golden[name]['flags'] == case['flags'], name


@pytest.mark.parametrize('name', sorted(VC.CASES))
def test_restatement_equals_golden(name, golden):
    rec = golden[name]
    s, e = rec['sites']
    got = VR.view(VC.case_pat(VC.CASES[name]), s, e, sort=rec['sorted'], **VC.flag_kwargs(rec['flags']))
    assert got.decode() == rec['stdout']


def test_goldens_cover_what_the_issue_names(golden):
    assert golden['empty_region']['stdout'] == ''
    starts = [int(ln.split('\t')[1]) for ln in golden['wg_strip']['stdout'].splitlines()]
    assert starts != sorted(starts)                                  # --strip without a sort leaves the ascending order
    rec = golden['signed_strict']
    kept = VR.survivors(VC.case_pat(VC.CASES['signed_strict']), *rec['sites'], strict=True)
    runs = {}
    for chrom, rs, pat, count in kept:
        runs[(chrom, rs, pat)] = runs.get((chrom, rs, pat), 0) + count
    assert sum(1 for v in runs.values() if v <= 0) > 10 and sum(1 for v in runs.values() if v > 0) == rec['stdout'].count('\n')
    plain, unsorted = golden['sites_plain']['stdout'], golden['sites_no_sort']['stdout']
    assert plain != unsorted and sorted(plain.splitlines()) != sorted(unsorted.splitlines())     # (the sort lets more lines collapse)


def test_restatement_refusals():
    good = b'chr1\t1\tCCCC\t1\nchr1\t3\tTTTT\t2\n'
    for bad in (b'chr1\t5\tCT\n', b'chr1\tx\tCT\t3\n', b'chr1\t5\tCT\t\n', b'chr1\t5\t\t3\n', b'chr1\t5\tCT\t3\t9\n', b'chr1\t5\tCT\t3\r\n',
                b'chr1\t5\tCT\t3 \n', b'chr1\t5\tCT\t2147483648\n'):
        with pytest.raises(VR.Refused) as e:
            VR.view(good + bad + b'chr1\t2\tC\t1\n', 1, 100)
        assert (e.value.kind, e.value.offset) == ('bad', len(good)), bad
    with pytest.raises(VR.Refused) as e:
        VR.view(good + b'chr1\t2\tCCC\t1\n', 1, 2)                    # the whole genome too
    assert (e.value.kind, e.value.offset) == ('desc', len(good))
    with pytest.raises(VR.Refused) as e:
        VR.view(b'chr1\t5\tC\t2147483647\n' * 465662, 1, 9)
    assert e.value.kind == 'sum'
    assert VR.view(b'chr1\t5\tC\t2147483647\n' * 465661, 1, 9) == b'chr1\t5\tC\t%d\n' % (465661 * (2 ** 31 - 1))


# ---- view_core.h against the restatement ----
def test_constants(L):
    k = np.zeros(8, dtype=np.int64)
    L.view_constants(k.ctypes.data)
    assert k.tolist() == [RUN, 16, 8 << 20, 1 << 20, 7, VR.MAX_SUM, 2 ** 31 - 1, 32]


def test_cut_rule_corners(L):
    s, e = 100, 110
    every = [dict(), dict(strict=True), dict(strip=True), dict(strict=True, strip=True), dict(strict=True, strip=True, min_len=3),
             dict(no_gaps=True), dict(strict=True, no_gaps=True), dict(min_len=4)]
    corners = [(95, b'CTCTC'), (96, b'CTCTC'),                       # ends at s - 1, at s
               (109, b'TC'), (110, b'TC'),                           # starts at e - 1, at e
               (90, b'C' * 5 + b'T' * 5 + b'.CH.TTC.C.' + b'H' * 8), # spans the whole interval, clipped at both ends
               (101, b'....'), (98, b'CC...'), (98, b'..C..T...'), (104, b'.'), (99, b'.C'), (108, b'C..'), (100, b'C.T'), (1, b'C' * 99), (1, b'C' * 100)]
    for kw in every:
        for rs, pat in corners:
            assert host_cut(L, rs, pat, s, e, **kw) == VR.cut(rs, pat, s, e, **kw), (kw, rs, pat)
    assert host_cut(L, 90, corners[4][1], s, e, strict=True) == (100, b'.CH.TTC.C.')
    assert host_cut(L, 90, corners[4][1], s, e, strict=True, strip=True) == (101, b'CH.TTC.C')
    assert host_cut(L, 95, b'CTCTC', s, e) is None and host_cut(L, 96, b'CTCTC', s, e, strict=True) == (100, b'C')
    assert host_cut(L, 109, b'TC', s, e, strict=True) == (109, b'T') and host_cut(L, 110, b'TC', s, e) is None


def test_cut_rule_random(L):
    rng = np.random.default_rng(20261101)
    for _ in range(4000):
        s = int(rng.integers(1, 60))
        e = s + int(rng.integers(1, 30))
        rs = int(rng.integers(-5, 100))
        pat = VC.random_pattern(rng, int(rng.integers(1, 40)), float(rng.choice([0.1, 0.5, 0.9]))).encode()
        kw = dict(strict=bool(rng.integers(2)), strip=bool(rng.integers(2)), no_gaps=bool(rng.integers(2)), min_len=int(rng.choice([1, 2, 3, 9])))
        assert host_cut(L, rs, pat, s, e, **kw) == VR.cut(rs, pat, s, e, **kw), (rs, pat, s, e, kw)


def _sort_lines():
    rng = np.random.default_rng(20261102)
    long_a, long_b = b'CT' * 40 + b'C', b'CT' * 40 + b'T'              # first differ beyond byte 64
    lines = [(b'chr1', 7, b'CT', 1), (b'chr1', 7, b'CTC', 2), (b'chr1', 7, b'C', 3), (b'chr10', 7, b'CT', 4), (b'chr1', 7, b'CT', 5),
             (b'chr2', 7, b'CT', 6), (b'chr1', 7, long_b, 7), (b'chr1', 7, long_a, 8), (b'chr1', 7, long_a[:-1], 9), (b'chr1', 10, b'.', 1),
             (b'chr1', 9, b'T', 1), (b'chr1', 100, b'C', 1), (b'chr1', 99, b'T', 1), (b'chr1', -2, b'TTTT', 1), (b'chr1', 0, b'C', 2)]
    for _ in range(600):
        lines.append((b'chr%d' % rng.choice([1, 2, 10, 11]), int(rng.integers(1, 40)), VC.random_pattern(rng, int(rng.integers(1, 6))).encode(),
                      int(rng.integers(1, 50))))
    order = rng.permutation(len(lines))
    return [lines[i] for i in order]


def test_comparator_equals_live_sort(L):
    lines = _sort_lines()
    t = Table(L, lines)
    try:
        perm = t.sort()
        got = [lines[i] for i in perm]
        text = b''.join(b'%s\t%d\t%s\t%d\n' % ln for ln in lines)
        live = subprocess.run(['sort', '-k2,2n', '-k3,3'], input=text, stdout=subprocess.PIPE, check=True, env=dict(os.environ, LC_ALL='C')).stdout
        # lines tied in everything but the count may stand in either order: compared without the count, and as multisets with it
        assert [ln[:3] for ln in got] == [tuple(x if k != 1 else int(x) for k, x in enumerate(r.split(b'\t')[:3])) for r in live.splitlines()]
        assert sorted(got) == sorted(lines)
        assert got == sorted(lines, key=VR.sort_key)                   # and ties keep the input order
        n = len(lines)
        for i, j in np.random.default_rng(3).integers(0, n, (3000, 2)).tolist():
            ki, kj = VR.sort_key(lines[i]), VR.sort_key(lines[j])
            assert L.view_cmp(t.h, i, j) == (ki > kj) - (ki < kj)
            assert L.view_less(t.h, i, j) == int((ki, i) < (kj, j))
            assert L.view_run_head(t.h, i, j) == int(ki != kj)
    finally:
        t.close()


def test_comparator_corners(L):
    long_a, long_b = b'C' * 70 + b'T', b'C' * 70 + b'C'
    lines = [(b'chr1', 5, b'CT', 1), (b'chr1', 5, b'CTC', 1), (b'chr1', 5, long_a, 1), (b'chr1', 5, long_b, 1), (b'chr1', 5, b'CT', 9),
             (b'chr10', 5, b'CT', 1), (b'chr1', 6, b'C', 1)]
    t = Table(L, lines)
    try:
        assert L.view_less(t.h, 0, 1) == 1 and L.view_less(t.h, 1, 0) == 0          # a prefix first
        assert L.view_less(t.h, 3, 2) == 1 and L.view_cmp(t.h, 2, 3) == 1           # the whole pattern, not its first 64 bytes
        assert L.view_cmp(t.h, 0, 4) == 0 and L.view_less(t.h, 0, 4) == 1 and L.view_less(t.h, 4, 0) == 0 and L.view_run_head(t.h, 0, 4) == 0
        assert L.view_less(t.h, 0, 5) == 1 and L.view_run_head(t.h, 0, 5) == 1      # chr1 before chr10; another run
        assert L.view_less(t.h, 2, 6) == 1
        assert L.view_less(t.h, 0, 0) == 0
    finally:
        t.close()


def test_line_length_and_numbers(L):
    lines = [(b'chr1', 5, b'CT', 1), (b'chrUn_gl000220', 28217448, b'C' * 300, 1), (b'', 0, b'.', 1), (b'chr1', -12, b'CCCC', 1)]
    t = Table(L, lines)
    try:
        for i, (chrom, rs, pat, _) in enumerate(lines):
            for total in (1, 9, 10, 2 ** 31 - 1, 3 * (2 ** 31 - 1), 10 ** 15 - 1):
                assert L.view_line_len(t.h, i, total) == len(b'%s\t%d\t%s\t%d\n' % (chrom, rs, pat, total))
            assert L.view_line_len(t.h, i, 0) == 0 and L.view_line_len(t.h, i, -7) == 0
    finally:
        t.close()
    buf = C.create_string_buffer(32)
    for v in (0, 7, -1, -10, 99, 100, 2 ** 31 - 1, -(2 ** 31)):
        n = L.view_int_text(v, buf)
        assert buf.raw[:n] == b'%d' % v


# ---- view_plan.h ----
def _plan(L, *a):
    info = np.full(5, -7, dtype=np.int64)
    msg = C.create_string_buffer(600)
    rc = L.view_plan(*a, info.ctypes.data, msg, 600)
    return rc, msg.value.decode(), info.tolist()


def test_plan_and_refusals(L):
    assert _plan(L, 1, 4001, STRICT | SORT, 3, 0) == (OK, '', [1, 4001, STRICT | SORT, 3, 1 << 20])
    assert _plan(L, 5, 6, 0, 1, 17)[2][4] == 17 and _plan(L, 5, 6, 0, 1, -1)[2][4] == 1 << 20
    assert _plan(L, 0, 6, 0, 1, 0)[:2] == (E_ARG, 'view: the interval starts at site 0 (sites count from 1)')
    assert _plan(L, 6, 6, 0, 1, 0)[:2] == (E_ARG, 'view: the interval [6, 6) is empty')
    assert _plan(L, 6, 2 ** 31, 0, 1, 0)[:2] == (E_ARG, 'view: the interval ends at site 2147483648 (at most 2147483647)')
    assert _plan(L, 1, 6, 16, 1, 0)[:2] == (E_ARG, 'view: unknown flags 16')
    assert _plan(L, 1, 6, 0, 0, 0)[:2] == (E_ARG, 'view: min_len 0 (at least 1)')
    assert _plan(L, 1, 6, 0, 1, 2 ** 31)[:2] == (E_ARG, 'view: 2147483648 initial records (below 2^31)')
    msg = C.create_string_buffer(600)
    assert L.view_plan_chunk(0, 64 << 20, msg, 600) == OK
    assert L.view_plan_chunk(0, 2 ** 31, msg, 600) == E_ARG and msg.value == b'view: a chunk of 2147483648 bytes (at most 2147483647)'
    assert L.view_plan_chunk(2 ** 31 - 10, 70, msg, 600) == E_CAPACITY and msg.value == b'view: more than 2147483647 reads selected'
    assert L.view_plan_chunk(2 ** 31 - 12, 70, msg, 600) == OK
    assert L.view_plan_read(0, 10, 10, 1, msg, 600) == OK and L.view_plan_read(10, 0, 10, 0, msg, 600) == OK
    for a in ((-1, 2, 10, 1), (5, 6, 10, 1), (0, -1, 10, 1), (0, 4, 10, 0)):
        assert L.view_plan_read(*a, msg, 600) == E_ARG and msg.value.startswith(b'view: read of [')


def test_growth_rule_and_bounds(L):
    assert [L.view_chunk_records(n) for n in (0, 6, 7, 70)] == [1, 1, 2, 11]
    assert L.view_grow(100, 100) == 100 and L.view_grow(100, 101) == 200 and L.view_grow(100, 500) == 500 and L.view_grow(0, 3) == 3
    cap, grown = 4, 0
    for need in range(1, 5000):                                      # geometric: a handful of growths for a thousandfold need
        new = L.view_grow(cap, need)
        grown += new != cap
        cap = new
    assert cap >= 4999 and grown == 11
    assert [L.view_slabs(n) for n in (0, 1, 8 << 20, (8 << 20) + 1)] == [0, 1, 1, 2]
    assert L.view_slab_len((8 << 20) + 5, 0) == 8 << 20 and L.view_slab_len((8 << 20) + 5, 1) == 5


def test_pass_count(L):
    want = {0: 0, 1: 0, RUN: 0, RUN + 1: 1}
    for k in range(1, 12):
        want[(1 << k) * RUN - 1] = k
        want[(1 << k) * RUN] = k
        want[(1 << k) * RUN + 1] = k + 1
    for n, passes in want.items():
        assert L.view_merge_passes(n) == passes, n
        assert L.view_runs(n) == -(-n // RUN)
    assert L.view_merge_passes(2 ** 31 - 1) == 22


# ---- the command line ----
def test_cli_surface(capsys, tmp_path):
    for name in ('view', 'cview'):
        assert name in wgbs_tools.COMMANDS
        with pytest.raises(SystemExit) as e:
            wgbs_tools.main(['wgbstools', name, '-h'])
        assert e.value.code == 0
        out = capsys.readouterr()
        assert 'not part of this build' not in out.err
        for flag in ('--strict', '--strip', '--min_len', '--no_gaps', '--no_sort', '--sites', '--region', '--genome', '--out_path', '--nanopore',
                     '--device', '--inflate', '--deflate'):
            assert flag in out.out
    assert wgbs_tools.MODULES['cview'] == 'view' and 'cview' not in wgbs_tools.REFERENCE_ONLY
    assert wgbs_tools.main(['wgbstools', 'view']) == 1                 # no input file: the usual refusal, not argparse's exit 2
    assert 'Invalid input argument' in capsys.readouterr().err
    assert wgbs_tools.main(['wgbstools', 'cview', str(tmp_path / 'missing.pat.gz')]) == 1
    assert 'No such file' in capsys.readouterr().err
    args = view.parse_args(['a.pat.gz', '-s', '5-9', '--strict', '--strip', '--min_len', '3', '-np', '--inflate', 'device', '-o', 'x.gz', '--deflate', 'device'])
    assert (args.input_file, args.sites, args.strict, args.strip, args.min_len, args.no_gaps, args.no_sort, args.nanopore, args.inflate,
            args.out_path, args.deflate) == ('a.pat.gz', '5-9', True, True, 3, False, False, True, 'device', 'x.gz', 'device')


def test_cli_refusals(capsys, tmp_path):
    pat = tmp_path / 'x.pat.gz'
    pat.write_bytes(b'')
    bed = tmp_path / 'b.bed'
    bed.write_text('chr1\t1\t2\t5\t9\n')
    for extra, what in ((['--sub_sample', '0.5'], 'view --sub_sample is not part of this build'),
                        (['--shuffle'], 'view --shuffle is not part of this build'),
                        (['-L', str(bed)], 'view -L / --bed_file is not part of this build'),
                        (['--min_len', '0'], '--min_len must be at least 1'),
                        (['--deflate', 'device'], 'give -o a path that ends in .gz'),
                        (['--deflate', 'device', '-o', str(tmp_path / 'o.pat')], 'give -o a path that ends in .gz')):
        for name in ('view', 'cview'):
            assert wgbs_tools.main(['wgbstools', name, str(pat)] + extra) == 1
            assert what in capsys.readouterr().err
    for other, what in (('x.beta', 'wgbstools beta2bed'), ('x.lbeta', 'wgbstools beta2bed'), ('x.pat', 'must end with .pat.gz'), ('x.bin', 'must end with .pat.gz')):
        (tmp_path / other).write_bytes(b'')
        assert wgbs_tools.main(['wgbstools', 'view', str(tmp_path / other)]) == 1
        err = capsys.readouterr().err
        assert what in err and 'not part of this build' in err
    for s, e, what in ((0, 5, 'starts at site 0'), (5, 5, 'is empty'), (9, 5, 'is empty')):
        with pytest.raises(view.IllegalArgumentError, match=what):
            view.check_interval(s, e)


# ---- the shared core under the sanitizers ----
def _have_sanitizers():
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null', '-fsanitize=address,undefined'], input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason='no g++ with sanitizer runtimes')
def test_goldens_through_the_core_under_sanitizers(golden, tmp_path):
    """tests/native/san_view.cpp — the whole of `view` on the host by view_core.h's functions, the arena grown by view_plan.h's rule —
    built plain and with ASan + UBSan: both print every golden's stdout; exit status 0 says that no read or write left its array"""
    texts = {}
    for name in sorted(VC.CASES):
        texts[name] = str(tmp_path / (name + '.pat'))
        with open(texts[name], 'wb') as f:
            f.write(VC.case_pat(VC.CASES[name]))
    for kind, flags in (('plain', []), ('asan_ubsan', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exe = str(tmp_path / ('san_view_' + kind))
        subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-I', CSRC, op.join(HERE, 'native', 'san_view.cpp'), '-o', exe] + flags)
        for name, rec in golden.items():
            kw = VC.flag_kwargs(rec['flags'])
            r = subprocess.run([exe, texts[name], str(rec['sites'][0]), str(rec['sites'][1]), str(flags_of(**kw) | (SORT if rec['sorted'] else 0)),
                                str(kw['min_len'])], capture_output=True, timeout=120, env={'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'})
            assert r.returncode == 0, (kind, name, r.stderr[-3000:])
            assert r.stdout.decode() == rec['stdout'], (kind, name)
            assert r.stderr.startswith(b'records ') and r.stderr.count(b'\n') == 1, (kind, name, r.stderr[-3000:])
