"""`wgbstools mask_pat` without a GPU: the restatement tests/mask_ref.py against every golden the reference's cview, mask_pat, sort and
collapse script wrote (tests/golden/mask_cases.json); csrc/mask_plan.h and view_core.h's mask (through tests/native/mask_host.cpp) against
the restatement — the union, the bitmap, wg_view_hidden, wg_view_hidden64 and the masked cut on every read of the cases and on an
exhaustive sweep — and every refusal of the plan; the command line, the reading of the blocks table and their refusals; the goldens
through a stand-alone program over the same headers (tests/native/san_mask.cpp), built plain and with ASan + UBSan."""
import ctypes as C
import hashlib
import itertools
import json
import os.path as op
import shutil
import subprocess

import numpy as np
import pytest

import mask_cases as KC
import mask_ref as KR
import view_ref as VR
from wgbs_tools_amd import mask_pat, wgbs_tools
from wgbs_tools_amd.genome import IllegalArgumentError

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(HERE)
CSRC = op.join(ROOT, 'wgbs_tools_amd', 'csrc')
SRC = op.join(HERE, 'native', 'mask_host.cpp')
LIB = op.join(HERE, 'native', 'libmask_host.so')
DEPS = [SRC, op.join(ROOT, 'include', 'wgbsseg.h')] + [op.join(CSRC, h) for h in ('mask_plan.h', 'view_core.h', 'bed_fmt.h', 'block_plan.h')]
OK, E_ARG = 0, -1
P, I64, I32, U32, U64 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_uint64
STRICT, STRIP, NO_GAPS, SORT = 1, 2, 4, 8


@pytest.fixture(scope='module')
def L():
    """tests/native/libmask_host.so (built when missing or older than its sources)"""
    if not op.isfile(LIB) or op.getmtime(LIB) < max(op.getmtime(d) for d in DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', SRC, '-o', LIB])
    lib = C.CDLL(LIB)
    lib.mask_plan.restype = C.c_int
    lib.mask_plan.argtypes = [P, P, I64, P, C.POINTER(P), C.c_char_p, C.c_size_t]
    lib.mask_free.argtypes = [P]
    lib.mask_intervals.argtypes = [P, P, P]
    lib.mask_words.argtypes = [P, P]
    lib.mask_hidden.restype = C.c_int
    lib.mask_hidden.argtypes = [P, I64]
    lib.mask_hidden64.restype = U64
    lib.mask_hidden64.argtypes = [P, I64]
    lib.mask_cut.argtypes = [P, I64, C.c_char_p, I64, I64, I64, I32, I64, P, C.c_char_p]
    lib.mask_cut_many.argtypes = [I64, P, P, C.c_char_p, P, I64, C.c_int, I64, I32, I64, I64, P]
    lib.mask_sweep.restype = I64
    lib.mask_sweep.argtypes = [I64, C.c_int, C.c_int, I64, I32, I64, I64, P]
    return lib


@pytest.fixture(scope='module')
def golden():
    with open(op.join(HERE, 'golden', 'mask_cases.json')) as f:
        return json.load(f)


class Mask:
    """a plan of tests/native/mask_host.cpp and the bitmap composed from it"""

    def __init__(self, L, blocks):
        s = np.ascontiguousarray([b[0] for b in blocks], dtype=np.int64)
        e = np.ascontiguousarray([b[1] for b in blocks], dtype=np.int64)
        info = np.full(5, -7, dtype=np.int64)
        msg = C.create_string_buffer(400)
        self.L, self.h = L, P()
        self.rc = L.mask_plan(s.ctypes.data if s.size else None, e.ctypes.data if e.size else None, s.size, info.ctypes.data, C.byref(self.h), msg, 400)
        self.msg = msg.value.decode()
        self.lo, self.hi, self.n_words, self.n_hidden, self.n_intervals = info.tolist()

    def intervals(self):
        s, e = np.zeros(self.n_intervals, dtype=np.int64), np.zeros(self.n_intervals, dtype=np.int64)
        self.L.mask_intervals(self.h, s.ctypes.data, e.ctypes.data)
        return list(zip(s.tolist(), e.tolist()))

    def words(self):
        w = np.zeros(self.n_words, dtype=np.uint32)
        self.L.mask_words(self.h, w.ctypes.data)
        return w.tolist()

    def cut(self, rs, pat, s, e, flags=STRIP, min_len=1):
        out = np.zeros(3, dtype=np.int64)
        masked = C.create_string_buffer(len(pat) + 1)
        self.L.mask_cut(self.h, rs, pat, len(pat), s, e, flags, min_len, out.ctypes.data, masked)
        rs2, first, ln = out.tolist()
        return masked.raw[:len(pat)], ((rs2, masked.raw[first:first + ln]) if ln else None)

    def close(self):
        if self.h:
            self.L.mask_free(self.h)
            self.h = P()


# ---- the restatement against the reference's own output ----
def test_every_case_has_a_golden(golden):
    assert sorted(golden) == sorted(KC.CASES)
    for name, case in KC.CASES.items():
        assert golden[name]['pat_sha1'] == hashlib.sha1(KC.case_pat(case)).hexdigest(), name
        assert golden[name]['table_sha1'] == hashlib.sha1(KC.case_table(case).encode()).hexdigest(), name
        assert golden[name]['where'] == KC.case_where(case), name
        for chrom, rs, pat, count in VR.reads_of(KC.case_pat(case)):       # where this build and the reference agree
            assert count >= 1 and (rs >= 1 and rs + len(pat) - 1 <= 2500 if chrom == b'chr1' else rs > 2500 and rs + len(pat) - 1 <= KC.N_SITES), name


@pytest.mark.parametrize('name', sorted(KC.CASES))
def test_restatement_equals_golden(name, golden):
    rec, case = golden[name], KC.CASES[name]
    assert KR.mask_pat(KC.case_pat(case), KC.case_blocks(case), *rec['sites']).decode() == rec['stdout']
    assert len(KR.Hidden(KC.case_blocks(case))) == rec['loaded']          # the reference's `loaded N sites`
    assert mask_pat.mask_blocks_of(KC.case_table(case))[0].tolist() == [b[0] for b in KC.case_blocks(case)]


def test_goldens_cover_what_the_issue_names(golden):
    assert golden['worked']['stdout'].encode() == KC.WORKED_OUT == golden['worked_header_comments']['stdout'].encode()
    assert sorted(s for s in range(1, 20) if s in KR.Hidden(KC.WORKED_BLOCKS)) == [6, 8, 9, 12]
    out = golden['edges']['stdout']
    assert 'chr1\t292\tCCCC\t2\n' in out and 'chr1\t293\tT\t1\n' in out        # heads that moved over three words of the bitmap
    assert 'chr1\t180\t' + 'T' * 16 + '\t1\n' in out                           # a hidden tail
    assert 'chr1\t170\t' + ('CT' * 13) + '.' * 96 + 'CTCTCTCT' + '.' * 15 + 'TCTCT\t1\n' in out      # hidden interiors: the dots stay
    assert 'chr1\t10\tCTC\t1\n' in out and 'chr1\t2000\tCCC\t2\n' in out       # outside [lo, hi): untouched
    long_line = [ln for ln in golden['long_read']['stdout'].splitlines() if len(ln) > 1000]
    assert len(long_line) == 1 and long_line[0].split('\t')[1] == '301' and long_line[0].split('\t')[2].count('.') == 749
    assert golden['wg_short']['stdout'].count('\n') > 2000 and len(KC.case_pat(KC.CASES['wg_short'])) > 3 * 4096


def test_restatement_refusals():
    good = b'chr1\t4\tCC\t1\nchr1\t9\tT\t2\n'
    for kind, bad in (('bad', b'chr1\t9\tCT\n'), ('desc', b'chr1\t8\tC\t1\n'), ('low', b'chr1\t9\tC\t0\n'), ('low', b'chr1\t9\tC\t-2\n')):
        with pytest.raises(KR.Refused) as e:
            KR.mask_pat(good + bad + b'chr1\t10\tC\t1\n', [(4, 5)], 1, 100)
        assert (e.value.kind, e.value.offset) == (kind, len(good))


# ---- mask_plan.h ----
def test_plan_union_and_bitmap(L):
    for name, case in KC.CASES.items():
        blocks = KC.case_blocks(case)
        m, want = Mask(L, blocks), KR.Hidden(blocks)
        try:
            lo, hi, words = want.words()
            assert (m.rc, m.msg) == (OK, '')
            assert m.intervals() == want.intervals and (m.lo, m.hi, m.n_hidden, m.n_words) == (lo, hi, len(want), len(words)), name
            assert m.words() == words, name
            for site in list(range(max(lo - 70, -5), lo + 70)) + list(range(hi - 70, hi + 70)):
                assert bool(L.mask_hidden(m.h, site)) == (site in want), (name, site)
                got = L.mask_hidden64(m.h, site)
                assert got == sum(1 << i for i in range(64) if site + i in want), (name, site)
        finally:
            m.close()
    m = Mask(L, KC.EDGE_BLOCKS)
    try:
        assert (m.lo, m.hi, m.n_words) == (KC.EDGE_LO, KC.EDGE_HI, 10)
        w = m.words()
        assert w[0] == 0x80000001 and w[1] == 0x80000001 and w[2] == 1 and w[3:6] == [0xffffffff] * 3 and w[9] == 1 << 12
        assert m.intervals()[:6] == [(100, 101), (131, 133), (163, 165), (196, 292), (300, 315), (320, 321)]
    finally:
        m.close()
    one = Mask(L, [(7, 8)])
    assert (one.lo, one.hi, one.n_words, one.n_hidden, one.words()) == (7, 8, 1, 1, [1])
    one.close()
    top = Mask(L, [(2 ** 31 - 2, 2 ** 31 - 1)])
    assert top.rc == OK and bool(L.mask_hidden(top.h, 2 ** 31 - 2)) and not L.mask_hidden(top.h, 2 ** 31 - 1) and L.mask_hidden64(top.h, 2 ** 31 - 65) == 1 << 63
    top.close()


def test_plan_refusals(L):
    for blocks, what in (([], 'mask: no blocks (at least 1)'),
                         ([(5, 9), (0, 4)], 'mask: block 1 starts at site 0 (sites count from 1)'),
                         ([(5, 9), (8, 12), (-3, 4)], 'mask: block 2 starts at site -3 (sites count from 1)'),
                         ([(5, 5)], 'mask: block 0 = sites [5, 5) is empty'),
                         ([(5, 9), (9, 4)], 'mask: block 1 = sites [9, 4) is empty'),
                         ([(5, 2 ** 31)], 'mask: block 0 ends at site 2147483648 (at most 2147483647)')):
        m = Mask(L, blocks)
        assert (m.rc, m.msg) == (E_ARG, what) and not m.h
    ok = Mask(L, [(5, 2 ** 31 - 1)])
    assert ok.rc == OK and ok.n_hidden == 2 ** 31 - 6 and ok.n_words == (2 ** 31 - 6 + 31) // 32
    ok.close()


# ---- the masked cut ----
def test_masked_cut_on_every_read_of_the_cases(L, golden):
    for name, case in KC.CASES.items():
        blocks, (s, e) = KC.case_blocks(case), golden[name]['sites']
        m, hidden = Mask(L, blocks), KR.Hidden(blocks)
        try:
            for chrom, rs, pat, count in VR.reads_of(KC.case_pat(case)):
                masked, got = m.cut(rs, pat, s, e)
                assert masked == KR.mask_pattern(rs, pat, hidden), (name, rs, pat)
                assert got == KR.cut(rs, pat, hidden, s, e), (name, rs, pat)
        finally:
            m.close()
    m, hidden = Mask(L, KC.WORKED_BLOCKS), KR.Hidden(KC.WORKED_BLOCKS)     # the other flags: the mask between --strict and the strip
    try:
        for flags, kw in ((0, dict(strip=False)), (STRICT, dict(strict=True, strip=False)), (STRICT | STRIP, dict(strict=True)),
                          (STRIP | NO_GAPS, dict(no_gaps=True)), (STRICT | STRIP | NO_GAPS, dict(strict=True, no_gaps=True))):
            for rs, pat, _ in KC.WORKED_READS + [(3, b'CCCCCCCCCCCC', 1), (7, b'TCT', 1)]:
                for s, e, min_len in ((1, 100, 1), (7, 11, 1), (7, 11, 2), (9, 10, 1)):
                    assert m.cut(rs, pat, s, e, flags, min_len)[1] == KR.cut(rs, pat, hidden, s, e, min_len=min_len, **kw), (flags, rs, pat, s, e, min_len)
    finally:
        m.close()


FIRST, WINDOW, MAX_LEN = 60, 12, 6


@pytest.mark.parametrize('lo', [FIRST, FIRST - 40, FIRST + 5])
def test_exhaustive_sweep(L, lo):
    """all patterns over {C, T, .} of length <= 6 at every start of a 12-site window against every subset of its sites: natively the
    masked cut (64 sites at a time) against the cut of the read masked byte by byte; here every pattern, start and subset of the READ'S OWN
    sites — what its cut depends on — against tests/mask_ref.py.  lo: the bitmap begins at the window, 40 sites (a word and a bit) in
    front of it, or inside it (then the sites in front of lo cannot be hidden)."""
    n_reads = I64(0)
    assert L.mask_sweep(FIRST, WINDOW, MAX_LEN, lo, STRIP, 1, 1000, C.byref(n_reads)) == 0
    assert n_reads.value == (1 << WINDOW) * sum(3 ** k for k in range(1, MAX_LEN + 1)) * WINDOW
    rs, off, pats, subsets, want = [], [0], [], [], []
    for ln in range(1, MAX_LEN + 1):
        for pat in itertools.product(b'CT.', repeat=ln):
            pat = bytes(pat)
            for r in range(FIRST, FIRST + WINDOW):
                own = [k for k in range(r - FIRST, min(r - FIRST + ln, WINDOW))]
                for bits in range(1 << len(own)):
                    sub = sum(1 << own[i] for i in range(len(own)) if bits >> i & 1)
                    hidden = {FIRST + k for k in own if sub >> k & 1 and FIRST + k >= lo}
                    rs.append(r); pats.append(pat); off.append(off[-1] + ln); subsets.append(sub)
                    want.append(KR.cut(r, pat, hidden, 1, 1000))
    n = len(rs)
    out = np.zeros((n, 3), dtype=np.int64)
    rs_a, off_a, sub_a = np.array(rs, dtype=np.int64), np.array(off, dtype=np.int64), np.array(subsets, dtype=np.uint32)
    L.mask_cut_many(n, rs_a.ctypes.data, off_a.ctypes.data, b''.join(pats), sub_a.ctypes.data, FIRST, WINDOW, lo, STRIP, 1, 1000, out.ctypes.data)
    for i in range(n):
        r2, first, ln = out[i].tolist()
        hidden = {FIRST + k for k in range(WINDOW) if subsets[i] >> k & 1 and FIRST + k >= lo}
        got = (r2, KR.mask_pattern(rs[i], pats[i], hidden)[first:first + ln]) if ln else None
        assert got == want[i], (rs[i], pats[i], subsets[i])


# ---- the command line ----
FLAGS = ('--prefix', '--sites_to_hide', '--sites', '--region', '--genome', '--beta', '--lbeta', '--force', '--threads', '--device', '--inflate', '--bed_file')


def test_cli_surface(capsys):
    assert 'mask_pat' in wgbs_tools.COMMANDS and 'mask_pat' not in wgbs_tools.REFERENCE_ONLY and 'mix_pat' in wgbs_tools.REFERENCE_ONLY
    with pytest.raises(SystemExit) as e:
        wgbs_tools.main(['wgbstools', 'mask_pat', '-h'])
    assert e.value.code == 0
    out = capsys.readouterr()
    assert 'not part of this build' not in out.err and 'not part of this build' not in out.out
    for flag in FLAGS:
        assert flag in out.out, flag
    args = mask_pat.parse_args(['a.pat.gz', '-p', 'out', '-b', 'snp.bed', '-s', '5-9', '--lbeta', '-f', '-@', '3', '--inflate', 'device', '--device', '1'])
    assert (args.pat_path, args.prefix, args.sites_to_hide, args.sites, args.beta, args.lbeta, args.force, args.threads, args.inflate,
            args.device) == ('a.pat.gz', 'out', 'snp.bed', '5-9', False, True, True, 3, 'device', 1)
    for argv in (['a.pat.gz', '-b', 'snp.bed'], ['a.pat.gz', '-p', 'out'], ['a.pat.gz', '-p', 'o', '-b', 'b', '--beta', '--lbeta']):
        with pytest.raises(SystemExit):                                # -p and -b are required; --beta and --lbeta exclude each other
            mask_pat.parse_args(argv)
    capsys.readouterr()
    for word in ('-L / --bed_file', '.csi', 'row number', 'fifth column', 'C locale', 'count below 1'):     # the deviations are stated
        assert word in mask_pat.__doc__, word


def test_blocks_table():
    text = KC.table_text(KC.WORKED_BLOCKS, header=True, comments=True)
    s, e = mask_pat.mask_blocks_of(text)
    assert list(zip(s.tolist(), e.tolist())) == KC.WORKED_BLOCKS
    assert mask_pat.mask_blocks_of('chr1\t1\t2\t +5x\t9.7\n')[0].tolist() == [5]                  # std::stoi's reading
    for bad, what in (('chr1\t1\t2\tNA\tNA\n', 'row 1: startCpG / endCpG "NA" / "NA" is not a number'),
                      ('chr1\t1\t2\t5\t9\n\nchr1\t1\t2\t9\t9\n', 'row 3: endCpG <= startCpG (9, 9)'),
                      ('#c\nchr1\t1\t2\t0\t9\n', 'row 2: startCpG < 1 (0)'),
                      ('chr1\t1\t2\t5\t9\nchr1\t1\t2\t5\n', 'row 2 has 4 columns'),
                      ('chr1\t1\t2\t5\t%d\n' % 2 ** 31, 'row 1: endCpG 2147483648 (at most 2147483647)'),
                      ('chr\tstart\tend\tstartCpG\tendCpG\n# nothing\n\n', 'no usable row'),
                      ('', 'no usable row'),
                      ('chr1\t1\t2\t5\t9\nchr\tstart\tend\tstartCpG\tendCpG\n', 'row 2: startCpG / endCpG "startCpG" / "endCpG" is not a number')):
        with pytest.raises(IllegalArgumentError) as err:
            mask_pat.mask_blocks_of(bad, 'snp.bed')
        assert 'mask_pat: snp.bed: ' + what in str(err.value), bad


def test_cli_refusals(capsys, tmp_path):
    pat = str(tmp_path / 'a.pat.gz')
    open(pat, 'wb').close()
    bed = tmp_path / 'b.bed'
    bed.write_text('chr1\t1\t2\t5\t9\n')
    na = tmp_path / 'na.bed'
    na.write_text('chr1\t1\t2\t5\t9\nchr1\t1\t2\tNA\tNA\n')
    pre = str(tmp_path / 'out')
    (tmp_path / 'x.pat').write_bytes(b'')
    for argv, what in (([pat, '-p', pre, '-b', str(bed), '-L', str(bed)], 'mask_pat -L / --bed_file is not part of this build'),
                       ([str(tmp_path / 'missing.pat.gz'), '-p', pre, '-b', str(bed)], 'No such file'),
                       ([pat, '-p', pre, '-b', str(tmp_path / 'missing.bed')], 'No such file'),
                       ([str(tmp_path / 'x.pat'), '-p', pre, '-b', str(bed)], 'must end with .pat.gz'),
                       ([pat, '-p', str(tmp_path / 'a'), '-b', str(bed)], 'the output path is identical to the input file'),
                       ([pat, '-p', pre, '-b', str(na)], 'row 2: startCpG / endCpG "NA" / "NA" is not a number')):
        assert wgbs_tools.main(['wgbstools', 'mask_pat'] + argv) == 1, argv
        err = capsys.readouterr().err
        assert 'Invalid input argument' in err and what in err, (argv, err)
    assert not op.exists(pre + '.pat.gz')
    # an existing output without -f: skipped with the reference's line, nothing touched (and no device asked for)
    with open(pre + '.pat.gz', 'wb') as f:
        f.write(b'kept')
    assert wgbs_tools.main(['wgbstools', 'mask_pat', pat, '-p', pre, '-b', str(bed)]) == 0
    assert f'File {pre}.pat.gz already exists. Skipping it. Use [-f] flag to force overwrite.' in capsys.readouterr().err
    with open(pre + '.pat.gz', 'rb') as f:
        assert f.read() == b'kept'


# ---- the shared headers under the sanitizers ----
def _have_sanitizers():
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null', '-fsanitize=address,undefined'], input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason='no g++ with sanitizer runtimes')
def test_goldens_through_the_headers_under_sanitizers(golden, tmp_path):
    """tests/native/san_mask.cpp — the whole of `mask_pat` on the host by the functions the kernels call, the bitmap in an array of
    exactly its size — built plain and with ASan + UBSan: both print every golden's stdout; exit status 0 says that no read or write
    left its array"""
    for kind, flags in (('plain', []), ('asan_ubsan', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exe = str(tmp_path / ('san_mask_' + kind))
        subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-I', CSRC, op.join(HERE, 'native', 'san_mask.cpp'), '-o', exe] + flags)
        for name, rec in golden.items():
            case = KC.CASES[name]
            pat, blocks = str(tmp_path / (name + '.pat')), str(tmp_path / (name + '.blocks'))
            with open(pat, 'wb') as f:
                f.write(KC.case_pat(case))
            with open(blocks, 'w') as f:
                f.write(''.join('%d %d\n' % b for b in KC.case_blocks(case)))
            r = subprocess.run([exe, pat, blocks, str(rec['sites'][0]), str(rec['sites'][1]), str(STRIP | SORT)], capture_output=True, timeout=120,
                               env={'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'})
            assert r.returncode == 0, (kind, name, r.stderr[-3000:])
            assert r.stdout.decode() == rec['stdout'], (kind, name)
            assert r.stderr.startswith(b'loaded %d sites ' % rec['loaded']) and r.stderr.count(b'\n') == 1, (kind, name, r.stderr[-3000:])
