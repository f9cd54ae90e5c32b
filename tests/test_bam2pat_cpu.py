"""`wgbstools bam2pat` without a GPU: the restatement tests/bam2pat_ref.py against every golden the reference's own `patter` and
`sort | uniq -c` wrote (tests/golden/bam2pat_cases.json); csrc/sam_plan.h and sam_core.h (through tests/native/sam_host.cpp) — every
refusal of the plan with its message, the field split, the numbers, the filter, the CIGAR check and its cursor, a line's pat, the mate
rule, the merge, and whole files through the functions the kernels call — against the restatement; the command line: help, every
refusal with its message, output names, the skip without -f; and the goldens through a stand-alone program over the same headers
(tests/native/san_bam2pat.cpp), built plain and with ASan + UBSan."""
import ctypes as C
import gzip
import hashlib
import io
import json
import os.path as op
import shutil
import subprocess

import numpy as np
import pytest

import bam2pat_cases as SC
import bam2pat_ref as BR
import frag_cases as FC
from wgbs_tools_amd import bam2pat, wgbs_tools

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(HERE)
CSRC = op.join(ROOT, 'wgbs_tools_amd', 'csrc')
SRC = op.join(HERE, 'native', 'sam_host.cpp')
LIB = op.join(HERE, 'native', 'libsam_host.so')
DEPS = [SRC, op.join(HERE, 'native', 'sam_run.h'), op.join(ROOT, 'include', 'wgbsseg.h')] + [
    op.join(CSRC, h) for h in ('sam_plan.h', 'sam_core.h', 'bed2beta_plan.h', 'bed2beta_core.h', 'view_plan.h', 'view_core.h', 'merge_plan.h', 'bed_fmt.h', 'block_plan.h')]
OK, E_ARG, E_CAPACITY, E_STATE = 0, -1, -6, -7
P, I64, I32, U32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32
LOCI = SC.LOCI.astype(np.uint32)
CHROMS = SC.CHROMS
ARG_ORDER = ('paired', 'exclude', 'include', 'mapq', 'strand', 'clip', 'min_cpg')


@pytest.fixture(scope='module')
def L():
    """tests/native/libsam_host.so (built when missing or older than its sources)"""
    if not op.isfile(LIB) or op.getmtime(LIB) < max(op.getmtime(d) for d in DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-ffp-contract=off', '-shared', '-fPIC', SRC, '-o', LIB])
    lib = C.CDLL(LIB)
    lib.sam_plan.restype = C.c_int
    lib.sam_plan.argtypes = [P, I64, C.POINTER(C.c_char_p), P, P, I32, I32, I64, I64, I32, I32, I32, I32, C.POINTER(P), C.c_char_p, C.c_size_t]
    lib.sam_free.argtypes = [P]
    lib.sam_state.restype = C.c_int
    lib.sam_state.argtypes = [C.c_int] * 6 + [C.c_char_p, C.c_size_t]
    lib.sam_lines.restype = C.c_int
    lib.sam_lines.argtypes = [I64, I64, P, C.c_char_p, C.c_size_t]
    lib.sam_records.restype = C.c_int
    lib.sam_records.argtypes = [I64, I64, C.c_char_p, C.c_size_t]
    lib.sam_split.restype = C.c_int
    lib.sam_split.argtypes = [C.c_char_p, I64, I64, P]
    lib.sam_number.restype = I64
    lib.sam_number.argtypes = [C.c_char_p, I64, I64]
    lib.sam_keep.restype = C.c_int
    lib.sam_keep.argtypes = [U32, I64, P]
    lib.sam_is_bottom.restype = C.c_int
    lib.sam_is_bottom.argtypes = [U32, C.c_int]
    lib.sam_cigar.restype = I64
    lib.sam_cigar.argtypes = [C.c_char_p, I64, C.c_char_p, I64, C.c_char_p]
    lib.sam_eval.argtypes = [P, P, C.c_char_p, I64, I64, P, C.c_char_p, I64]
    lib.sam_merge.argtypes = [I64, C.c_char_p, I64, I64, C.c_char_p, I64, P, C.c_char_p]
    lib.sam_same_read.restype = C.c_int
    lib.sam_same_read.argtypes = [C.c_char_p, U32, I32, C.c_char_p, U32, I32]
    lib.sam_sizes.argtypes = [P]
    lib.sam_run.restype = I64
    lib.sam_run.argtypes = [P, P, C.c_char_p, I64, C.c_char_p, I64, P]
    return lib


@pytest.fixture(scope='module')
def golden():
    with open(op.join(HERE, 'golden', 'bam2pat_cases.json')) as f:
        return json.load(f)


class Plan:
    """a plan of tests/native/sam_host.cpp over the tiny genome (or one given)"""

    def __init__(self, L, loci=LOCI, chroms=CHROMS, **a):
        a = dict(SC.DEFAULTS, **a)
        self.loci = np.ascontiguousarray(loci, dtype=np.uint32)
        sizes = np.array([s for _, s in chroms], dtype=np.int64)
        hi = np.cumsum(sizes)
        lo = np.ascontiguousarray(hi - sizes)
        raw = [c.encode() for c, _ in chroms]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        msg = C.create_string_buffer(600)
        self.L, self.h = L, P()
        self.rc = L.sam_plan(self.loci.ctypes.data, self.loci.size, arr, lo.ctypes.data if lo.size else None, hi.ctypes.data if hi.size else None, len(raw),
                             *[int(a[k]) for k in ARG_ORDER], C.byref(self.h), msg, 600)
        self.msg = msg.value.decode()

    def eval(self, text, p=0):
        out = np.zeros(6, dtype=np.int64)
        pat = C.create_string_buffer(4096)
        self.L.sam_eval(self.h, self.loci.ctypes.data, text, len(text), p, out.ctypes.data, pat, 4096)
        state, chrom, qlen, start, plen, bottom = out.tolist()
        return state, chrom, qlen, start, pat.raw[:plen] if state == BR.PAT else b'', bottom

    def run(self, text):
        out = C.create_string_buffer(len(text) + 64)
        stats = np.zeros(len(BR.COUNTERS), dtype=np.int64)
        n = self.L.sam_run(self.h, self.loci.ctypes.data, text, len(text), out, len(text) + 64, stats.ctypes.data)
        assert n >= 0
        return out.raw[:n], dict(zip(BR.COUNTERS, stats.tolist()))

    def close(self):
        if self.h:
            self.L.sam_free(self.h)
            self.h = P()


def ref(text, a):
    return BR.bam2pat(text, SC.LOCI, CHROMS, **a)


# ---- the restatement against the reference's own output ----
def test_every_case_has_a_golden(golden):
    assert sorted(golden) == sorted(SC.CASES)
    for name, case in SC.CASES.items():
        assert golden[name]['text_sha1'] == hashlib.sha1(SC.case_text(case)).hexdigest(), name
        assert golden[name]['args'] == SC.case_args(case), name


@pytest.mark.parametrize('name', sorted(SC.CASES))
def test_restatement_equals_golden(name, golden):
    case = SC.CASES[name]
    got, n = ref(SC.case_text(case), SC.case_args(case))
    assert got.decode() == golden[name]['stdout'], name
    assert n['lines'] == sum(1 for ln in SC.case_text(case).split(b'\n') if ln), name


def test_goldens_cover_what_the_issue_names(golden):
    out = {k: [ln.split('\t') for ln in v['stdout'].splitlines()] for k, v in golden.items()}
    n = {k: ref(SC.case_text(c), SC.case_args(c))[1] for k, c in SC.CASES.items()}
    assert any(int(row[3]) == 3 for row in out['se_both_strands']) and n['se_both_strands']['header'] == 4 and n['se_both_strands']['filtered'] == 3
    assert len(out['se_top_only']) + len(out['se_bottom_only']) == len(out['se_both_strands'])
    assert n['pe_four_flags']['pairs'] == 6 and n['pe_four_flags']['filtered'] == 2 and n['pe_no_include']['pairs'] == 7
    assert len(out['pe_top_only']) == len(out['pe_bottom_only']) == 3
    assert n['cigar_ops']['invalid'] == 6 and len(out['cigar_ops']) == 4 and any('.' in row[2] for row in out['cigar_ops'])      # D and N leave dots
    assert out['clip_0'] != out['clip_1'] != out['clip_3'] and out['clip_read_len'] == out['clip_more'] == [] and n['clip_more']['empty'] == 6
    assert n['past_last_cpg']['empty'] == 4 and {row[1] for row in out['past_last_cpg']} == {str(SC.N1 - 1), str(SC.N_SITES - 1)}
    assert n['unknown_rname']['unknown_chrom'] == 3 and n['unknown_rname']['pairs'] == 1
    assert n['min_cpg_3']['short'] == 2 and all(len(row[2]) >= 3 for row in out['min_cpg_3'] + out['min_cpg_3_pe']) and n['min_cpg_3_pe']['short'] == 2
    assert n['mates']['pairs'] == 8 and n['mates']['left_single'] == 1 and any('.' in row[2] for row in out['mates'])
    assert out['span_300'] == [['chr2', str(SC.N1 + 401), 'C' + '.' * 298 + 'T', '2']] and out['span_301'] == [] and n['span_301']['too_long'] == 2
    assert n['runs']['pairs'] == 6 and n['runs']['left_single'] == 3                      # 3, 4, 5, 2, 1 equal names: 1 + 2 + 2 + 1 + 0 pairs
    assert n['invalid_between_mates']['pairs'] == 1 and n['invalid_between_mates']['left_single'] == 4 and len(out['invalid_between_mates']) == 2
    assert n['filtered_between_mates']['pairs'] == 1 and n['filtered_between_mates']['filtered'] == 3 and len(out['filtered_between_mates']) == 1
    assert n['too_short_line']['invalid'] == 3 and n['header_only_and_blank']['header'] == 4
    for name, case in SC.CASES.items():
        text, a = SC.case_text(case), SC.case_args(case)
        alive = [BR.tokens_of(ln) for ln in text.split(b'\n') if ln and not ln.startswith(b'@')]
        assert not SC.names_split_by_other_chromosomes([(t[0], t[2]) for t in alive if len(t) >= 3 and t[2] in (b'chr1', b'chr2')]), name


# ---- sam_plan.h ----
def test_plan_refusals_and_sizes(L):
    for a, what in ((dict(exclude=-1), 'patview_set_sam: flags -1 / 0 (0 .. 65535)'), (dict(include=65536), 'patview_set_sam: flags 1796 / 65536 (0 .. 65535)'),
                    (dict(mapq=256), 'patview_set_sam: mapq 256 (0 .. 255)'), (dict(strand=3), 'patview_set_sam: strand 3 (0 both, 1 top, 2 bottom)'),
                    (dict(clip=-1), 'patview_set_sam: clip -1 (at least 0)'), (dict(min_cpg=-2), 'patview_set_sam: min_cpg -2 (at least 0)'),
                    (dict(paired=2), 'patview_set_sam: paired 2 (0 or 1)')):
        p = Plan(L, **a)
        assert (p.rc, p.msg) == (E_ARG, what) and not p.h, a
    p = Plan(L, chroms=[('a', 2500), ('a', 1500)])
    assert (p.rc, p.msg) == (E_ARG, 'bedbeta: chromosomes 0 and 1 have the same name (a)')      # the table's checks are bed2beta_plan.h's
    msg = C.create_string_buffer(400)
    for args, rc, what in (((0, 0, 0, 0, 0, 8), OK, ''), ((1, 0, 0, 0, 0, 8), E_STATE, 'patview_set_sam: called twice'),
                           ((0, 1, 0, 0, 0, 8), E_STATE, 'patview_set_sam: called after the first feed'), ((0, 0, 1, 0, 0, 8), E_STATE, 'patview_set_sam: called after the first feed'),
                           ((0, 0, 0, 1, 0, 8), E_STATE, 'patview_set_sam: the engine has a mask: SAM text does not go with it'),
                           ((0, 0, 0, 0, 1, 8), E_STATE, 'patview_set_sam: the engine has labels: SAM text does not go with it'),
                           ((0, 0, 0, 0, 0, 0), E_ARG, 'patview_set_sam: the engine must be created with WGBSSEG_VIEW_SORT and no other flag (got 0)'),
                           ((0, 0, 0, 0, 0, 10), E_ARG, 'patview_set_sam: the engine must be created with WGBSSEG_VIEW_SORT and no other flag (got 10)')):
        msg.value = b''
        assert (L.sam_state(*args, msg, 400), msg.value.decode()) == (rc, what), args
    out = np.zeros(3, dtype=np.int64)
    assert L.sam_lines(1000, 0, out.ctypes.data, msg, 400) == OK and out.tolist() == [0, 0, 8]
    assert L.sam_lines(10 ** 6, 257, out.ctypes.data, msg, 400) == OK and out.tolist() == [257, 2, 24]
    assert L.sam_lines(2 ** 31, 5, out.ctypes.data, msg, 400) == E_ARG and msg.value == b'view: a chunk of 2147483648 bytes (at most 2147483647)'
    assert L.sam_lines(10, 11, out.ctypes.data, msg, 400) == E_ARG and msg.value == b'view: 11 lines in a chunk of 10 bytes'
    assert L.sam_records(2 ** 31 - 10, 9, msg, 400) == OK and L.sam_records(2 ** 31 - 10, 10, msg, 400) == E_CAPACITY
    assert msg.value == b'view: more than 2147483647 reads selected'
    sizes = np.zeros(4, dtype=np.int64)
    L.sam_sizes(sizes.ctypes.data)
    assert sizes.tolist() == [24, 288, len(BR.COUNTERS), 256]


# ---- sam_core.h, function by function ----
def test_field_split_and_numbers(L):
    b = np.zeros(20, dtype=np.uint32)
    for line in (b'a\tb\tc', b'a\tb\tc\t', b'a\t\tc\t\t', b'\t', b'x', b'\t'.join([b'f%d' % k for k in range(10)]), b'\t'.join([b'f%d' % k for k in range(10)]) + b'\t',
                 b'\t'.join([b'f%d' % k for k in range(11)]), b'\t'.join([b'f%d' % k for k in range(10)]) + b'\t\t', b'\t'.join([b'f%d' % k for k in range(15)]),
                 b'q\t0\tchr1\t5\t9\t3M\t=\t5\t0\t\tF'):
        tok = BR.tokens_of(line)
        text = b'zz\n' + line + b'\nnext\tline\n'
        nf = L.sam_split(text, len(text), 3, b.ctypes.data)
        assert nf == min(len(tok), 11), line
        for k in range(min(nf, 10)):
            assert text[3 + b[2 * k]:3 + b[2 * k + 1]] == tok[k], (line, k)
    for field, most, want in ((b'0', 9, 0), (b'99', 2 ** 31 - 1, 99), (b'0099', 2 ** 31 - 1, 99), (b'2147483647', 2 ** 31 - 1, 2 ** 31 - 1), (b'2147483648', 2 ** 31 - 1, -1),
                              (b'4294967295', 2 ** 32 - 1, 2 ** 32 - 1), (b'99999999999999999999999', 2 ** 32 - 1, -1), (b'', 9, -1), (b'+5', 9, -1), (b'-5', 9, -1),
                              (b' 5', 9, -1), (b'5x', 9, -1), (b'x', 9, -1), (b'1e3', 9999, -1)):
        assert L.sam_number(field, len(field), most) == want, field
        assert (BR.number(field, most) if BR.number(field, most) is not None else -1) == want, field


def test_filter_and_strand(L):
    for a in (dict(), dict(paired=True, include=3), dict(strand=1), dict(strand=2), dict(paired=True, strand=1), dict(paired=True, strand=2),
              dict(exclude=0, mapq=0), dict(include=16, mapq=255)):
        a = dict(SC.DEFAULTS, **a)
        p = Plan(L, **a)
        try:
            for flag in list(range(0, 260)) + [1024, 1123, 1796, 2048, 2147, 65535]:
                for mapq in (0, 9, 10, 254, 255):
                    assert bool(L.sam_keep(flag, mapq, p.h)) == BR.keep(flag, mapq, a['paired'], a['exclude'], a['include'], a['mapq'], a['strand']), (a, flag, mapq)
        finally:
            p.close()
    for flag in range(0, 4096):
        for paired in (0, 1):
            assert bool(L.sam_is_bottom(flag, paired)) == BR.is_bottom(flag, bool(paired)), (flag, paired)


def test_cigar_check_and_cursor(L):
    seq = b'ACGTACGTACGTACGTACGTAAAA'
    rng = np.random.default_rng(20261021)
    cigars = [b'24M', b'4S20M', b'10M2I12M', b'10M3D14M', b'10M300N14M', b'2H24M3H', b'12=12X', b'5M', b'', b'24M7', b'007M', b'0M', b'*', b'M', b'5M*', b'25M', b'24M1S',
              b'24M1I', b'10M2P14M', b'5m', b'2147483647D', b'2147483648D', b'99999999999999999999M', b'3D', b'1M1I1M1D1M1N1M1S1H', b'4S', b'25S', b'10M-2D']
    for _ in range(200):
        cigars.append(b''.join(b'%d%s' % (int(rng.integers(0, 9)), bytes([rng.choice(list(b'MIDNSH=XMMM'))])) for _ in range(int(rng.integers(1, 8)))))
    adj = C.create_string_buffer(1 << 16)
    for cg in cigars:
        want = BR.clean_cigar(seq, cg) if not cg.startswith(b'2147483647') else None
        big = cg.startswith(b'2147483647')
        got = L.sam_cigar(cg, len(cg), seq, len(seq), None if big else adj)
        if big:
            assert got == 2 ** 31 - 1                               # (the restatement would really make the Ns)
            continue
        assert got == (len(want) if want is not None else -1), cg
        if want is not None:
            assert adj.raw[:got + 2] == want + b'\0\0', cg


def test_lines_and_their_pats(L):
    for a in (dict(), dict(clip=2), dict(paired=True, include=3), dict(paired=True, include=3, clip=1)):
        a = dict(SC.DEFAULTS, **a)
        p = Plan(L, **a)
        table, at = {}, 0
        for name, size in CHROMS:
            table[name.encode()] = ([int(x) for x in SC.LOCI[at:at + size]], at + 1)
            at += size
        try:
            for name, case in SC.CASES.items():
                text = SC.case_text(case) + b'r\t0\tchr1\t1\t40\t1M\t=\t1\t0\t' + b'Q' * 300 + b'\tF\n' + b'N' * 255 + b'\t0\tchr1\t1\t40\t1M\t=\t1\t0\tA\tF\n'
                pos = 0
                for line in text.split(b'\n'):
                    if line:
                        state, key, chrom, start, pat = BR.classify(line, a['paired'], table, a['exclude'], a['include'], a['mapq'], a['strand'], a['clip'])
                        got = p.eval(text, pos)
                        assert (got[0], got[3] if state == BR.PAT else 0, got[4]) == (state, start, pat), (name, line[:60])
                        if state >= BR.INVALID:
                            assert got[1] == [c for c, _ in CHROMS].index(chrom.decode()) and got[2] == min(len(BR.tokens_of(line)[0]), 255)
                    pos += len(line) + 1
        finally:
            p.close()


def test_mate_rule_and_merge(L):
    same = lambda a, ra, b, rb: bool(L.sam_same_read(a, len(a), ra, b, len(b), rb))
    assert same(b'read1', 0, b'read1', 0) and not same(b'read1', 0, b'read1', 1) and not same(b'read1', 0, b'read2', 0) and not same(b'read1', 0, b'read10', 0)
    assert same(b'', 1, b'', 1) and same(b'q' * 254, 0, b'q' * 254, 0)
    assert L.sam_same_read(b'q' * 255, 255, 0, b'q' * 255, 255, 0) == 0                      # a name above 254 bytes pairs with nothing
    rng = np.random.default_rng(3)
    out = np.zeros(4, dtype=np.int64)
    span = C.create_string_buffer(400)
    cases = [((5, b'CT'), (5, b'CT')), ((5, b'C'), (5, b'T')), ((5, b'CT'), (7, b'TC')), ((9, b'C'), (5, b'T')), ((5, b'C'), (304, b'T')), ((5, b'C'), (305, b'T')),
             ((5, b'C' * 300), (5, b'C')), ((5, b'C' * 301), (5, b'C')), ((5, b'CTC'), (6, b'C')), ((5, b'C.T'), (5, b'T.C')), ((1, b'C.T'), (2, b'T'))]
    for _ in range(300):
        one = lambda: (int(rng.integers(1, 400)), b'C' + bytes(rng.choice(list(b'CT.'), int(rng.integers(0, 12))).tolist()) + b'T')
        cases.append((one(), one()))
    for a, b in cases:
        want = BR.merge(a, b)
        L.sam_merge(a[0], a[1], len(a[1]), b[0], b[1], len(b[1]), out.ctypes.data, span)
        why, rs, first, ln = out.tolist()
        if want == 'long':
            assert why == 1, (a, b)
        elif want == 'empty':
            assert why == 2, (a, b)
        else:
            assert why == 0 and (rs, span.raw[first:first + ln]) == want, (a, b)


def test_whole_files_on_the_host(L, golden):
    for name, case in SC.CASES.items():
        text, a = SC.case_text(case), SC.case_args(case)
        p = Plan(L, **a)
        try:
            got, st = p.run(text)
            assert got.decode() == golden[name]['stdout'] and st == ref(text, a)[1], name
            assert p.run(text.rstrip(b'\n'))[0] == got, name                 # a last line without its newline
        finally:
            p.close()
    rng = np.random.default_rng(20261021)
    for k in range(12):
        text, a = SC.random_world(rng, 300)
        p = Plan(L, **a)
        try:
            assert p.run(text) == ref(text, a), k
        finally:
            p.close()


# ---- the command line ----
FLAGS = ('--out_dir', '--force', '--genome', '--min_cpg', '--clip', '--mapq', '--exclude_flags', '--include_flags', '--top_strand', '--bottom_strand', '--no_beta',
         '--lbeta', '--device', '--inflate', '--name', '--temp_dir', '--threads')


def test_cli_surface(capsys):
    assert 'bam2pat' in wgbs_tools.COMMANDS and 'bam2pat' in wgbs_tools.REFERENCE_ONLY
    with pytest.raises(SystemExit) as e:
        wgbs_tools.main(['wgbstools', 'bam2pat', '-h'])
    assert e.value.code == 0
    out = capsys.readouterr()
    assert 'not part of this build' in out.out and 'Generate pat & beta files out of SAM text' in out.out and out.err == ''
    for flag in FLAGS:
        assert flag in out.out, flag
    args = bam2pat.parse_args(['a.sam', 'b.sam.gz', '-o', 'out', '-f', '--genome', 'hg19', '--min_cpg', '3', '--clip', '5', '-q', '20', '-F', '1024', '--include_flags', '2',
                               '--top_strand', '--no_beta', '-l', '--device', '1', '--inflate', 'device', '-T', '/tmp', '-@', '8'])
    assert (args.sam, args.out_dir, args.force, args.genome, args.min_cpg, args.clip, args.mapq, args.exclude_flags, args.include_flags, args.top_strand, args.bottom_strand,
            args.no_beta, args.lbeta, args.device, args.inflate) == (['a.sam', 'b.sam.gz'], 'out', True, 'hg19', 3, 5, 20, 1024, 2, True, False, True, True, 1, 'device')
    d = bam2pat.parse_args(['x.sam'])
    assert (d.min_cpg, d.clip, d.mapq, d.exclude_flags, d.include_flags) == (1, 0, 10, 1796, None)
    with pytest.raises(SystemExit):
        bam2pat.parse_args(['x.sam', '--top_strand', '--bottom_strand'])
    capsys.readouterr()
    for word in ('samtools view', 'MATES ARE ADJACENT', 'samtools collate -O', 'samtools sort -n', '.csi', 'one RNAME', 'streams every', 'match_maker', '254'):
        assert word in bam2pat.__doc__, word
    assert [bam2pat.pretty_name(p) for p in ('/x/y/a.sam', 'b.sam.gz', 's.sorted.sam', 'c.bam')] == ['a', 'b', 's.sorted', 'c']


def test_head_peek():
    pe, se = SC.case_text(SC.CASES['pe_four_flags']), SC.case_text(SC.CASES['se_both_strands'])
    lines = lambda t: io.BytesIO(t)
    assert bam2pat.peek(lines(pe)) == (True, False, False) and bam2pat.peek(lines(se)) == (False, False, False)
    assert bam2pat.peek(lines(b'@HD\tVN:1.6\tSO:coordinate\n' + pe)) == (True, True, False) and bam2pat.peek(lines(b'@HD\tVN:1.6\tSO:queryname\n\n' + pe)) == (True, False, False)
    assert bam2pat.peek(lines(b'@HD\tVN:1.6\n@CO\tSO:coordinate\n' + se)) == (False, False, False)
    assert bam2pat.peek(lines(SC.HEADER.encode() + b'\n')) is None and bam2pat.peek(lines(b'')) is None
    one = se.split(b'\n')[5] + b'\n'
    assert bam2pat.peek(lines(one * 150 + one.replace(b'\tNM:i:0', b'\tMM:Z:C+m,1;')))[2] is True
    assert bam2pat.peek(lines(one * 199 + one.replace(b'\tNM:i:0', b'\tMm:Z:C+m,1;')))[2] is True
    assert bam2pat.peek(lines(one * 200 + one.replace(b'\tNM:i:0', b'\tMM:Z:C+m,1;')))[2] is False      # the first 200 alignments are looked at
    with pytest.raises(bam2pat.IllegalArgumentError, match='has no FLAG'):
        bam2pat.peek(lines(b'name\tflag\tchr1\n'))


def test_cli_refusals_names_and_skip(capsys, tmp_path, monkeypatch):
    ref_dir, _ = FC.genome_dir(str(tmp_path))
    pe = tmp_path / 'pe.sam'
    pe.write_bytes(SC.case_text(SC.CASES['pe_four_flags']))
    sorted_pe = tmp_path / 'sorted.sam.gz'
    with gzip.open(str(sorted_pe), 'wb') as f:
        f.write(b'@HD\tVN:1.6\tSO:coordinate\n' + SC.case_text(SC.CASES['pe_four_flags']))
    sorted_se = tmp_path / 'sorted_se.sam'
    sorted_se.write_bytes(b'@HD\tVN:1.6\tSO:coordinate\n' + SC.case_text(SC.CASES['se_both_strands']))
    np_sam = tmp_path / 'ont.sam'
    np_sam.write_bytes(SC.case_text(SC.CASES['se_both_strands']).replace(b'\tNM:i:0', b'\tMM:Z:C+m,5;', 1))
    empty = tmp_path / 'e.sam'
    empty.write_bytes(SC.HEADER.encode())
    out = tmp_path / 'out'
    out.mkdir()
    common = ['-o', str(out), '--genome', ref_dir]
    for argv, what in (([str(tmp_path / 'x.bam')], f"is not part of this build (it reads SAM text, not BAM / CRAM): samtools view -h {tmp_path / 'x.bam'} | wgbstools bam2pat - --name x"),
                       ([str(tmp_path / 'y.cram')], 'wgbstools bam2pat - --name y'),
                       ([str(pe), '-r', 'chr1:1-100'], 'bam2pat -r / --region is not part of this build'), ([str(pe), '-s', '1-5'], 'bam2pat -s / --sites is not part of this build'),
                       ([str(pe), '-L', 'x.bed'], 'bam2pat -L / --whitelist is not part of this build'), ([str(pe), '--blacklist'], 'bam2pat --blacklist is not part of this build'),
                       ([str(pe), '--mbias'], 'bam2pat --mbias is not part of this build'), ([str(pe), '--blueprint'], 'bam2pat --blueprint is not part of this build'),
                       ([str(pe), '--nanopore'], 'bam2pat --nanopore is not part of this build'), ([str(pe), '--long'], 'bam2pat --long is not part of this build'),
                       ([str(pe), '-rg', 'g1'], 'bam2pat -rg / --read_group is not part of this build'), ([str(pe), '-d'], 'bam2pat -d / --debug is not part of this build'),
                       ([str(np_sam)], 'carries MM:Z: / Mm:Z: modification tags: --nanopore is not part of this build'),
                       ([str(sorted_pe)], 'is paired-end and sorted by coordinate (@HD SO:coordinate)'), ([str(sorted_pe)], 'samtools collate -O'),
                       ([str(sorted_pe)], 'samtools sort -n'), ([str(empty)], 'e.sam holds no alignment'), ([str(tmp_path / 'missing.sam')], 'No such file'),
                       (['-'], 'standard input needs --name'), (['-', str(pe), '--name', 'n'], 'standard input (-) is the only input'),
                       ([str(pe), '--min_cpg', '-1'], '--min_cpg and --clip must be at least 0'), ([str(pe), '-q', '300'], '-q is a mapping quality')):
        assert wgbs_tools.main(['wgbstools', 'bam2pat'] + argv + common) == 1, argv
        err = capsys.readouterr().err
        assert 'Invalid input argument' in err and what in err, (argv, err)
    assert wgbs_tools.main(['wgbstools', 'bam2pat', str(pe), '-o', str(tmp_path / 'nowhere'), '--genome', ref_dir]) == 1
    assert 'Invalid output dir' in capsys.readouterr().err
    assert not list(out.iterdir())
    # an existing output without -f: skipped with the reference's line, nothing touched (no device asked for); a coordinate-sorted
    # single-end file is no refusal of its own (it gets as far as the skip)
    for name in ('pe', 'sorted_se', 'n'):
        (out / (name + '.pat.gz')).write_bytes(b'kept')
    assert wgbs_tools.main(['wgbstools', 'bam2pat', str(pe), str(sorted_se)] + common) == 0
    err = capsys.readouterr().err
    for name in ('pe', 'sorted_se'):
        assert f"File {out / (name + '.pat.gz')} already exists. Skipping it. Use [-f] flag to force overwrite." in err
    monkeypatch.setattr('sys.stdin', io.TextIOWrapper(io.BytesIO(SC.case_text(SC.CASES['pe_four_flags']))))
    assert wgbs_tools.main(['wgbstools', 'bam2pat', '-', '--name', 'n'] + common) == 0
    assert f"File {out / 'n.pat.gz'} already exists. Skipping it." in capsys.readouterr().err
    assert {p.name: p.read_bytes() for p in out.iterdir()} == {'pe.pat.gz': b'kept', 'sorted_se.pat.gz': b'kept', 'n.pat.gz': b'kept'}


def test_stdin_chunks():
    text = SC.case_text(SC.CASES['mates'])
    for first_len in (0, 1, 700, len(text)):
        for chunk in (64, 1000, 1 << 20):
            got = list(bam2pat.stdin_chunks(text[:first_len], io.BytesIO(text[first_len:]), chunk))
            assert b''.join(got) == text and all(c.endswith(b'\n') for c in got), (first_len, chunk)
    assert b''.join(bam2pat.stdin_chunks(b'', io.BytesIO(text.rstrip(b'\n')), 500)) == text      # a last line without its newline gets one


# ---- the shared headers under the sanitizers ----
def _have_sanitizers():
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null', '-fsanitize=address,undefined'], input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason='no g++ with sanitizer runtimes')
def test_goldens_through_the_headers_under_sanitizers(golden, tmp_path):
    """tests/native/san_bam2pat.cpp — the whole of `bam2pat` on the host by the functions the kernels call, the text, the loci and the table
    of exactly their size — built plain and with ASan + UBSan: both write every golden's bytes and the restatement's counters; exit status 0
    says that no read left its array"""
    loci, chroms = str(tmp_path / 'loci.u32'), str(tmp_path / 'chroms.tsv')
    LOCI.tofile(loci)
    with open(chroms, 'w') as f:
        f.write(''.join('%s\t%d\n' % c for c in CHROMS))
    rng = np.random.default_rng(11)
    worlds = {'world%d' % k: SC.random_world(rng, 250) for k in range(3)}
    for kind, flags in (('plain', []), ('asan_ubsan', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exe = str(tmp_path / ('san_bam2pat_' + kind))
        subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-ffp-contract=off', '-I', CSRC, op.join(HERE, 'native', 'san_bam2pat.cpp'), '-o', exe] + flags)
        env = {'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'}
        jobs = [(name, SC.case_text(case), SC.case_args(case), golden[name]['stdout'].encode()) for name, case in SC.CASES.items()]
        jobs += [(name, text, a, ref(text, a)[0]) for name, (text, a) in worlds.items()]
        jobs.append(('no_last_newline', SC.case_text(SC.CASES['mates']).rstrip(b'\n'), SC.case_args(SC.CASES['mates']), golden['mates']['stdout'].encode()))
        for name, text, a, want in jobs:
            path = str(tmp_path / (name + '.sam'))
            with open(path, 'wb') as f:
                f.write(text)
            r = subprocess.run([exe, path, loci, chroms] + [str(int(a[k])) for k in ARG_ORDER], capture_output=True, timeout=120, env=env)
            assert r.returncode == 0, (kind, name, r.stderr[-3000:])
            assert r.stdout == want, (kind, name)
            assert r.stderr.decode() == 'stats ' + ' '.join(str(ref(text, a)[1][k]) for k in BR.COUNTERS) + '\n', (kind, name)
