"""`wgbstools frag_len` without a GPU: the host plan (csrc/frag_plan.h through tests/native/fragplan_host.cpp) against numpy and
every refusal text; the restatement tests/frag_ref.py — its streaming walk and its read-by-read rule — against every golden line of
the reference's tools (tests/golden/frag_cases.json); the command's ordering of a blocks table against the order the reference's
own `sort` gave; argument parsing and help through the dispatcher."""
import ctypes as C
import hashlib
import json
import os.path as op
import subprocess

import numpy as np
import pytest

import frag_cases as FC
import frag_ref as FR
from wgbs_tools_amd import frag_len, wgbs_tools
from wgbs_tools_amd.beta_to_blocks import load_blocks_file
from wgbs_tools_amd.genome import IllegalArgumentError

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(HERE)
CSRC = op.join(ROOT, 'wgbs_tools_amd', 'csrc')
SRC = op.join(HERE, 'native', 'fragplan_host.cpp')
LIB = op.join(HERE, 'native', 'libfragplan_host.so')
DEPS = [SRC, op.join(ROOT, 'include', 'wgbsseg.h')] + [op.join(CSRC, h) for h in ('frag_plan.h', 'homog_plan.h', 'block_plan.h')]
OK, E_ARG = 0, -1
P = C.c_void_p


@pytest.fixture(scope='module')
def L():
    """tests/native/libfragplan_host.so (built when missing or older than its sources)"""
    if not op.isfile(LIB) or op.getmtime(LIB) < max(op.getmtime(d) for d in DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', SRC, '-o', LIB])
    lib = C.CDLL(LIB)
    lib.fragplan_constants.argtypes = [P]
    lib.fragplan.restype = C.c_int
    lib.fragplan.argtypes = [P, P, C.c_int64, C.c_int32, C.c_int32, P, P, P, C.c_char_p, C.c_size_t]
    return lib


@pytest.fixture(scope='module')
def golden():
    with open(op.join(HERE, 'golden', 'frag_cases.json')) as f:
        return json.load(f)


def plan(L, s, e, m=30, groups=-1, null=False):
    s, e = np.ascontiguousarray(s, dtype=np.int64), np.ascontiguousarray(e, dtype=np.int64)
    start, pmax = np.full(s.size, -7, dtype=np.int32), np.full(s.size, -7, dtype=np.int32)
    info = np.full(4, -7, dtype=np.int64)
    msg = C.create_string_buffer(600)
    rc = L.fragplan(None if null else s.ctypes.data, None if null else e.ctypes.data, s.size, m, groups, start.ctypes.data, pmax.ctypes.data,
                    info.ctypes.data, msg, 600)
    return rc, msg.value.decode(), start, pmax, info.tolist()


def test_constants(L):
    k = np.zeros(3, dtype=np.int64)
    L.fragplan_constants(k.ctypes.data)
    assert k.tolist() == [2048, 1 << 20, 1536]
    assert FC.LDS_BINS == k[0] and frag_len.MAX_FRAG_SIZE == k[1]


def test_plan_tables_against_numpy(L):
    rng = np.random.default_rng(20261021)
    for _ in range(50):
        nb = int(rng.integers(1, 300))
        s = np.sort(rng.integers(1, 500, nb))                     # equal starts among them
        e = s + rng.integers(1, rng.choice([3, 50, 2000]), nb)     # nested: the ends do not ascend
        rc, msg, start, pmax, info = plan(L, s, e, 17, 3)
        assert rc == OK and msg == ''
        assert np.array_equal(start, s) and np.array_equal(pmax, np.maximum.accumulate(e))
        assert info == [int(e[-1]), nb, 17, 3]
    # the block that sorts last lies inside an earlier one: end_last is ITS end, not the largest
    rc, _, start, pmax, info = plan(L, [10, 40, 40], [20, 100, 45])
    assert rc == OK and info[0] == 45 and pmax.tolist() == [20, 100, 100] and info[3] == 1536
    # the largest values an int32 table holds
    rc, _, start, pmax, info = plan(L, [2 ** 31 - 2], [2 ** 31 - 1], 1 << 20)
    assert rc == OK and start.tolist() == [2 ** 31 - 2] and pmax.tolist() == [2 ** 31 - 1] and info[0] == 2 ** 31 - 1
    # no selection
    rc, _, _, _, info = plan(L, [], [], 30)
    assert rc == OK and info == [0, 0, 30, 1536]


def test_plan_refusals(L):
    for m in (0, -4, (1 << 20) + 1):
        rc, msg, *_ = plan(L, [1], [2], m)
        assert rc == E_ARG and msg == 'frag_len: max_frag_size %d (1..1048576)' % m
    rc, msg, *_ = plan(L, [1, 2], [2, 3], 30, null=True)
    assert rc == E_ARG and msg == 'frag_len: bad block list'
    rc, msg, *_ = plan(L, [5, 0], [9, 3])
    assert rc == E_ARG and msg == 'frag_len: block 1 (in sorted order) has startCpG 0 < 1'
    rc, msg, *_ = plan(L, [5, 7], [9, 7])
    assert rc == E_ARG and msg == 'frag_len: block 1 (in sorted order) has endCpG 7 (startCpG 7)'
    rc, msg, *_ = plan(L, [5], [2 ** 31])
    assert rc == E_ARG and msg == 'frag_len: block 0 (in sorted order) has endCpG 2147483648 (startCpG 5)'
    rc, msg, *_ = plan(L, [5, 4], [9, 9])
    assert rc == E_ARG and msg == 'frag_len: blocks must be given sorted by startCpG (block 1)'
    for g in (0, 1537):
        rc, msg, *_ = plan(L, [5], [9], 30, g)
        assert rc == E_ARG and msg == 'frag_len: %d workgroups (1..1536, or -1 for the default)' % g
    assert plan(L, [5, 5], [9, 7])[0] == OK                        # equal starts come in the caller's order


def _blocks_of(where):
    return FR.cview_order(FC.table_pairs(where[1]))


def _case_blocks(rec):
    where = rec['where']
    if not where:
        return None
    if where[0] == '-L':
        return _blocks_of(where)
    s, e = rec['sites']
    return np.array([s]), np.array([e])


def test_every_case_has_a_golden(golden):
    assert sorted(golden) == sorted(FC.CASES)
    for name, case in FC.CASES.items():
        assert golden[name]['pat_sha1'] == hashlib.sha1(FC.case_pat(case)).hexdigest(), name
        assert golden[name]['where'] == FC.case_where(case) and golden[name]['m'] == case['m'], name


@pytest.mark.parametrize('name', sorted(FC.CASES))
def test_restatement_equals_golden(name, golden):
    rec = golden[name]
    text = FC.case_pat(FC.CASES[name])
    blocks = _case_blocks(rec)
    rule = FR.frag_hist(text, rec['m'], blocks)
    assert FR.line_of(rule) == rec['stdout'], name
    if blocks is not None:
        assert FR.frag_hist(text, rec['m'], blocks, walk=True) == rule
        assert len(FR.select_rule(FR.reads_of(text), *blocks)) == rec['passed']


def test_boundary_cases_select_what_the_contract_says(golden):
    """which of the boundary reads each list lets through (their counts are powers of two): with the issue's list the block that
    sorts last is [40, 50) — "40\\t45" < "40\\t50" — and the read at 46 counts; with [40, 100) in its place [40, 45) sorts last and
    the reads at 45, 46 and 49 are dropped although [40, 100) holds them"""
    got = {}
    for name in ('L_boundary', 'L_boundary_last_nested'):
        rec = golden[name]
        got[name] = sum(int(v) for v in rec['stdout'].split())
    assert got['L_boundary'] == 2 + 4 + 64 + 128 + 256 + 512 + 1024
    assert got['L_boundary_last_nested'] == 2 + 4 + 64 + 128


def test_walk_equals_rule_on_random_worlds():
    rng = np.random.default_rng(20261022)
    n = 0
    while n < 40:
        text, m, blocks = FC.random_world(rng)
        if blocks is None:
            continue
        n += 1
        assert FR.frag_hist(text, m, blocks, walk=True) == FR.frag_hist(text, m, blocks)


def test_restatement_refusals():
    good = b'chr1\t1\tCCCC\t1\nchr1\t3\tTTTT\t2\n'
    for bad in (b'chr1\t5\tCT\n', b'chr1\tx\tCT\t3\n', b'chr1\t5\tCT\t\n', b'chr1\t5\t\t3\n'):
        with pytest.raises(FR.Refused) as e:
            FR.frag_hist(good + bad, 30)
        assert (e.value.kind, e.value.offset) == ('bad', len(good))
    unsorted = good + b'chr1\t2\tCCC\t1\n'
    assert FR.frag_hist(unsorted, 4) == [0, 0, 1, 3]
    with pytest.raises(FR.Refused) as e:
        FR.frag_hist(unsorted, 4, (np.array([1]), np.array([9])))
    assert (e.value.kind, e.value.offset) == ('desc', len(good))


@pytest.mark.parametrize('name', sorted(n for n, c in FC.CASES.items() if c['where'][:1] == ['-L']))
def test_python_ordering_equals_sort(name, golden, tmp_path):
    """frag_len.cview_order on the table as the command reads it == the order `cut -f4-5 | sort -k1,1n` (LC_ALL=C) gave the
    reference (its header and NA lines left out), equal starts included"""
    rec = golden[name]
    path = tmp_path / 'blocks.bed'
    path.write_text(rec['where'][1])
    s, e = frag_len.cview_order(load_blocks_file(str(path)), str(path))
    want = [ln.split('\t') for ln in rec['order'] if ln.split('\t')[0].isdigit()]
    assert [[str(a), str(b)] for a, b in zip(s.tolist(), e.tolist())] == want
    rs, re_ = _blocks_of(rec['where'])
    assert np.array_equal(rs, s) and np.array_equal(re_, e)


def test_ordering_by_the_files_own_text(tmp_path):
    path = tmp_path / 'b.bed'
    path.write_text('chr1\t1\t2\t50\t60\nchr1\t1\t2\t50\t100\nchr1\t1\t2\t7\t9\nchr1\t1\t2\tNA\tNA\n')
    s, e = frag_len.cview_order(load_blocks_file(str(path)))
    assert s.tolist() == [7, 50, 50] and e.tolist() == [9, 100, 60]


def test_block_list_refusals(tmp_path):
    path = tmp_path / 'b.bed'
    for text, what in (('chr1\t1\t2\t5\t9\nchr1\t1\t2\t7\t7\n', 'row 2 has endCpG 7 <= startCpG 7'),
                       ('chr1\t1\t2\t0\t9\n', 'row 1 has startCpG 0 < 1'),
                       ('chr1\t1\t2\tNA\tNA\n', 'no row with startCpG and endCpG')):
        path.write_text(text)
        with pytest.raises(IllegalArgumentError, match=what):
            frag_len.cview_order(load_blocks_file(str(path)), str(path))


def test_cli_surface(capsys, tmp_path):
    assert 'frag_len' in wgbs_tools.COMMANDS and 'frag_len' not in wgbs_tools.REFERENCE_ONLY
    with pytest.raises(SystemExit) as e:
        wgbs_tools.main(['wgbstools', 'frag_len', '-h'])
    assert e.value.code == 0
    out = capsys.readouterr()
    assert 'not part of this build' not in out.out + out.err
    for flag in ('--max_frag_size', '--outdir', '--display', '--sites', '--region', '--bed_file', '--genome', '--device', '--inflate', '--verbose'):
        assert flag in out.out
    args = frag_len.parse_args(['a.pat.gz', 'b.pat.gz', '-v', '-m', '12', '-s', '5-9', '--inflate', 'device', '-o', 'figs'])
    assert (args.pat_paths, args.verbose, args.max_frag_size, args.sites, args.inflate, args.outdir, args.display) == \
        (['a.pat.gz', 'b.pat.gz'], True, 12, '5-9', 'device', 'figs', False)
    assert frag_len.parse_args(['a.pat.gz']).max_frag_size == 30
    with pytest.raises(SystemExit):
        frag_len.parse_args(['a.pat.gz', '-s', '5-9', '-r', 'chr1:1-2'])
    # the checks that need no GPU: the file list, then --max_frag_size
    assert wgbs_tools.main(['wgbstools', 'frag_len', str(tmp_path / 'missing.pat.gz')]) == 1
    assert 'No such file' in capsys.readouterr().err
    pat = tmp_path / 'x.pat.gz'
    pat.write_bytes(b'')
    for m in ('0', str((1 << 20) + 1)):
        assert wgbs_tools.main(['wgbstools', 'frag_len', str(pat), '-m', m]) == 1
        assert '--max_frag_size must be in [1, 1048576]' in capsys.readouterr().err
    other = tmp_path / 'x.pat'
    other.write_bytes(b'')
    assert wgbs_tools.main(['wgbstools', 'frag_len', str(other)]) == 1
    assert 'must end with .pat.gz' in capsys.readouterr().err
