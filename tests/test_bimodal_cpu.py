"""`wgbstools test_bimodal` without a GPU: the golden cases (written by the reference itself, tests/golden/make_golden_bimodal.py)
against the test restatement tests/bimodal_ref.py, the census of the hand-built corner cases (tests/bimodal_corners.py: each case
reaches the corners it is named for), the Benjamini-Hochberg step on hand-worked cases, the command line's checks and messages, and
the dispatcher."""
import json
import os.path as op

import numpy as np
import pytest

import bimodal_cases as BC
import bimodal_corners as BK
import bimodal_ref as BR
from wgbs_tools_amd import test_bimodal as tb
from wgbs_tools_amd import wgbs_tools
from wgbs_tools_amd.genome import IllegalArgumentError

ROOT = op.dirname(op.dirname(op.abspath(__file__)))
with open(op.join(ROOT, 'tests', 'golden', 'bimodal_cases.json')) as _f:
    GOLDEN = json.load(_f)


def test_golden_covers_the_cases():
    cases = GOLDEN['cases']
    assert GOLDEN['n_cases'] == len(BC.CASES) and set(cases) | {d['case'] for d in GOLDEN['dropped']} == set(BC.CASES)
    assert len(GOLDEN['dropped']) <= 3
    # the FDR quirks: empty because the first block is not rejected, empty because every block is, everything printed
    assert cases['L_first_not_rejected']['text'] == '' and min(b[4] for b in cases['L_first_not_rejected']['per_block']) > 0.05
    assert cases['L_all_rejected']['text'] == '' and cases['L_all_rejected_printed']['text'].count('\n') == 6
    assert cases['s_empty']['text'] == ''
    assert any(c['text'].startswith('LL: ') for c in cases.values())


@pytest.mark.parametrize('name', sorted(GOLDEN['cases']))
def test_restatement_reproduces_the_reference(name):
    import hashlib
    rec = GOLDEN['cases'][name]
    case = BC.CASES[name]
    pat, bed, args = BC.case_inputs(case)
    assert hashlib.sha1(pat).hexdigest() == rec['pat_sha1'], 'the case generator changed'
    strict = '--strict' in args
    min_len = int(args[args.index('--min_len') + 1]) if '--min_len' in args else 1
    starts, reads = BR.parse_pat(pat)
    if bed is None:
        s, e = [case['sites'][0]], [case['sites'][1]]
        res = [BR.block_result(starts, reads, s[0], e[0], strict, min_len)]
        assert BR.single_text(res[0]) == rec['text']
    else:
        assert hashlib.sha1(bed.encode()).hexdigest() == rec['bed_sha1']
        chroms = [c for c, _ in BC.CHROMS]
        lines = [ln for c in chroms for ln in bed.splitlines() if not ln.startswith('#') and ln.split('\t')[0] == c]
        s = [int(ln.split('\t')[3]) for ln in lines]
        e = [int(ln.split('\t')[4]) for ln in lines]
        res = [BR.block_result(starts, reads, a, b, strict, min_len) for a, b in zip(s, e)]
        p32 = np.array([BR.pvalue(r[0], r[1], r[3], r[4]) for r in res]).astype(np.float32)
        assert BR.multi_text(lines, p32, '--print_all_regions' in args) == rec['text']
    assert len(res) == len(rec['per_block'])
    off = 0
    for r, (ll0, ll, ncols, rows, _) in zip(res, rec['per_block']):
        assert (r[3], r[4]) == (ncols, rows)
        if rows:
            assert r[0] == pytest.approx(ll0, rel=1e-12)
            off += r[1] != pytest.approx(ll, rel=1e-12)
    # ll_em: a row with as many C as T sits on a near-tie of the first assignment (p_t = 1 - 0.9 is not 0.1), which the
    # reference's BLAS order of summation may break the other way; such blocks are few and leave the printed text alone
    assert off <= max(1, len(res) // 20), off


def test_cases_reach_their_corners():
    """what each case is there for actually happens in it"""
    strict = [ln.split('\t') for ln in BC.case_inputs(BC.CASES['L_strict'])[0].decode().splitlines()]
    assert max(len(t[2]) for t in strict) > 150                                              # reads longer than the look-back
    case = BC.CASES['L_default']
    pat, bed, _ = BC.case_inputs(case)
    reads = [ln.split('\t') for ln in pat.decode().splitlines()]
    assert any(t[3] == '0' for t in reads)
    assert 'chrUn' in bed
    s, e = BC.case_blocks(case['blocks'])
    assert len(set(zip(s.tolist(), e.tolist()))) < s.size                                    # duplicates
    assert (np.maximum.accumulate(e)[:-1] > e[1:]).any()                                     # nesting
    assert (e - s > 256).any()                                                               # wider than the LDS tables
    starts, rr = BR.parse_pat(pat)
    res = [BR.block_result(starts, rr, a, b) for a, b in zip(s.tolist(), e.tolist())]
    assert any(r[4] == 0 for r in res) and max(r[3] for r in res) > 256
    p = np.array([BR.pvalue(r[0], r[1], r[3], r[4]) for r in res])
    assert (p < 1e-6).any() and (p > 0.5).any()                                              # bimodal and unimodal blocks


@pytest.mark.parametrize('name', sorted(BK.cases()))
def test_corner_case_reaches_its_corners(name):
    """a case that stops reaching a corner it is named for must not go on passing"""
    case = BK.cases()[name]
    got = BK.census(name)
    assert case['corners'] and case['corners'] <= set(BK.CORNERS)
    assert not case['corners'] - got, sorted(case['corners'] - got)
    assert len(case['text']) < 16384                              # a few KB of pat text each
    assert sum(r[4] for r in BK.want(name)) <= 10 * 200000        # and a restatement that stays in seconds


def test_corner_cases_cover_every_corner():
    named = set().union(*(c['corners'] for c in BK.cases().values()))
    assert named == set(BK.CORNERS), sorted(set(BK.CORNERS) ^ named)
    # the numbers behind some of the names
    deep = BK.want('deep')[0]
    assert deep[4] <= 200000 and deep[2] > 100000                 # rows; the sum of the columns' counts
    assert BK.want('slow')[0][5] >= 8
    zero = BK.want('zero_counts')
    assert zero[1][3:] == (6, 0, 0) and zero[1][:3] == (0.0, 0.0, 0.0)      # counts all 0: the columns, nothing else
    lock = BK.cases()['lockstep']
    assert BK.want('blocks_descending') == BK.want('lockstep')[::-1]
    assert len(BK.cases()['blocks_shuffled']['s']) > len(lock['s'])


def test_fdr_bh_hand_worked():
    # n = 4, alpha 0.05: thresholds 0.0125, 0.025, 0.0375, 0.05
    rej, cor = tb.fdr_bh(np.array([0.01, 0.03, 0.035, 0.2], dtype=np.float32))
    assert rej.tolist() == [True, True, True, False]                                         # up to the last rejection
    want = np.minimum.accumulate((np.array([0.01, 0.03, 0.035, 0.2], dtype=np.float32).astype(np.float64) / (np.arange(1, 5) / 4.0))[::-1])[::-1]
    assert cor.tolist() == want.tolist()
    assert cor[0] == pytest.approx(0.04, rel=1e-6) and cor[1] == pytest.approx(0.04666666, rel=1e-6) and cor[3] == pytest.approx(0.2, rel=1e-6)
    rej, cor = tb.fdr_bh(np.array([0.5, 0.9], dtype=np.float32))              # p / (i / n) = 1.0, 0.9 -> both 0.9 (float32's)
    assert not rej.any() and cor.tolist() == [float(np.float32(0.9))] * 2
    _, cor = tb.fdr_bh(np.array([0.6, 0.7], dtype=np.float32))                 # 1.2 clipped to 1
    assert cor.tolist() == [float(np.float32(0.7)) * 2 if False else min(1.0, float(np.float32(0.7)))] * 2
    for p in (np.array([0.01, 0.02, 0.5]), np.array([0.2, 0.3]), np.array([0.0, 0.0, 0.0])):
        a, b = tb.fdr_bh(p.astype(np.float32)), BR.fdr_bh(p.astype(np.float32))
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist()


def test_choose_quirks():
    lines = ['a', 'b', 'c']
    assert tb.choose_by_fdr(lines, [0.9, 0.8, 0.7]) == []                                    # the first not rejected
    assert tb.choose_by_fdr(lines, [0.0, 0.0, 0.0]) == []                                    # every one rejected: argmax -> 0
    got = tb.choose_by_fdr(lines, [0.0, 0.0, 0.0], print_all=True)
    assert [g[0] for g in got] == lines
    got = tb.choose_by_fdr(lines, [0.5, 0.0, 0.001])                                         # stable sort by p
    assert [g[0] for g in got] == ['b', 'c']
    got = tb.choose_by_fdr(['x', 'y', 'z', 'w'], [1.0, 0.0, 1.0, 0.0], print_all=True)
    assert [g[0] for g in got] == ['y', 'w', 'x', 'z']
    assert tb.choose_by_fdr([], []) == []


def _args(*a):
    return tb.parse_args(['x.pat.gz'] + list(a))


def test_where_is_required_and_exclusive():
    with pytest.raises(SystemExit):
        tb.parse_args(['x.pat.gz'])
    with pytest.raises(SystemExit):
        tb.parse_args(['x.pat.gz', '-s', '1-5', '-L', 'b.bed'])
    a = _args('-L', 'b.bed', '--strict', '--min_len', '3', '-o', 'o.txt', '-v', '--print_all_regions', '-@', '4')
    assert a.strict and a.min_len == 3 and a.out_file == 'o.txt' and a.verbose and a.print_all_regions and a.bed_file == 'b.bed'
    a = _args('-s', '10-20')
    assert a.out_file == '-' and a.min_len == 1 and not a.strict and a.genome == 'default' and a.device == 0


def test_input_checks(tmp_path, capsys):
    pat = tmp_path / 's.pat.gz'
    pat.write_bytes(b'')
    bed = tmp_path / 'b.bed'
    cases = [
        (['-L', str(bed)], 'No such file'),
        ([str(tmp_path / 'nope.pat.gz'), '-L', str(bed)], 'No such file'),
        ([str(pat), '-L', str(bed), '--min_len', '0'], '--min_len must be at least 1'),
    ]
    for argv, msg in cases:
        if argv[0].startswith('-'):
            argv = [str(pat)] + argv
        assert wgbs_tools.main(['wgbstools', 'test_bimodal'] + argv) == 1
        assert msg in capsys.readouterr().err
    bed.write_text('chr1\t10\t20\n')
    assert wgbs_tools.main(['wgbstools', 'test_bimodal', str(pat), '-L', str(bed)]) == 1
    err = capsys.readouterr().err
    assert 'less than 5 columns' in err and 'wgbstools convert -L' in err


def test_blocks_rows_and_refusals(tmp_path):
    bed = tmp_path / 'b.bed'
    bed.write_text('#c\ts\te\ta\tb\nchr2\t1\t2\t30\t35\textra\nchr1\t1\t2\t3\t9\nchrUn\t5\t6\t1\t2\nchr1\t7\t8\t9\t12\n')
    rows = tb.read_bed(str(bed))
    got = tb.select_blocks(rows, ('chr1', 'chr2'), str(bed))
    assert got == [('chr1\t1\t2\t3\t9', 3, 9), ('chr1\t7\t8\t9\t12', 9, 12), ('chr2\t1\t2\t30\t35\textra', 30, 35)]
    for text, msg in (('chr1\t1\t2\tNA\t5\n', 'no integer CpG index'), ('chr1\t1\t2\t5\t5\n', 'endCpG 5'),
                      ('chr1\t1\t2\t0\t5\n', 'startCpG 0'), ('chr1\t1\t2\t3\t2.5\n', 'no integer CpG index')):
        bed.write_text(text)
        with pytest.raises(IllegalArgumentError, match=msg):
            tb.select_blocks(tb.read_bed(str(bed)), ('chr1',), str(bed))


def test_test_bimodal_is_dispatched(capsys):
    assert 'test_bimodal' in wgbs_tools.COMMANDS and 'test_bimodal' not in wgbs_tools.REFERENCE_ONLY
    with pytest.raises(SystemExit) as e:
        wgbs_tools.main(['wgbstools', 'test_bimodal', '-h'])
    assert e.value.code == 0
    out = capsys.readouterr()
    assert '--print_all_regions' in out.out and 'not part of this build' not in out.err
