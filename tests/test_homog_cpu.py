"""`wgbstools homog` without a GPU: the golden cases (written by the reference itself, tests/golden/make_golden_homog.py) against
the test restatement tests/homog_ref.py, the bin edges against the reference's float parse, the command line's checks and
messages, and the dispatcher."""
import json
import os.path as op

import numpy as np
import pytest

import homog_cases as HC
import homog_ref as HR
from wgbs_tools_amd import homog, wgbs_tools
from wgbs_tools_amd.genome import IllegalArgumentError

ROOT = op.dirname(op.dirname(op.abspath(__file__)))


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'homog_cases.json')) as f:
        return json.load(f)


def test_golden_covers_the_cases(golden):
    assert sorted(golden) == sorted(HC.CASES)
    assert golden['seg_l3']['rows'] > 6000                      # the reference's own full-file branch, unpatched
    assert any('--binary' in c['args'] and '16' in c['args'] for c in golden.values())


@pytest.mark.parametrize('name', sorted(HC.CASES))
def test_restatement_reproduces_the_reference(name, golden):
    import hashlib
    rec = golden[name]
    case = HC.CASES[name]
    assert rec['pat'] == case['pat'] and rec['blocks'] == case['blocks'] and rec['args'] == case['args']
    pat = HC.case_pat(case['pat'])
    assert hashlib.sha1(pat).hexdigest() == rec['pat_sha1'], 'the case generator changed'
    _, _, btext = HC.case_blocks(case['blocks'])
    got = HR.digests(pat, btext, case['args'])
    for k, v in got.items():
        assert v == rec[k], (name, k)


def test_cases_reach_their_corners(golden):
    """what each case is there for actually happens in it"""
    s, e, _ = HC.case_blocks(HC.CASES['nested']['blocks'])
    assert (np.maximum.accumulate(e)[:-1] > e[1:]).any() and e[0] > e[-1]                  # nesting; a block past the last end
    s, e, _ = HC.case_blocks(HC.CASES['unsorted']['blocks'])
    o = np.lexsort((e, s))
    assert not np.array_equal(o, np.argsort(s, kind='stable'))                               # the re-ordering quirk bites
    s, e, _ = HC.case_blocks(HC.CASES['duplicates']['blocks'])
    assert len(set(zip(s.tolist(), e.tolist()))) < s.size
    pat = HC.case_pat(HC.CASES['long_reads_signed']['pat']).decode().splitlines()
    assert max(len(ln.split('\t')[2]) for ln in pat) >= 2000
    assert any(ln.split('\t')[3].startswith('-') for ln in pat) and any(ln.split('\t')[3].startswith('+') for ln in pat)
    assert int(pat[0].split('\t')[1]) < 1 and int(pat[-1].split('\t')[1]) > 8000
    _, _, btext = HC.case_blocks(HC.CASES['deep_bin16']['blocks'])
    _, vals = HR.homog(HC.case_pat(HC.CASES['deep_bin16']['pat']), btext)
    assert (vals.max(axis=1) > 65535).any()                                                 # both trims (8 and 16 bits) bite


def test_edges_match_the_reference_parse():
    """the range text and its float32 values for l = 2..200 (l = 2 needs -t; the default text is still well defined)"""
    for rlen in range(2, 201):
        text, want = HR.edges_of(rlen)
        assert homog.range_text(rlen) == text
        if rlen == 2:                                            # "0,0.501,0.5,1": not ascending, refused (the reference asks for -t)
            with pytest.raises(IllegalArgumentError, match='Invalid range'):
                homog.parse_range(text)
            got = np.array([homog._strtof(t)[0] for t in text.split(',')], dtype=np.float32)
        else:
            got = homog.parse_range(text)
        assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), rlen
    assert homog.range_text(3) == '0,0.334,0.667,1'
    assert homog.range_text(4) == '0,0.251,0.75,1'
    assert homog.range_text(5) == '0,0.201,0.8,1'
    assert homog.range_text(2, '0.25,0.75') == '0,0.25,0.75,1'
    # one rounding: the decimal straight to float32, not through a double
    assert homog.parse_range('0,0.334,0.667,1')[1] == np.float32(0.334)
    with pytest.raises(IllegalArgumentError):
        homog.parse_range('0,0.5,0.5,1')


def _args(*a):
    return homog.parse_args(['x.pat.gz', '-b', 'b.bed'] + list(a))


@pytest.mark.parametrize('argv,msg', [
    (['--nr_bits', '12'], 'nr_bits must be in {8, 16}'),
    (['-l', '1'], 'rlen must be >= 2'),
    (['-t', '0.2'], 'Invalid thresholds'),
    (['-t', '0.7,0.3'], 'Invalid thresholds'),
    (['-t', '0,0.5'], 'Invalid thresholds'),
    (['-t', '0.5,1'], 'Invalid thresholds'),
    (['-l', '2'], 'for rlen==2, --thresholds must be specified'),
])
def test_argument_checks(argv, msg):
    with pytest.raises(IllegalArgumentError, match=msg.replace('{', r'\{').replace('}', r'\}')):
        homog.check_args(_args(*argv))


def test_argument_checks_pass():
    homog.check_args(_args())
    homog.check_args(_args('-l', '2', '-t', '0.25,0.75', '--nr_bits', '16'))


def test_out_dir_and_prefix_are_exclusive():
    with pytest.raises(SystemExit):
        homog.parse_args(['x.pat.gz', '-b', 'b.bed', '-o', 'd', '-p', 'p'])


def test_input_checks(tmp_path, capsys):
    pat = tmp_path / 's.pat.gz'
    pat.write_bytes(b'')
    blocks = tmp_path / 'b.bed'
    blocks.write_text('chr1\t10\t20\t1\t5\n')
    cases = [
        ([str(tmp_path / 's.pat'), '-b', str(blocks)], 'must end with .pat.gz'),
        ([str(tmp_path / 'nope.pat.gz'), '-b', str(blocks)], 'No such file'),
        ([str(pat), str(tmp_path / 'nope.pat.gz'), '-b', str(blocks)], 'No such file'),
    ]
    for argv, msg in cases:
        assert wgbs_tools.main(['wgbstools', 'homog'] + argv) == 1
        assert msg in capsys.readouterr().err
    for text, msg in (('chr1\t10\t20\t5\t5\n', 'Invalid blocks file'), ('chr1\t10\t20\tNA\t5\n', 'Invalid blocks file'),
                      ('chr1\t10\t20\t0\t5\n', 'startCpG 0 < 1')):
        blocks.write_text(text)
        assert wgbs_tools.main(['wgbstools', 'homog', str(pat), '-b', str(blocks), '-o', str(tmp_path)]) == 1
        assert msg in capsys.readouterr().err


def test_homog_is_dispatched(capsys):
    assert 'homog' in wgbs_tools.COMMANDS and 'homog' not in wgbs_tools.REFERENCE_ONLY
    with pytest.raises(SystemExit) as e:
        wgbs_tools.main(['wgbstools', 'homog', '-h'])
    assert e.value.code == 0
    out = capsys.readouterr()
    assert '--blocks_file' in out.out and 'not part of this build' not in out.err


def test_merge_and_trim_helpers():
    """the product's host-side pieces against the restatement's: row multiplication and the narrow types"""
    _, _, btext = HC.case_blocks(HC.CASES['duplicates']['blocks'])
    rows = HR.parse_blocks(btext)

    class T:
        startCpG = np.array([r[1] for r in rows], dtype=np.int64)
        endCpG = np.array([r[2] for r in rows], dtype=np.int64)

        def __len__(self):
            return len(rows)

        def coords_of(self, idx):
            return [rows[i][0] for i in idx]
    left, right = homog.merge_rows(T())
    keys = [r[0] + (r[1], r[2]) for r in rows]
    want = [(i, j) for i, k in enumerate(keys) for j, k2 in enumerate(keys) if k2 == k]
    assert list(zip(left.tolist(), right.tolist())) == want
    rng = np.random.default_rng(5)
    v = rng.integers(-300, 200000, size=(500, 3))
    for nb in (8, 16):
        assert homog.trim_uxm(v, nb).tobytes() == HR.trim(v, nb).tobytes()
