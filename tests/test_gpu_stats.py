"""Per-sample statistics on the GPU (k_sample_stats behind wgbsseg_sample_stats): every field against the numpy restatement
tests/stats_ref.py as integers, over the sizes, sample counts, row widths and range lists of tests/stats_cases.py; the 128-bit
carry case; bit-identical repeats and re-cut ranges; the refusals; `wgbstools beta_cov` and `beta_stats` end to end against
what the reference printed (tests/golden/stats_cases.json), byte for byte."""
import json
import os.path as op

import numpy as np
import pytest

import stats_cases as SC
import stats_ref as SR
from wgbs_tools_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))


@pytest.fixture(scope='module')
def seg():
    with _lib.Segmenter(0) as s:
        yield s


def _load(seg, rows, elem):
    (seg.set_betas if elem == 1 else seg.set_lbetas)(rows)


def _check(got, rows, ranges, depth_at, what):
    assert len(got) == len(rows)
    for s, r in enumerate(rows):
        assert SR.as_dict(got[s]) == SR.expect(r, ranges, depth_at), (what, 'sample', s)
        assert int(got[s]['reserved']) == 0


@pytest.mark.parametrize('elem', [1, 2])
@pytest.mark.parametrize('n', SC.SIZES)
def test_fields_match_restatement(seg, n, elem):
    sets = SC.range_sets(n)
    for n_samples in SC.SAMPLES:
        rows = SC.world(n, n_samples, elem)
        _load(seg, rows, elem)
        for name, ranges in sets.items():
            _check(seg.sample_stats(ranges), rows, ranges, 10, (n, n_samples, elem, name))
    if n_samples >= 3:
        assert int(seg.sample_stats(sets['whole'])[1]['covered']) == 0            # the all-zero sample


@pytest.mark.parametrize('depth_at', [0, 1, 255, 256, 40000])
def test_depth_threshold(seg, depth_at):
    for elem in (1, 2):
        rows = SC.world(4097, 3, elem, seed=1)
        _load(seg, rows, elem)
        ranges = SC.range_sets(4097)['random']
        _check(seg.sample_stats(ranges, depth_at=depth_at), rows, ranges, depth_at, (elem, depth_at))


def test_repeat_and_recut_give_identical_bytes(seg):
    n = 70001
    for elem in (1, 2):
        rows = SC.world(n, 5, elem, seed=2)
        _load(seg, rows, elem)
        whole = seg.sample_stats([(0, n)])
        assert whole.tobytes() == seg.sample_stats([(0, n)]).tobytes()
        for cuts in ([1], [7, 8, 9, 4096, 4097], [n - 1], list(range(3, n, 997))):
            edges = [0] + cuts + [n]
            pieces = list(zip(edges[:-1], edges[1:]))
            assert seg.sample_stats(pieces).tobytes() == whole.tobytes(), cuts
        part = [(5, 1001), (1001, 30000), (30003, 69999)]
        recut = [(5, 6), (6, 6), (6, 29999), (29999, 30000), (30003, 50000), (50000, 69999)]
        assert seg.sample_stats(part).tobytes() == seg.sample_stats(recut).tobytes()


def test_128_bit_carries(seg):
    rows = SC.carry_world()
    _load(seg, rows, 1)
    want = [SR.expect(r, SC.CARRY_RANGES['whole']) for r in rows]
    assert all(w['ratio_hi'] > 0 for w in want)
    whole = seg.sample_stats(SC.CARRY_RANGES['whole'])
    assert [SR.as_dict(g) for g in whole] == want
    assert seg.sample_stats(SC.CARRY_RANGES['split']).tobytes() == whole.tobytes()
    inner = seg.sample_stats(SC.CARRY_RANGES['inner'])
    assert SR.as_dict(inner[3]) == SR.expect(rows[3], SC.CARRY_RANGES['inner'])
    assert seg.last_block_sums_ms() > 0.0


@pytest.mark.parametrize('ranges, bad', [([(0, 10), (20, 15)], 1), ([(0, 10), (9, 15)], 1), ([(5, 8), (0, 3)], 1), ([(0, 101)], 0),
                                         ([(-1, 5)], 0), ([(0, 4), (4, 8), (8, 12), (11, 12)], 3)])
def test_bad_ranges_are_refused(seg, ranges, bad):
    _load(seg, SC.world(100, 1, 1), 1)
    with pytest.raises(_lib.SegmentorError) as e:
        seg.sample_stats(ranges)
    assert e.value.code == _lib.E_ARG and ('range %d ' % bad) in e.value.msg


def test_needs_rows():
    with _lib.Segmenter(0) as s:
        with pytest.raises(_lib.SegmentorError) as e:
            s.sample_stats([(0, 1)])
        assert e.value.code == _lib.E_STATE


# ---- the two commands end to end, against what the reference printed ----
@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'stats_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def cli_world(tmp_path_factory):
    td = str(tmp_path_factory.mktemp('stats_world'))
    world = SC.golden_world(td)
    with open(op.join(ROOT, 'tests', 'golden', 'block_cases.json')) as f:
        tables = json.load(f)['tables']
    for name, rows in (('nice', tables['nice']['rows']), ('ragged', tables['ragged']['rows']),
                       ('short', [r for r in tables['nice']['rows'] if r[4] - r[3] < 1000])):
        with open(op.join(td, name + '.bed'), 'w') as f:
            for c, s, e, a, b in rows:
                f.write('%s\t%d\t%d\t%s\t%s\n' % (c, s, e, 'NA' if a is None else a, 'NA' if b is None else b))
    with open(op.join(td, 'regions.bed'), 'w') as f:
        f.write(SC.golden_bed(world))
    return td, world


def _run(cli_world, capsys, cmd, args):
    from wgbs_tools_amd import wgbs_tools
    td, world = cli_world
    argv = [op.join(td, a) if a.endswith(('beta', '.bed')) else a for a in args]
    rc = wgbs_tools.main(['wgbstools', cmd] + argv + ['--genome', world['ref']])
    return rc, capsys.readouterr().out


CLI_CASES = ['beta_cov_L_nice', 'beta_cov_L_nice_lbeta', 'beta_cov_L_ragged', 'beta_cov_lbeta', 'beta_cov_one_site', 'beta_cov_region',
             'beta_cov_sites', 'beta_cov_sites_lbeta', 'beta_cov_whole', 'beta_stats_L', 'beta_stats_lbeta', 'beta_stats_long_names',
             'beta_stats_long_width60', 'beta_stats_region', 'beta_stats_sites', 'beta_stats_sites_lbeta', 'beta_stats_whole',
             'beta_stats_width60']


def test_every_golden_case_is_run(golden):
    assert sorted(golden['cases']) == CLI_CASES


@pytest.mark.parametrize('name', CLI_CASES)
def test_cli_matches_reference(name, golden, cli_world, capsys):
    rec = golden['cases'][name]
    rc, out = _run(cli_world, capsys, rec['cmd'], rec['args'])
    assert rc == 0
    assert out == rec['stdout'], name


def test_cli_in_pieces_and_mixed_widths(cli_world, capsys, golden, monkeypatch):
    """files that cannot be resident together (a byte budget of one file; uint8 and uint16 files in one call) give the lines of the
    separate calls, in argument order"""
    from wgbs_tools_amd import beta_cov
    monkeypatch.setattr(beta_cov, 'PIECE_BYTES', 2 * SC.GOLDEN_SITES)
    rec = golden['cases']['beta_cov_whole']
    rc, out = _run(cli_world, capsys, 'beta_cov', rec['args'])
    assert rc == 0 and out == rec['stdout']
    monkeypatch.undo()
    a, b = golden['cases']['beta_cov_whole']['stdout'].splitlines(True), golden['cases']['beta_cov_lbeta']['stdout'].splitlines(True)
    rc, out = _run(cli_world, capsys, 'beta_cov', ['smp0.beta', 'smp0.lbeta', 'smp1.beta', 'smp1.lbeta'])
    assert rc == 0 and out == a[0] + b[0] + a[1] + b[1]


def test_cli_empty_selection(cli_world, capsys, tmp_path):
    td, world = cli_world
    empty = str(tmp_path / 'empty.beta')
    open(empty, 'wb').close()
    for cmd in ('beta_cov', 'beta_stats'):
        with pytest.raises(AssertionError, match='Data table is empty!'):
            _run(cli_world, capsys, cmd, [empty])
    short = str(tmp_path / 'short.beta')
    np.zeros(200, dtype=np.uint8).tofile(short)
    with pytest.raises(AssertionError, match='Data table is empty!'):
        _run(cli_world, capsys, 'beta_cov', [short, '-s', '5000-5100'])
    nothing = str(tmp_path / 'nothing.bed')
    with open(nothing, 'w') as f:
        f.write('chr1\t1\t2\nchr9\t1\t100000\n')
    with pytest.raises(AssertionError, match='Data table is empty!'):
        _run(cli_world, capsys, 'beta_stats', ['smp0.beta', '-L', nothing])
