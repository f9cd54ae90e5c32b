"""`wgbstools compare_betas` without a GPU: the numpy restatement the GPU tests check the kernels against
(tests/compare_ref.py) equals np.histogram2d itself and what the reference's own comp2 drew (tests/golden/compare_cases.json);
the drawing function gives ax.hist2d's mesh; the dispatcher knows the command; the refusals that need no device; the host-only
argument and edge checks (csrc/pair_plan.h) under the sanitizers."""
import json
import os.path as op
import shutil
import subprocess

import numpy as np
import pytest

import compare_cases as CC
import compare_ref as CR

ROOT = op.dirname(op.dirname(op.abspath(__file__)))


def _run_sites():
    """a workgroup's run of sites, from the library (it loads without a device)"""
    from wgbs_tools_amd import _lib
    if not op.isfile(_lib.LIB_PATH):
        from wgbs_tools_amd import build
        build.build()
    return _lib.pair_hist_limits()[1]


def _worlds():
    RUN = _run_sites()
    for elem in (1, 2):
        for n in CC.SIZES:
            yield ('world', n, elem), CC.world(n, 5, elem)
        yield ('bimodal', elem), CC.bimodal(4097, elem)
        yield ('over', elem), CC.over(4097, elem)
        yield ('extremes', elem), CC.extremes(2 * RUN + 3, elem, RUN)


def _same_as_numpy(ra, rb, min_cov, bins, what):
    counts, xe, ye = CR.hist(ra, rb, min_cov, bins)
    x, y = CR.values(ra, rb, min_cov)
    h, hx, hy = np.histogram2d(x, y, bins)
    assert counts.dtype == np.uint64 and np.array_equal(counts, h.astype(np.uint64)), what
    assert xe.tobytes() == hx.tobytes() and ye.tobytes() == hy.tobytes(), what
    assert int(counts.sum()) == CR.pair_range(ra, rb, min_cov)['n'] == x.size


def test_restatement_equals_histogram2d():
    for what, rows in _worlds():
        for a, b in CR.all_pairs(len(rows)):
            for bins in CC.BINS + (126,):
                _same_as_numpy(rows[a], rows[b], 10, bins, (what, a, b, bins))
    rows = CC.world(4097, 5, 2, seed=3)
    for min_cov in (1, 255, 256, 1001):
        for a, b in CR.all_pairs(5):
            _same_as_numpy(rows[a], rows[b], min_cov, 7, (min_cov, a, b))
    for name, (a, b, min_cov, bins) in CC.golden_cases().items():
        _same_as_numpy(a, b, min_cov, bins, name)


def test_restatement_with_given_edges_equals_histogram2d():
    rows = CC.world(4097, 2, 1, seed=6)
    x, y = CR.values(rows[1], rows[0], 3)
    xe = np.array([0.1, 0.11, 0.5, 0.500001, 0.9])
    ye = np.array([-3.0, 0.0, 0.25, 1.0, 1e300])
    h, _, _ = np.histogram2d(x, y, bins=[xe, ye])
    assert np.array_equal(CR.count(x, y, xe, ye), h.astype(np.uint64))


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'compare_cases.json')) as f:
        return json.load(f)['cases']


def test_restatement_equals_what_the_reference_drew(golden):
    cases = CC.golden_cases()
    assert sorted(cases) == sorted(golden)
    for name, (a, b, min_cov, bins) in cases.items():
        rec = golden[name]
        assert (rec['min_cov'], rec['bins'], rec['n_sites']) == (min_cov, bins, a.shape[0]) and bins <= 7 and a.shape[0] <= 200
        counts, xe, ye = CR.hist(a, b, min_cov, bins)
        assert np.array_equal(counts.T, np.array(rec['drawn'], dtype=np.uint64)), name
        assert xe.tobytes() == np.array(rec['xedges']).tobytes() and ye.tobytes() == np.array(rec['yedges']).tobytes(), name
        assert rec['xlim'] == [0.0, 1.0] and rec['ylim'] == [0.0, 1.0]


def _mesh(ax):
    mesh, = ax.collections
    return np.ma.filled(mesh.get_array(), np.nan), np.asarray(mesh.get_coordinates())


def test_drawing_equals_hist2d():
    matplotlib = pytest.importorskip('matplotlib')
    matplotlib.use('Agg')
    import matplotlib.pyplot as plt
    from matplotlib.colors import LogNorm
    from wgbs_tools_amd import compare_betas
    rows = CC.world(200, 5, 1, seed=7)[:4]
    names = ['first', 'a_name_that_is_longer_than_twenty_characters', 'third', 'x' * 40]
    pairs = compare_betas.all_pairs(4)
    assert [tuple(p) for p in pairs] == CR.all_pairs(4)
    bins = 7
    hists = [CR.hist(rows[i], rows[j], 3, bins) for i, j in pairs]
    fig = compare_betas.draw(pairs, [h[0] for h in hists], [h[1] for h in hists], [h[2] for h in hists], names)
    # the reference's way, on the same values
    want, waxs = plt.subplots(4, 4)
    for i, j in pairs:
        x, y = CR.values(rows[i], rows[j], 3)
        waxs[i, j].hist2d(x, y, bins=bins, cmap=plt.cm.jet, norm=LogNorm())
        waxs[i, j].set_ylim(0, 1)
        waxs[i, j].set_xlim(0, 1)
    for i in range(4):
        for j in range(i + 1, 4):
            want.delaxes(waxs[i, j])
    assert len(fig.axes) == len(want.axes) == 10
    for got_ax, want_ax in zip(fig.axes, want.axes):
        ga, gc = _mesh(got_ax)
        wa, wc = _mesh(want_ax)
        assert ga.dtype == wa.dtype and np.array_equal(ga, wa) and gc.tobytes() == wc.tobytes()
        assert got_ax.get_xlim() == want_ax.get_xlim() == (0.0, 1.0) and got_ax.get_ylim() == want_ax.get_ylim() == (0.0, 1.0)
        assert got_ax.get_subplotspec().get_geometry() == want_ax.get_subplotspec().get_geometry()
        assert isinstance(got_ax.collections[0].norm, LogNorm) and got_ax.collections[0].get_cmap().name == 'jet'
    by_place = {ax.get_subplotspec().get_geometry()[2]: ax for ax in fig.axes}
    assert sorted(by_place) == [4 * i + j for i, j in CR.all_pairs(4)]
    assert by_place[4].get_ylabel() == 'a_name_that_is_longe\nr_than_twenty_charac\nters' and by_place[12].get_xlabel() == 'first'
    assert by_place[15].get_xlabel() == 'x' * 20 + '\n' + 'x' * 20
    plt.close(fig)
    plt.close(want)


def test_dispatcher_knows_the_command():
    from wgbs_tools_amd import wgbs_tools
    assert 'compare_betas' in wgbs_tools.COMMANDS and 'compare_betas' not in wgbs_tools.REFERENCE_ONLY


def test_refusals_without_a_device(tmp_path, capsys):
    from wgbs_tools_amd import wgbs_tools
    a, b, c = (str(tmp_path / n) for n in ('a.beta', 'b.beta', 'c.lbeta'))
    np.ones(200, dtype=np.uint8).tofile(a)
    np.ones(202, dtype=np.uint8).tofile(b)
    np.ones(200, dtype=np.uint16).tofile(c)
    for argv, word in (([a], 'at least 2 input files'), ([a, a, '-c', '0'], '--min_cov must be at least 1'), ([a, a, '--bins', '0'], '--bins must be at least 1'),
                       ([a, b], 'files of one length'), ([a, c, b], 'files of one length'), ([a, str(tmp_path / 'none.beta')], 'Invalid beta file')):
        assert wgbs_tools.main(['wgbstools', 'compare_betas'] + argv + ['-o', str(tmp_path / 'out.npz')]) == 1
        assert word in capsys.readouterr().err, argv
    assert not op.exists(str(tmp_path / 'out.npz'))


def test_edges_of_follows_numpy():
    from wgbs_tools_amd import compare_betas
    for v in (np.array([]), np.array([0.25]), np.array([0.25, 0.25]), np.array([0.0, 1.0 / 3, 3.0]), np.array([1.0])):
        for bins in (1, 2, 7, 101):
            lo, hi = (v.min(), v.max()) if v.size else (0.0, 0.0)
            want = np.histogram(v, bins)[1]
            assert compare_betas.edges_of(v.size, float(lo), float(hi), bins).tobytes() == want.tobytes() == CR.axis_edges(v, bins).tobytes()


def _have(flags):
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null'] + flags, input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


@pytest.mark.skipif(not _have(SAN), reason='no g++ with sanitizer runtimes')
def test_pair_checks_under_sanitizers(tmp_path):
    """csrc/pair_plan.h — the argument and edge checks of wgbsseg_pair_ranges / wgbsseg_pair_hist — compiled plain and with
    AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program: both finish clean and print the same lines"""
    outs = []
    for name, flags in (('plain', []), ('asan_ubsan', SAN)):
        exe = str(tmp_path / ('san_pair_' + name))
        r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-I', op.join(ROOT, 'wgbs_tools_amd', 'csrc'), op.join(ROOT, 'tests', 'native', 'san_pair.cpp'), '-o', exe] + flags,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-4000:]
        r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'})
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].splitlines()
    assert lines[0] == 'limits: bins 126 run %d lds 65536' % _run_sites()
    assert sum(l.startswith('refused: ') for l in lines) == 16 and sum(l.startswith('accepted: ') for l in lines) == 6
    for word in ('min_cov = 0', 'n_pairs = 0', 'pair 2 = (1, 5)', 'pair 0 = (-1, 0)', 'pair list is NULL', 'bins = 0', 'bins = 127', 'edges is NULL',
                 'edge 4 of axis 1 of pair 2 is not finite', 'edge 1 of axis 0 of pair 0', 'too many pairs x sites'):
        assert any(word in l for l in lines), word
