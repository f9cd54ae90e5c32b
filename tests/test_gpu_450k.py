"""`wgbstools beta_to_450k` on the GPU (k_site_gather, k_site_len, k_bed_scan, k_site_emit behind wgbsseg_site_counts and
wgbsseg_site_table): every case of tests/array_cases.py through the command line against what the reference printed
(tests/golden/array_cases.json) — bytes or sha1, the warnings on stderr, the refusal; site_counts against numpy's fancy indexing;
site_table against tests/array_ref.py over shapes whose rows straddle workgroups of fields, in three and more slabs and the
default, with labels of 0, 1 and the most bytes, on the every-pair and the ties worlds; bit-identical repeats; the refusals by
code and word; a closed pipe with slabs in flight and the next call on the same context."""
import errno
import json
import os
import os.path as op

import numpy as np
import pytest

import array_cases as AC
import array_ref as AR
from test_450k_cpu import check_against
from wgbs_tools_amd import _lib, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))
CASES = AC.cases()
COLS = (1, 2, 33, 65)
ROWS = (0, 1, 257, 1000)


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'array_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def worlds():
    return AC.worlds()


@pytest.fixture(scope='module')
def where(tmp_path_factory, worlds):
    td = str(tmp_path_factory.mktemp('array'))
    return {name: AC.write_world(td, name, w) for name, w in worlds.items()}


@pytest.fixture(scope='module')
def seg():
    with _lib.Segmenter(0) as s:
        yield s


@pytest.fixture(scope='module')
def resident(seg, worlds):
    """loads the 65 samples of the small world, .beta (elem 1) or .lbeta (elem 2), once per switch -> their rows"""
    state = {}

    def load(elem):
        rows = worlds['small']['samples'][elem]
        if state.get('elem') != elem:
            (seg.set_lbetas if elem == 2 else seg.set_betas)(rows)
            state['elem'] = elem
        return rows
    return load


def _site_orders(n):
    """name -> n sites of the small world: ascending, descending, with repeats, random"""
    rng = np.random.default_rng([AC.SEED, n])
    up = np.sort(rng.choice(AC.SMALL_SITES, n, replace=False)) if n else np.zeros(0, dtype=np.int64)
    rep = rng.integers(0, 5, n) * 599 if n else up
    return {'ascending': up, 'descending': up[::-1].copy(), 'repeated': rep, 'random': rng.integers(0, AC.SMALL_SITES, n)}


def _emit(seg, tmp_path, site0, samples, labels, **kw):
    """Segmenter.site_table into a file -> (its bytes, lines, bytes reported)"""
    path = str(tmp_path / 'out.csv')
    fd = os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    try:
        lines, nbytes = seg.site_table(fd, site0, samples, labels, **kw)
    finally:
        os.close(fd)
    with open(path, 'rb') as f:
        return f.read(), lines, nbytes


def _labels(n, kind='cg'):
    lim = _lib.site_table_limits()['max_label']
    if kind == 'cg':
        return [b'cg%08d' % i for i in range(n)]
    return [(b'', b'x', b'L' * lim, b'"a,""b"""')[i % 4] for i in range(n)]          # 0, 1 and the most bytes; quotes as the host hands them over


# ---- the command line against the reference's text ----
@pytest.mark.parametrize('name', sorted(CASES))
def test_cli_equals_the_reference(name, golden, where, tmp_path, capfd):
    case, entry = CASES[name], golden['cases'][name]
    d = where[case['world']]
    out = str(tmp_path / 'out.csv')
    rc = wgbs_tools.main(['wgbstools', 'beta_to_450k'] + AC.argv_of(case, where, out))
    said = capfd.readouterr().err.replace(d['map'], AR.MAP)
    want = entry['stderr'] + ('Invalid input argument\n' + entry['error'] + '\n' if 'error' in entry else '')
    # the command says exactly that, in one piece; what else is on stderr (the GPU runtime's own remarks) is no warning of the command's
    assert want in said and '[wt' not in said.replace(want, '', 1) and 'WARNING' not in said.replace(want, '', 1)
    if 'error' in entry:
        assert rc == 1 and not op.exists(out)
        return
    assert rc == 0
    with open(out, 'rb') as f:
        check_against(entry, f.read(), name)


def test_stdout_is_the_default(where, capfd):
    d = where['small']
    ref = op.join(d['dir'], 'ref_quoted.csv')
    assert wgbs_tools.main(['wgbstools', 'beta_to_450k', op.join(d['dir'], 's03.beta'), op.join(d['dir'], 's04.beta'), '--genome', d['ref'], '--ref', ref, '-@', '3']) == 0
    got = capfd.readouterr().out
    assert got.startswith('ilmn,s03,s04\n') and '"cg,0000comma",' in got and got.count('\n') == 5


# ---- the ABI: site_counts ----
@pytest.mark.parametrize('elem', [1, 2])
@pytest.mark.parametrize('n_cols', COLS)
def test_site_counts_equal_fancy_indexing(seg, resident, elem, n_cols):
    rows = resident(elem)
    rng = np.random.default_rng([AC.SEED, elem, n_cols])
    samples = rng.permutation(AC.MAX_SAMPLES)[:n_cols] if n_cols < AC.MAX_SAMPLES else np.arange(AC.MAX_SAMPLES)[::-1]
    for n_rows in ROWS:
        for order, site0 in _site_orders(n_rows).items():
            got = seg.site_counts(site0, samples)
            want = np.stack([rows[s][site0] for s in samples], axis=1) if n_rows else np.zeros((0, n_cols, 2), dtype=np.uint16)
            assert got.shape == (n_rows, n_cols, 2) and got.dtype == np.uint16 and np.array_equal(got, want), (order, n_rows)
    assert np.array_equal(seg.site_counts([5, 5, 0], [2, 2])[:, 0], seg.site_counts([5, 5, 0], [2, 2])[:, 1])       # a sample twice


# ---- the ABI: site_table ----
@pytest.mark.parametrize('elem', [1, 2])
@pytest.mark.parametrize('n_cols', COLS)
def test_site_table_equals_the_restatement(seg, resident, tmp_path, elem, n_cols):
    rows = resident(elem)
    samples = np.arange(n_cols)[::-1]
    cols = [rows[s] for s in samples]
    for n_rows in ROWS:
        labels = _labels(n_rows)
        for order, site0 in _site_orders(n_rows).items():
            min_cov = {'ascending': 3, 'descending': 0, 'repeated': 1, 'random': 300}[order]
            want = AR.table_body([x.decode() for x in labels], site0, cols, min_cov)
            slabs = (0,) if n_rows < 3 else (0, n_rows // 3, 100 if order == 'random' else n_rows // 4)
            for slab_rows in slabs:
                assert slab_rows == 0 or -(-n_rows // slab_rows) >= 3
                got, lines, nbytes = _emit(seg, tmp_path, site0, samples, labels, min_cov=min_cov, slab_rows=slab_rows)
                assert got == want, (order, n_rows, slab_rows)
                assert (lines, nbytes) == (n_rows, len(want))
                g, l, e = seg.site_table_pass_ms()
                assert min(g, l, e) >= 0.0 and abs(g + l + e - seg.last_block_sums_ms()) < 1e-9


def test_labels_of_no_one_and_the_most_bytes(seg, resident, tmp_path):
    rows = resident(1)
    site0 = _site_orders(1000)['random']
    labels = _labels(1000, 'mixed')
    assert {len(x) for x in labels} == {0, 1, 63, 9}
    want = AR.table_body([x.decode() for x in labels], site0, rows[:2], 3)
    for slab_rows in (0, 7, 333):
        assert _emit(seg, tmp_path, site0, [0, 1], labels, slab_rows=slab_rows) == (want, 1000, len(want))
    # the longest fields a workgroup can meet: one column, so every other field is a label of the most bytes
    full = [b'L' * 63] * 600
    want = AR.table_body([x.decode() for x in full], site0[:600], rows[:1], 70000)
    assert _emit(seg, tmp_path, site0[:600], [0], full, min_cov=70000)[0] == want and len(want) == 600 * 67


@pytest.mark.parametrize('world,min_covs', [('every_pair', (0, 1, 3)), ('ties', (0, 1))])
def test_every_pair_and_the_ties(worlds, tmp_path, world, min_covs):
    (elem, (rows,)), = worlds[world]['samples'].items()
    with _lib.Segmenter(0) as s:
        (s.set_lbetas if elem == 2 else s.set_betas)([rows])
        n = len(rows)
        labels = _labels(n)
        site0 = np.arange(n)
        for min_cov in min_covs:
            want = AR.table_body([x.decode() for x in labels], site0, [rows], min_cov)
            a = _emit(s, tmp_path, site0, [0], labels, min_cov=min_cov)
            assert a == (want, n, len(want)), min_cov
        assert _emit(s, tmp_path, site0, [0], labels, min_cov=min_covs[-1]) == a                      # a repeat: identical bytes
        assert _emit(s, tmp_path, site0, [0], labels, min_cov=min_covs[-1], slab_rows=4099) == a


# ---- refusals ----
def test_refusals(worlds, tmp_path):
    lim = _lib.site_table_limits()
    assert lim == dict(default_slab_rows=1 << 16, max_slab_rows=1 << 22, max_label=63, max_cols=4096)
    fd = os.open(str(tmp_path / 'never.csv'), os.O_WRONLY | os.O_CREAT, 0o644)
    try:
        with _lib.Segmenter(0) as s:
            for call in (lambda: s.site_counts([0], [0]), lambda: s.site_table(fd, [0], [0], [b'a'])):
                with pytest.raises(_lib.SegmentorError) as e:
                    call()
                assert e.value.code == _lib.E_STATE and 'betas not set' in e.value.msg
            s.set_betas(worlds['small']['samples'][1][:2])
            ok = dict(site0=[0, 2999, 5], samples=[0, 1], labels=[b'a', b'', b'c'])
            for kw, word in ((dict(samples=[0, 2]), 'column 1: sample 2 is outside the 2 resident samples'), (dict(samples=[-1]), 'column 0: sample -1'),
                             (dict(samples=[]), 'n_cols = 0 is outside 1 .. 4096'), (dict(samples=[0] * 4097), 'n_cols = 4097'),
                             (dict(site0=[0, 3000, 5]), 'row 1: site 3000 is outside the 3000 resident sites'), (dict(site0=[0, 1, -1]), 'row 2: site -1'),
                             (dict(min_cov=-1), 'min_cov = -1 is negative'), (dict(labels=[b'a', b'L' * 64, b'c']), 'the label of row 1 has 64 bytes, at most 63'),
                             (dict(slab_rows=-5), 'slab_rows = -5'), (dict(slab_rows=(1 << 22) + 1), 'slab_rows = 4194305')):
                args = dict(ok)
                args.update(kw)
                with pytest.raises(_lib.SegmentorError) as e:
                    s.site_table(fd, **args)
                assert e.value.code == _lib.E_ARG and word in e.value.msg and e.value.msg.startswith('site_table: '), (kw, e.value.msg)
            for kw, word in ((dict(samples=[2]), 'site_counts: column 0: sample 2'), (dict(site0=[3000]), 'site_counts: row 0: site 3000'), (dict(samples=[]), 'site_counts: n_cols = 0')):
                args = dict(site0=[0], samples=[0])
                args.update(kw)
                with pytest.raises(_lib.SegmentorError) as e:
                    s.site_counts(**args)
                assert e.value.code == _lib.E_ARG and word in e.value.msg, (kw, e.value.msg)
            # what the binding cannot get wrong on its own: NULL pointers and a label_off that descends, through the raw call
            import ctypes as C
            site0, cols, off = np.array([0, 1], dtype=np.int64), np.array([0], dtype=np.int32), np.array([0, 2, 1], dtype=np.int64)
            opts = _lib.SiteTableOpts(3, 0, 0)
            err = C.create_string_buffer(512)
            raw = lambda *a: s._L.wgbsseg_site_table(s._h, *a, fd, None, None, err, 512)
            for argv, word in (((site0.ctypes.data, 2, cols.ctypes.data, 1, b'abc', off.ctypes.data, C.byref(opts)), 'label_off[2] = 1 descends'),
                               ((None, 2, cols.ctypes.data, 1, b'abc', off.ctypes.data, C.byref(opts)), 'site0 is NULL'),
                               ((site0.ctypes.data, 2, None, 1, b'abc', off.ctypes.data, C.byref(opts)), 'samples is NULL'),
                               ((site0.ctypes.data, 2, cols.ctypes.data, 1, b'abc', None, C.byref(opts)), 'label_off is NULL'),
                               ((site0.ctypes.data, 2, cols.ctypes.data, 1, b'abc', off.ctypes.data, None), 'opts is NULL'),
                               ((site0.ctypes.data, -1, cols.ctypes.data, 1, b'abc', off.ctypes.data, C.byref(opts)), 'n_rows = -1 is negative')):
                assert raw(*argv) == _lib.E_ARG and word in err.value.decode(), word
            assert s._L.wgbsseg_site_counts(s._h, site0.ctypes.data, 2, cols.ctypes.data, 1, None, err, 512) == _lib.E_ARG and 'out is NULL' in err.value.decode()
            assert s.site_table(fd, [], [0, 1], []) == (0, 0)
        assert os.fstat(fd).st_size == 0
    finally:
        os.close(fd)


def test_a_closed_pipe_with_slabs_in_flight_leaves_the_context_usable(seg, resident, tmp_path):
    """slabs of 100 rows: when the write of slab 0 fails, the text of slab 1 and the counts and lengths of slab 2 are queued; they
    land in buffers the context keeps, and the next call on the same context writes what a single-slab call writes"""
    rows = resident(1)
    site0 = _site_orders(1000)['random']
    labels = _labels(1000)
    r, wr = os.pipe()
    os.close(r)
    try:
        with pytest.raises(BrokenPipeError) as e:
            seg.site_table(wr, site0, [0, 1, 2], labels, slab_rows=100)
        assert e.value.errno == errno.EPIPE
    finally:
        os.close(wr)
    want = AR.table_body([x.decode() for x in labels], site0, rows[:3], 3)
    assert _emit(seg, tmp_path, site0, [0, 1, 2], labels, slab_rows=100) == (want, 1000, len(want))
    assert np.array_equal(seg.site_counts(site0, [2]), rows[2][site0][:, None])
