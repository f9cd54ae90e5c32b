"""`wgbstools merge` on the GPU.  The view engine over several files (wgbsseg_patview_next_file): a file that begins below where the one
before ended, a last line without its newline, equal lines in different files and on both sides of a file boundary that is a tile
boundary, several sort runs and merge passes with buffers that grow across a boundary, the cut flags, the whole genome, text and BGZF
mixed, the refusals with file and offset, BGZF out — byte for byte against tests/merge_ref.py and the goldens of the reference's tools.
k_beta_merge (wgbsseg_merge_rows) against the numpy restatement, exact: sizes around the vector width, the whole saturated domain of two
files, uint16 rows, meth > cov, borrowed rows at a tight, poisoned pitch, a row named twice, the refusals.  The command end to end."""
import ctypes as C
import gzip
import json
import os.path as op

import numpy as np
import pytest

import borrowed_rows as BW
import merge_cases as MC
import merge_ref as MR
from wgbs_tools_amd import _lib, homog, view, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))
RUN = 512                                                          # csrc/view_plan.h WG_VIEW_RUN
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'merge_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def genome(tmp_path_factory):
    return MC.genome_dir(str(tmp_path_factory.mktemp('merge_genome')))[0]


@pytest.fixture(scope='module')
def seg():
    with _lib.Segmenter(0) as s:
        yield s


def bgzf_bytes(text, member=3000):
    return b''.join(homog._bgzf_member(text[p:p + member]) for p in range(0, len(text), member)) + homog._bgzf_member(b'')


def run_files(files, s, e, how=None, next_file=True, initial_records=0, deflate=False, info=None, **flags):
    """the device's output for the texts `files` fed to ONE engine, next_file() between two of them; how[k]: 'text' (the text must end
    with a newline) or 'bgzf'; info: a dict that receives PatView.info()"""
    how = how or ['text'] * len(files)
    with _lib.PatView(s, e, sort=True, initial_records=initial_records, **flags) as v:
        for k, text in enumerate(files):
            if k and next_file:
                v.next_file()
            if how[k] == 'bgzf':
                data = bgzf_bytes(text)
                assert v.feed_bgzf(data) == len(data)
            else:
                v.feed(text)
        lines, nbytes = v.finish(deflate=deflate)
        out = v.read()
        assert len(out) == nbytes and (deflate or out.count(b'\n') == lines)
        if info is not None:
            info.update(v.info(), lines=lines)
        return out


def passes_of(n):
    runs, k = -(-n // RUN), 0
    while runs > 1:
        runs, k = (runs + 1) // 2, k + 1
    return k


def case(name, golden):
    rec = golden[name]
    return MC.case_files(MC.PAT_CASES[name]), rec['sites'], MC.flag_kwargs(rec['flags']), rec['stdout'].encode()


# ---- the engine over several files ----
def test_second_file_begins_below_the_first_ones_end(golden):
    files, (s, e), kw, want = case('tiny_overlap', golden)
    assert MR.merge_pats(files, s, e, **kw) == want
    assert run_files(files, s, e, **kw) == want
    assert run_files(files[::-1], s, e, **kw) == want                 # the order of the files does not show: counts only are summed
    with pytest.raises(_lib.SegmentorError, match='failed in view: the pat file is not sorted'):
        run_files(files, s, e, next_file=False, **kw)                 # one file's text would be refused as descending


def test_last_line_without_its_newline(golden, tmp_path):
    files, (s, e), kw, want = case('tiny_no_newline', golden)
    assert not files[0].endswith(b'\n')
    assert run_files(files, s, e, how=['bgzf', 'bgzf'], **kw) == want
    assert run_files(files, s, e, how=['bgzf', 'text'], **kw) == want
    with pytest.raises(_lib.SegmentorError, match='failed in view: invalid line'):
        run_files(files, s, e, how=['bgzf', 'bgzf'], next_file=False, **kw)       # the line glues to the next file's first
    paths = []
    for k, text in enumerate(files):                                  # as text: plain gzip files, inflated on the host
        paths.append(str(tmp_path / ('f%d.pat.gz' % k)))
        with gzip.open(paths[-1], 'wb') as f:
            f.write(text)
    got = []
    assert view.view_pats(paths, s, e, got.append, sort=True, **kw)[0] == want.count(b'\n')
    assert b''.join(got) == want


def test_equal_lines_in_different_files_are_summed():
    a = b'chr1\t5\tCT\t2\nchr1\t9\tC\t1\n'
    b = b'chr1\t5\tCT\t3\nchr1\t5\tCTT\t1\n'
    c = b'chr1\t2\tT\t1\nchr1\t5\tCT\t10\nchr2\t5\tCT\t1\n'
    want = b'chr1\t2\tT\t1\nchr1\t5\tCT\t15\nchr2\t5\tCT\t1\nchr1\t5\tCTT\t1\nchr1\t9\tC\t1\n'
    assert MR.merge_pats([a, b, c], 1, 100) == want
    assert run_files([a, b, c], 1, 100) == want
    assert run_files([a, b'', b, b'\n', c], 1, 100) == want           # empty files between


def test_equal_lines_on_both_sides_of_a_file_and_tile_boundary():
    same = b'chr1\t5\tCCT\t1\n'
    first = same * 100 + b'chr1\t5\tCCTT\t1\n' + same * 214             # 315 lines, one a byte longer: 4096 bytes, the last line is `same`
    assert len(first) == 4096 and first.endswith(same)
    second = same * 3 + b'chr1\t6\tT\t2\n'
    want = b'chr1\t5\tCCT\t317\nchr1\t5\tCCTT\t1\nchr1\t6\tT\t2\n'
    assert MR.merge_pats([first, second], 1, 100) == want
    assert run_files([first, second], 1, 100) == want
    assert run_files([first, second], 1, 100, how=['bgzf', 'text']) == want


def test_three_files_several_runs_and_growth_across_a_boundary(golden):
    files, (s, e), kw, want = case('wg_three', golden)
    n = sum(f.count(b'\n') for f in files)
    assert n == 1200 and passes_of(n) >= 2
    info = {}
    assert run_files(files, s, e, initial_records=8, info=info, **kw) == want == MR.merge_pats(files, s, e, **kw)
    assert info['records'] == n and info['order'] == 2 and info['merge_passes'] == passes_of(n)
    assert info['grown_records'] >= 2 and info['grown_arena'] >= 2     # the second file's chunk needs more than the first one's left
    assert run_files(files, s, e, how=['text', 'bgzf', 'text'], **kw) == want


@pytest.mark.parametrize('name', ['sites_two', 'sites_strict_strip_min3', 'region_two', 'wg_two'])
def test_goldens_through_the_engine(name, golden):
    files, (s, e), kw, want = case(name, golden)
    assert run_files(files, s, e, **kw) == want
    assert run_files(files, s, e, how=['bgzf'] * len(files), initial_records=8, **kw) == want


def test_text_and_bgzf_mixed_through_the_feed(golden, tmp_path):
    """view.view_pats with --inflate device: a BGZF file is inflated on the GPU, a plain gzip file falls back to the host's text feed"""
    files, (s, e), kw, want = case('sites_two', golden)
    a, b = str(tmp_path / 'a.pat.gz'), str(tmp_path / 'b.pat.gz')
    with gzip.open(a, 'wb') as f:
        f.write(files[0])
    homog.write_bgzf(b, files[1], 1)
    for order in ([a, b], [b, a]):
        got = []
        view.view_pats(order, s, e, got.append, sort=True, inflate='device', **kw)
        assert b''.join(got) == want


def _refusal(files, **kw):
    with pytest.raises(_lib.SegmentorError) as err:
        run_files(files, 1, 5000, **kw)
    assert err.value.code == _lib.E_ARG
    return err.value.msg


def test_refusals_name_the_file_and_the_offset_inside_it():
    first = b''.join(b'chr1\t%d\tCCTT\t1\n' % (10 + i) for i in range(40))
    good = b''.join(b'chr1\t%d\tCT\t2\n' % (3 + i) for i in range(25))
    tail = b'chr1\t900\tC\t1\n'
    for how in (['text', 'text'], ['bgzf', 'bgzf'], ['text', 'bgzf']):
        msg = _refusal([first, good + b'chr1\t905\tCT\n' + tail], how=how)
        assert msg.startswith('failed in view: file 1: invalid line at byte offset %d of the file' % len(good)), msg
        msg = _refusal([first, good + b'chr1\t20\tC\t1\n' + tail], how=how)
        assert msg.startswith('failed in view: file 1: the pat file is not sorted: the read at byte offset %d of the file' % len(good)), msg
        for low in (b'0', b'-3'):
            assert _refusal([first, good + b'chr1\t30\tCT\t' + low + b'\n' + tail], how=how) == 'failed in view: file 1: count < 1 at byte %d' % len(good)
    assert _refusal([first + b'chr1\t60\tC\t0\n', good]) == 'failed in view: file 0: count < 1 at byte %d' % len(first)
    assert _refusal([first, b'', good + b'chr1\t1\tC\t1\n']).startswith('failed in view: file 2: the pat file is not sorted: the read at byte offset %d ' % len(good))
    # one file: nothing changes — a count below 1 is summed, and the messages are view's
    assert run_files([b'chr1\t7\tC\t3\nchr1\t7\tC\t-1\n'], 1, 100) == b'chr1\t7\tC\t2\n'
    assert 'byte offset %d of the input' % len(good) in _refusal([good + b'chr1\t905\tCT\n'])
    # BGZF bytes left over, and a call after finish()
    with _lib.PatView(1, 100, sort=True) as v:
        data = bgzf_bytes(good)
        assert v.feed_bgzf(data[:-7]) < len(data) - 7
        with pytest.raises(_lib.SegmentorError, match='failed in view: file 0: truncated'):
            v.next_file()
    with _lib.PatView(1, 100, sort=True) as v:
        v.feed(good)
        v.finish()
        with pytest.raises(_lib.SegmentorError, match=r'finish\(\) has been called') as err:
            v.next_file()
        assert err.value.code == _lib.E_STATE


def test_deflate_on_the_device(golden):
    files, (s, e), kw, want = case('wg_two', golden)
    packed = run_files(files, s, e, deflate=True, **kw)
    assert packed.endswith(BGZF_EOF) and packed[:4] == b'\x1f\x8b\x08\x04' and gzip.decompress(packed) == want


# ---- k_beta_merge ----
def _merge(seg, rows, samples=None, lbeta=False):
    wide = rows[0].dtype == np.uint16
    (seg.set_lbetas if wide else seg.set_betas)(rows)
    return seg.merge_rows(list(range(len(rows))) if samples is None else samples, lbeta=lbeta)


def _rows(rng, n, n_rows, wide=False, lo=0):
    top = 65536 if wide else 256
    return [rng.integers(lo, top, (n, 2)).astype(np.uint16 if wide else np.uint8) for _ in range(n_rows)]


@pytest.mark.parametrize('n_rows', [2, 3, 33])
def test_merge_rows_sizes(seg, n_rows):
    rng = np.random.default_rng(20261121 + n_rows)
    for n in (1, 7, 8, 9, 4099):
        rows = _rows(rng, n, n_rows)
        for lbeta in (False, True):
            got = _merge(seg, rows, lbeta=lbeta)
            want = MR.merge_betas(rows, lbeta=lbeta)
            assert got.dtype == want.dtype and np.array_equal(got, want), (n, n_rows, lbeta)
        wide = _rows(rng, n, n_rows, wide=True)
        for lbeta in (False, True):
            assert np.array_equal(_merge(seg, wide, lbeta=lbeta), MR.merge_betas(wide, lbeta=lbeta)), (n, n_rows, lbeta, 'uint16 rows')
    assert seg.last_merge_rows_ms() > 0.0


@pytest.mark.parametrize('name', sorted(MC.BETA_CASES))
def test_merge_rows_goldens(seg, name, golden):
    import hashlib
    rec = golden[name]
    got = _merge(seg, MC.BETA_CASES[name]['rows'](), lbeta=rec['lbeta'])
    assert str(got.dtype) == rec['dtype'] and hashlib.sha1(got.tobytes()).hexdigest() == rec['out_sha1']


def test_whole_saturated_domain_of_two_files(seg):
    rows = MC.saturated_domain()
    want = MR.merge_betas(rows)
    assert (want[:, 1] == 255).all() and want[:, 0].max() == 255
    assert np.array_equal(_merge(seg, rows), want)


def test_uint16_rows_saturated(seg):
    rng = np.random.default_rng(20261122)
    n = 1 << 20
    cov = rng.integers(32768, 65536, (2, n))
    meth = (rng.random((2, n)) * (cov + 1)).astype(np.int64)
    rows = [np.concatenate([np.stack([meth[k], cov[k]], axis=1).astype(np.uint16), MC.wide_corners()[k]]) for k in range(2)]
    want = MR.merge_betas(rows, lbeta=True)
    assert (want[:, 1] == 65535).all()                                # every site saturates
    assert want[-8:].tolist() == [[0, 65535], [0, 65535], [65534, 65535], [65535, 65535], [0, 65535], [0, 65535], [65534, 65535], [65535, 65535]]
    assert np.array_equal(_merge(seg, rows, lbeta=True), want)


def test_uint8_rows_into_lbeta_nothing_saturates(seg):
    rng = np.random.default_rng(20261123)
    rows = _rows(rng, 4099, 33, lo=200)
    want = np.sum([r.astype(np.int64) for r in rows], axis=0)
    assert want.max() > 255 * 28 and want.max() <= 65535
    got = _merge(seg, rows, lbeta=True)
    assert got.dtype == np.uint16 and np.array_equal(got, want) and np.array_equal(got, MR.merge_betas(rows, lbeta=True))


def test_meth_above_cov_wraps(seg):
    n = 1000
    rows = [np.stack([np.full(n, 255), np.arange(n) % 120], axis=1).astype(np.uint8) for _ in range(3)]
    want = MR.merge_betas(rows)
    assert want[1].tolist() == [765 % 256, 3] and want[100].tolist() == [int(765 / 300 * 255) % 256, 255]
    assert np.array_equal(_merge(seg, rows), want)


@pytest.mark.parametrize('poison', BW.ROW_POISONS)
def test_borrowed_rows_at_a_tight_poisoned_pitch(seg, poison):
    rng = np.random.default_rng(20261124)
    for n in (9, 4099):                                               # pitch 32 / 8208: 14 / 10 bytes of poison behind every row
        rows = _rows(rng, n, 3)
        b = BW.BorrowedRows(rows, poison, DEV, seed=n)
        assert b.pitch - 2 * n in (14, 10)
        seg.set_betas_device(b.ptr, 3, b.pitch, n, keepalive=b)
        for lbeta in (False, True):
            assert np.array_equal(seg.merge_rows([0, 1, 2], lbeta=lbeta), MR.merge_betas(rows, lbeta=lbeta)), (n, poison, lbeta)
        b.assert_untouched()


def test_a_row_named_twice_and_the_refusals(seg):
    rng = np.random.default_rng(20261125)
    rows = _rows(rng, 515, 3)
    seg.set_betas(rows)
    assert np.array_equal(seg.merge_rows([2, 0, 2, 2]), MR.merge_betas([rows[2], rows[0], rows[2], rows[2]]))
    assert np.array_equal(seg.merge_rows([1]), rows[1])               # one row: nothing saturates, nothing changes
    for samples, what in (([], 'merge_rows: 0 rows named'), ([0, 3], 'merge_rows: no row 3 \\(3 are resident\\)'), ([-1], 'merge_rows: no row -1')):
        with pytest.raises(_lib.SegmentorError, match=what) as err:
            seg.merge_rows(samples)
        assert err.value.code == _lib.E_ARG
    idx = np.array([0, 1], dtype=np.int32)
    buf = C.create_string_buffer(512)
    assert seg._L.wgbsseg_merge_rows(seg._h, idx.ctypes.data, 2, 0, None, buf, 512) == _lib.E_ARG and buf.value == b'merge_rows: out is NULL'
    with _lib.Segmenter(0) as fresh:
        with pytest.raises(_lib.SegmentorError, match='betas not set'):
            fresh.merge_rows([0])


# ---- the command end to end ----
def test_cli_pat(golden, genome, tmp_path, capfd):
    files, _, _, want = case('tiny_overlap', golden)
    a, b = str(tmp_path / 'a.pat.gz'), str(tmp_path / 'b.pat.gz')
    homog.write_bgzf(a, files[0], 1)
    homog.write_bgzf(b, files[1], 1)
    pre = str(tmp_path / 'out')
    argv = ['wgbstools', 'merge', a, b, '-p', pre, '--genome', genome] + golden['tiny_overlap']['where']
    assert wgbs_tools.main(argv + ['--no_sort', '-np']) == 0
    err = capfd.readouterr().err
    assert '--no_sort, -np: accepted and without effect' in err and 'no .csi index is written' in err
    with open(pre + '.pat.gz', 'rb') as f:
        data = f.read()
    assert data.endswith(BGZF_EOF) and gzip.decompress(data) == want
    assert wgbs_tools.main(argv) == 0 and 'already exists. Skipping it.' in capfd.readouterr().err
    assert wgbs_tools.main(argv + ['-f', '--inflate', 'device']) == 0
    with open(pre + '.pat.gz', 'rb') as f:
        assert gzip.decompress(f.read()) == want
    homog.write_bgzf(b, files[1] + b'chr1\t50\tC\t0\n', 1)
    assert wgbs_tools.main(argv + ['-f']) == 1
    assert f'{b}: failed in view: file 1: count < 1 at byte {len(files[1])}' in capfd.readouterr().err


def test_cli_whole_genome_pat(golden, genome, tmp_path, capfd):
    files, _, _, want = case('wg_two', golden)
    paths = []
    for k, text in enumerate(files):
        paths.append(str(tmp_path / ('w%d.pat.gz' % k)))
        homog.write_bgzf(paths[-1], text, 1)
    assert wgbs_tools.main(['wgbstools', 'merge'] + paths + ['-p', str(tmp_path / 'wg'), '--genome', genome, '--inflate', 'device']) == 0
    capfd.readouterr()
    with open(str(tmp_path / 'wg.pat.gz'), 'rb') as f:
        assert gzip.decompress(f.read()) == want


def test_cli_betas(tmp_path, capfd):
    rows = MC.BETA_CASES['u8_three_4099']['rows']()
    paths = []
    for k, r in enumerate(rows):
        paths.append(str(tmp_path / ('s%d.beta' % k)))
        r.tofile(paths[-1])
    pre = str(tmp_path / 'pool')
    assert wgbs_tools.main(['wgbstools', 'merge'] + paths + ['-p', pre]) == 0
    assert np.array_equal(np.fromfile(pre + '.beta', dtype=np.uint8).reshape(-1, 2), MR.merge_betas(rows))
    assert wgbs_tools.main(['wgbstools', 'merge'] + paths + ['-p', pre, '-l']) == 0
    assert np.array_equal(np.fromfile(pre + '.lbeta', dtype=np.uint16).reshape(-1, 2), MR.merge_betas(rows, lbeta=True))
    wide = []
    for k, r in enumerate(MC.BETA_CASES['u16_two_lbeta']['rows']()):
        wide.append(str(tmp_path / ('w%d.lbeta' % k)))
        r.tofile(wide[-1])
    assert wgbs_tools.main(['wgbstools', 'merge'] + wide + ['-p', str(tmp_path / 'wpool'), '-l']) == 0
    assert np.array_equal(np.fromfile(str(tmp_path / 'wpool.lbeta'), dtype=np.uint16).reshape(-1, 2), MR.merge_betas(MC.BETA_CASES['u16_two_lbeta']['rows'](), lbeta=True))
    capfd.readouterr()
