"""`wgbstools frag_len` on the GPU (k_frag_hist behind wgbsseg_fraglen_*): every golden case of the reference's tools through the
command line, with BGZF input inflated on the device and with plain gzip; the edges of the text and of the histogram; the tile loop;
chunking; the refusals and their byte offsets; a time-boxed random comparison against the restatement tests/frag_ref.py."""
import gzip
import json
import os
import os.path as op
import time

import numpy as np
import pytest

import frag_cases as FC
import frag_ref as FR
from wgbs_tools_amd import _lib, frag_len, homog, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))
EVERYWHERE = (np.array([1]), np.array([2 ** 31 - 1]))          # one block that holds every read: selection on, nothing dropped


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'frag_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def genome(tmp_path_factory):
    return FC.genome_dir(str(tmp_path_factory.mktemp('frag_genome')))[0]


def bgzf_bytes(text, member=65280):
    return b''.join(homog._bgzf_member(text[p:p + member]) for p in range(0, len(text), member)) + homog._bgzf_member(b'')


def run(text, m, blocks=None, groups=-1, cuts=None, bgzf=False):
    """the device's histogram of `text` as Python integers; cuts: byte offsets (line ends) at which the text is cut into feeds; bgzf:
    fed as BGZF bytes (a text without its last newline must go this way)"""
    s, e = blocks if blocks is not None else (None, None)
    with _lib.FragLen(m, s, e, groups=groups) as h:
        if bgzf:
            data = bgzf_bytes(text, 3000)
            assert h.feed_bgzf(data) == len(data)
        else:
            pos = 0
            for cut in list(cuts or []) + [len(text)]:
                h.feed(text[pos:cut])
                pos = cut
        return h.finish().tolist()


# ---- the reference's lines through the command line ----
@pytest.mark.parametrize('how', ['bgzf_device', 'gzip'])
@pytest.mark.parametrize('name', sorted(FC.CASES))
def test_cli_matches_reference(name, how, golden, genome, tmp_path, capsys):
    rec = golden[name]
    text = FC.case_pat(FC.CASES[name])
    pat = str(tmp_path / 'smp.pat.gz')
    if how == 'gzip':
        with gzip.open(pat, 'wb') as f:
            f.write(text)
    else:
        homog.write_bgzf(pat, text, 4)
    where = list(rec['where'])
    if where[:1] == ['-L']:
        (tmp_path / 'blocks.bed').write_text(where[1])
        where[1] = str(tmp_path / 'blocks.bed')
    argv = ['wgbstools', 'frag_len', pat, '-v', '-m', str(rec['m']), '--genome', genome] + where
    assert wgbs_tools.main(argv + (['--inflate', 'device'] if how == 'bgzf_device' else [])) == 0
    io = capsys.readouterr()
    assert io.out == rec['stdout'], name
    assert io.err.startswith(pat + '\n')
    assert ('[wt frag] Empty list of lengths for ' + pat in io.err) == (rec['stdout'] == '')


def test_several_files_and_a_figure(tmp_path, capsys):
    a, b, c = (str(tmp_path / n) for n in ('a.pat.gz', 'none.pat.gz', 'c.pat.gz'))
    homog.write_bgzf(a, b'chr1\t5\tCCT\t2\n', 1)
    homog.write_bgzf(b, b'', 1)
    with gzip.open(c, 'wb') as f:
        f.write(b'chr1\t5\tCCT\t2\nchr1\t3\tC\t7')                  # (unsorted, and no newline at the end: whole genome takes both)
    out = str(tmp_path / 'figs')
    try:
        import matplotlib                                            # noqa: F401
        drawn = True
    except ImportError:
        drawn = False
    rc = wgbs_tools.main(['wgbstools', 'frag_len', c, b, a, '-v', '-m', '4', '-o', out])
    io = capsys.readouterr()
    if drawn:
        assert rc == 0
        assert io.out == '7 0 2 0\n0 0 2 0\n'
        assert sorted(os.listdir(out)) == ['a.png', 'c.png']
        assert [ln for ln in io.err.splitlines() if ln in (a, b, c)] == [c, b, a]
        assert '[wt frag] Empty list of lengths for ' + b in io.err and '[wt frag] dumping ' + op.join(out, 'c.png') in io.err
    else:
        assert rc == 1 and '-v prints the values and needs no figure' in io.err


# ---- the edges of the text and of the histogram ----
def test_text_edges():
    long_read = b'chr1\t38\t' + b'CT' * 750 + b'\t3\n'               # 1,500 CpGs: longer than the spill behind a tile
    lines = [b'chr1\t%d\t%s\t%d\n' % (10 + i // 7, b'CTH.'[:1 + i % 4] * (1 + i % 5), 1 + i % 9) for i in range(600)]
    text = b'\n\n' + b''.join(lines[:200]) + b'\n' + long_read + b'\n\n\n' + b''.join(lines[200:]) + b'\n'
    assert len(text) > 2 * 4096                                       # lines straddle two tile edges
    for m in (1, 5, 30, FC.LDS_BINS + 5):
        for blocks in (None, EVERYWHERE, (np.array([12, 30, 30]), np.array([20, 90, 45]))):
            want = FR.frag_hist(text, m, blocks)
            assert run(text, m, blocks) == want, (m, blocks)
            assert run(text.rstrip(b'\n'), m, blocks, bgzf=True) == want, (m, blocks)      # a last line without its newline


def test_bins_beyond_lds_and_wide_sums():
    m = FC.LDS_BINS + 5
    reads = [(3, FC.LDS_BINS, 5), (4, FC.LDS_BINS + 1, 7), (4, m - 1, 11), (5, m, 13), (6, 3000, 17), (7, 1, 2 ** 31 - 1), (7, 1, 2 ** 31 - 1),
             (8, 1, 2 ** 31 - 1), (9, 2, -4)]
    text = FC.lines_text(reads)
    got = run(text, m, EVERYWHERE)
    assert got == FR.frag_hist(text, m, EVERYWHERE)
    assert got[0] == 3 * (2 ** 31 - 1) and got[1] == -4               # exact: three such counts overflow 32 bits
    assert got[FC.LDS_BINS - 1:] == [5, 7, 0, 0, 11, 13 + 17]
    assert run(text, 1) == [sum(c for _, _, c in reads)]
    assert run(text, FC.LDS_BINS)[-1] == 5 + 7 + 11 + 13 + 17


def _forty_kb():
    rng = np.random.default_rng(5)
    st = np.sort(rng.integers(1, 900, 2000))
    ln = rng.integers(1, 14, 2000)
    text = b''.join(b'chr1\t%d\t%s\t%d\n' % (st[i], b'C' * ln[i], 1 + i % 30) for i in range(2000))
    assert 9 * 4096 < len(text) <= 10 * 4096                          # ten tiles
    return text


def test_tile_loop():
    text = _forty_kb()
    blocks = FR.cview_order([(str(s), str(s + w)) for s, w in ((5, 40), (100, 30), (100, 250), (300, 3), (420, 100), (421, 20), (800, 50))])
    for b in (None, blocks):
        want = FR.frag_hist(text, 30, b)
        assert run(text, 30, b) == want
        for groups in (1, 3):
            assert run(text, 30, b, groups=groups) == want, groups
    with pytest.raises(_lib.SegmentorError, match='0 workgroups'):
        _lib.FragLen(30, groups=0)


def test_chunking():
    text = _forty_kb()
    blocks = (np.array([50, 300]), np.array([200, 700]))
    one = run(text, 30, blocks)
    assert one == FR.frag_hist(text, 30, blocks)
    rng = np.random.default_rng(3)
    ends = [i + 1 for i, ch in enumerate(text) if ch == 10]
    for _ in range(3):
        cuts = sorted(set(rng.choice(ends, int(rng.integers(1, 12))).tolist()))
        assert run(text, 30, blocks, cuts=cuts) == one, cuts
    with _lib.FragLen(30, *blocks) as h:
        h.feed(b'')
        h.feed(text)
        h.feed(b'')
        assert h.kernel_ms() >= 0
        assert h.inflate_ms() == 0
        assert h.finish().tolist() == one
    with _lib.FragLen(30) as h:
        h.feed(text)
        with pytest.raises(_lib.SegmentorError, match='cannot be mixed'):
            h.feed_bgzf(bgzf_bytes(text))
    with _lib.FragLen(30) as h:
        with pytest.raises(_lib.SegmentorError, match='complete line'):
            h.feed(b'chr1\t5\tCC\t1')


# ---- refusals ----
def _refused(feeds, blocks, pattern):
    s, e = blocks if blocks is not None else (None, None)
    with _lib.FragLen(30, s, e) as h:
        for f in feeds:
            h.feed(f)
        with pytest.raises(_lib.SegmentorError, match=pattern) as err:
            h.finish()
    assert err.value.msg.startswith('failed calculating frag_len:')


def test_descending_reads():
    good = b'chr1\t1\tCCCC\t1\nchr1\t3\tTTTT\t2\n'
    late = b'chr1\t2\tCCC\t1\n'
    # inside a tile
    _refused([good + late], EVERYWHERE, r'not sorted.*byte offset %d of' % len(good))
    # the first line of the second tile against the last line of the first, found by scanning back — over empty lines too
    row = b'chr1\t100\tCCCC\t1\n'
    assert len(row) == 16
    for front in (row * 256, row * 255 + b'\n' * 16, row * 300 + b'\n' * (4096 * 2 - 4800)):
        assert len(front) % 4096 == 0
        _refused([front + b'chr1\t99\tCC\t1\n'], EVERYWHERE, r'not sorted.*byte offset %d of' % len(front))
        assert run(front + b'chr1\t100\tCC\t1\n', 30, EVERYWHERE)[1] == 1           # (equal starts are in order)
    assert run(b'\n' * 4096 + b'chr1\t99\tCC\t1\n', 30, EVERYWHERE)[1] == 1         # (nothing but empty lines in front: no read before it)
    # across two feeds, empty ones between them
    _refused([good, b'\n\n', late], EVERYWHERE, r'not sorted.*byte offset %d of' % (len(good) + 2))
    _refused([row * 256, late], (np.array([500]), np.array([600])), r'not sorted.*byte offset 4096 of')    # (reads the block drops are checked too)
    # the lowest offset is named
    _refused([good + late + row + late], EVERYWHERE, r'byte offset %d of' % len(good))
    # without a selection the order does not matter
    assert run(good + late, 4) == [0, 0, 1, 3]
    assert run(good + late, 4, cuts=[len(good)]) == [0, 0, 1, 3]


def test_malformed_lines():
    good = b'chr1\t1\tCCCC\t1\nchr1\t3\tTTTT\t2\n'
    for bad in (b'chr1\t5\tCT\n', b'chr1\tx\tCT\t3\n', b'chr1\t5\tCT\t\n', b'chr1\t5\t\t3\n'):
        for blocks in (None, EVERYWHERE):
            _refused([good, bad], blocks, r'invalid line at byte offset %d of' % len(good))
    # a malformed line is named before a descending read, wherever the two lie
    late = b'chr1\t2\tCCC\t1\n'
    _refused([good + late + good + b'chr1\t5\t\t3\n'], EVERYWHERE, r'invalid line at byte offset %d of' % (2 * len(good) + len(late)))
    with pytest.raises(_lib.SegmentorError, match='startCpG 0 < 1'):
        _lib.FragLen(30, [0], [3])
    with pytest.raises(_lib.SegmentorError, match=r'max_frag_size 0 \(1\.\.1048576\)'):
        _lib.FragLen(0)


def test_refusals_through_the_command_line(tmp_path, capsys):
    pat = str(tmp_path / 'u.pat.gz')
    text = b'chr1\t1\tCCCC\t1\nchr1\t3\tTTTT\t2\nchr1\t2\tCCC\t1\n'
    with gzip.open(pat, 'wb') as f:
        f.write(text)
    blocks = tmp_path / 'b.bed'
    blocks.write_text('chr1\t10\t20\t1\t5\n')
    assert wgbs_tools.main(['wgbstools', 'frag_len', pat, '-v', '-L', str(blocks)]) == 1
    io = capsys.readouterr()
    assert io.out == '' and pat + ': failed calculating frag_len: the pat file is not sorted: the read at byte offset %d of' % text.rfind(b'chr1') in io.err
    assert wgbs_tools.main(['wgbstools', 'frag_len', pat, '-v', '-m', '5']) == 0
    assert capsys.readouterr().out == '0 0 1 3 0\n'
    blocks.write_text('chr1\t10\t20\t4\t4\n')
    assert wgbs_tools.main(['wgbstools', 'frag_len', pat, '-v', '-L', str(blocks)]) == 1
    assert 'row 1 has endCpG 4 <= startCpG 4' in capsys.readouterr().err


# ---- random worlds ----
def test_random_against_restatement():
    """random reads, block lists (nested, tied, with gaps), sizes of the histogram, feeds and grid caps against frag_ref, for at most ~4 s"""
    seed0 = int.from_bytes(os.urandom(4), 'little')
    print('frag_len random comparison: seeds from', seed0)
    t_end = time.time() + 4
    k = 0
    while time.time() < t_end and k < 200:
        rng = np.random.default_rng(seed0 + k)
        text, m, blocks = FC.random_world(rng)
        want = FR.frag_hist(text, m, blocks)
        groups = int(rng.choice([-1, 1, 2, 7]))
        if text.endswith(b'\n'):
            ends = [i + 1 for i, ch in enumerate(text) if ch == 10]
            cuts = sorted(set(rng.choice(ends, int(rng.integers(0, 4))).tolist()))
            got = run(text, m, blocks, groups=groups, cuts=cuts)
        else:
            got = run(text, m, blocks, groups=groups, bgzf=True)
        assert got == want, ('seed', seed0 + k)
        k += 1
    assert k > 0
