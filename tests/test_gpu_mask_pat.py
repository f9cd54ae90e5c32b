"""`wgbstools mask_pat` on the GPU: the view engine with a site mask (wgbsseg_patview_set_mask) — k_view_mask_fill's bitmap at its word
edges, the masked forms of k_view_measure / k_view_pack on reads whose head, tail, interior or whole is hidden, a read of 1,500 sites,
several tiles and rounds with buffers that grow, a line split between two feeds, the sort that the mask makes necessary, lines that
become equal through the mask, an interval, BGZF in and out, the ABI's states and refusals — byte for byte against the goldens of the
reference's tools (tests/golden/mask_cases.json) or tests/mask_ref.py.  The command end to end."""
import gzip
import json
import os.path as op

import numpy as np
import pytest

import mask_cases as KC
import mask_ref as KR
import view_ref as VR
from wgbs_tools_amd import _lib, homog, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))
RUN = 512                                                          # csrc/view_plan.h WG_VIEW_RUN
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'mask_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def genome(tmp_path_factory):
    return KC.genome_dir(str(tmp_path_factory.mktemp('mask_genome')))[0]


def bgzf_bytes(text, member=3000):
    return b''.join(homog._bgzf_member(text[p:p + member]) for p in range(0, len(text), member)) + homog._bgzf_member(b'')


def run(text, blocks, s, e, how='text', initial_records=0, deflate=False, info=None, strip=True, sort=True, **flags):
    """the device's output for `text` with the sites of `blocks` hidden (None: no mask); how: 'text' (whole lines), 'bgzf', or a list of
    byte strings fed one by one with feed_bgzf; info: a dict that receives PatView.info() and mask_info()"""
    mask = None if blocks is None else ([b[0] for b in blocks], [b[1] for b in blocks])
    with _lib.PatView(s, e, strip=strip, sort=sort, initial_records=initial_records, mask=mask, **flags) as v:
        if how == 'text':
            v.feed(text)
        else:
            left = b''
            for piece in ([bgzf_bytes(text)] if how == 'bgzf' else how):
                data = left + piece
                left = data[v.feed_bgzf(data):]
            assert left == b''
        lines, nbytes = v.finish(deflate=deflate)
        out = v.read()
        assert len(out) == nbytes and (deflate or out.count(b'\n') == lines)
        if info is not None:
            info.update(v.info(), lines=lines, **v.mask_info())
        return out


def passes_of(n):
    runs, k = -(-n // RUN), 0
    while runs > 1:
        runs, k = (runs + 1) // 2, k + 1
    return k


def case(name, golden):
    rec, c = golden[name], KC.CASES[name]
    return KC.case_pat(c), KC.case_blocks(c), rec['sites'], rec['stdout'].encode()


# ---- the worked case ----
def test_worked_case_as_text_as_bgzf_and_without_its_last_newline(golden):
    text, blocks, (s, e), want = case('worked', golden)
    assert want == KC.WORKED_OUT == KR.mask_pat(text, blocks, s, e)
    info = {}
    assert run(text, blocks, s, e, info=info) == want
    assert (info['hidden_sites'], info['mask_words'], info['masked']) == (4, 1, 1) and info['records'] == 6
    assert run(text, blocks, s, e, how='bgzf') == want
    assert not text[:-1].endswith(b'\n') and run(text[:-1], blocks, s, e, how='bgzf') == want
    assert run(text, blocks[::-1] + blocks, s, e) == want              # the order of the blocks and their repeats do not show
    assert run(text, None, s, e) == VR.view(text, s, e, sort=True, strip=True) != want


# ---- the bitmap's edges ----
def test_bitmap_edges(golden):
    text, blocks, (s, e), want = case('edges', golden)
    hidden = KR.Hidden(blocks)
    for site in (KC.EDGE_LO, KC.EDGE_LO + 31, KC.EDGE_LO + 32, KC.EDGE_LO + 63, KC.EDGE_LO + 64, KC.EDGE_HI - 1):
        assert site in hidden
    info = {}
    assert run(text, blocks, s, e, info=info) == want == KR.mask_pat(text, blocks, s, e)
    assert (info['hidden_sites'], info['mask_words']) == (golden['edges']['loaded'], 10) and info['mask_ms'] > 0.0
    assert run(text, blocks, s, e, how='bgzf', initial_records=8) == want
    assert run(text, KR.union(blocks), s, e) == want                  # overlapping, nested, duplicate, unsorted blocks against their union
    # one hidden site at a time at every edge of the words: reads that start before lo, end behind hi or lie outside come through
    reads = KC.lines_text([(rs, b'CTTC' * 3, 1 + rs % 2) for rs in range(80, 180, 3)] + [(500, b'CT', 1)])
    for site in (100, 131, 132, 163, 164):
        for one in ([(site, site + 1)], [(100, 101), (site, site + 1), (164, 165)]):
            assert run(reads, one, 1, 4001) == KR.mask_pat(reads, one, 1, 4001), one
    whole = [(100, 196)]                                               # three whole words
    assert run(reads, whole, 1, 4001) == KR.mask_pat(reads, whole, 1, 4001)


def test_reads_hidden_at_the_head_the_tail_inside_and_wholly():
    blocks = [(10, 14), (20, 21), (50, 150)]
    reads = [(8, b'CTCCCCT', 1),                                        # interior 10 .. 13: dots, kept
             (10, b'CCCC', 9),                                          # wholly hidden: dropped
             (10, b'CCCCT', 2),                                         # hidden head: starts at 14
             (11, b'TT', 1),                                            # wholly hidden: dropped
             (12, b'CC.T', 1),                                          # a dot of the file behind the hidden head: starts at 15
             (17, b'TTTC', 3), (19, b'.C.', 1),                         # hidden tail; dots on both sides of a hidden site: dropped
             (45, b'T' * 5 + b'C' * 100 + b'T', 1),                     # interior of 100
             (50, b'C' * 100 + b'TT', 4), (60, b'C' * 90 + b'T', 1),    # heads that move across a 64- and a 32-site boundary
             (149, b'C.C', 2), (150, b'C', 1)]
    text = KC.lines_text(reads)
    want = (b'chr1\t8\tCT....T\t1\nchr1\t14\tT\t2\nchr1\t15\tT\t1\nchr1\t17\tTTT\t3\nchr1\t45\tTTTTT' + b'.' * 100 + b'T\t1\n'
            b'chr1\t150\tC\t1\nchr1\t150\tT\t1\nchr1\t150\tTT\t4\nchr1\t151\tC\t2\n')
    assert KR.mask_pat(text, blocks, 1, 4001) == want
    assert run(text, blocks, 1, 4001) == want
    assert run(text, blocks, 1, 4001, how='bgzf') == want


def test_a_read_of_1500_sites(golden):
    text, blocks, (s, e), want = case('long_read', golden)
    assert len(text.split(b'\n')[2]) > 1500 and len(blocks) == 825
    info = {}
    assert run(text, blocks, s, e, info=info) == want
    assert info['hidden_sites'] == 825 and info['mask_words'] == (1899 - 250 + 31) // 32
    assert run(text, blocks, s, e, how='bgzf') == want
    front = b''.join(b'chr1\t%d\tCT\t1\n' % (1 + i // 3) for i in range(290))     # the long line begins in the first tile and ends behind the bytes staged with it
    assert 3600 < len(front) < 4096
    assert run(front + text, blocks, s, e) == KR.mask_pat(front + text, blocks, s, e)


# ---- the engine ----
def engine_text():
    """about 3,000 short reads over sites 1 .. 999: more than 256 lines in a 4 KB tile, several tiles"""
    text = KC.MC.reads_text(97, 3000, 1, 999, max_len=3)
    assert len(text) > 8 * 4096 and text[:4096].count(b'\n') > 256
    return text


def test_tiles_rounds_growth_and_a_line_split_between_two_feeds():
    text = engine_text()
    blocks = KC.seeded_blocks(98, 150, 1, 999, max_len=2)
    want = KR.mask_pat(text, blocks, 1, 4001)
    hidden = KR.Hidden(blocks)
    kept = sum(1 for c, rs, pat, n in VR.reads_of(text) if KR.cut(rs, pat, hidden, 1, 4001))
    info = {}
    assert run(text, blocks, 1, 4001, initial_records=64, info=info) == want
    assert info['records'] == kept < 3000 and info['grown_records'] >= 1 and info['grown_arena'] >= 1
    assert info['order'] == 2 and info['merge_passes'] == passes_of(kept) >= 2     # hidden heads: the input order is not the sorted one
    cut_at = text.index(b'\n', 20000) - 3                               # inside a line
    assert text[cut_at - 1] != 0x0a and text[cut_at] != 0x0a
    pieces = [homog._bgzf_member(text[:cut_at]), homog._bgzf_member(text[cut_at:]) + homog._bgzf_member(b'')]
    assert run(text, blocks, 1, 4001, how=pieces, initial_records=64) == want
    assert run(text, blocks, 1, 4001, how='bgzf') == want


def test_a_mask_that_touches_no_read_leaves_the_order():
    text = VR.view(engine_text(), 1, 4001, sort=True)                  # sorted and collapsed: its own view
    info = {}
    assert run(text, [(3000, 3100), (1500, 1501)], 1, 4001, info=info) == text
    assert info['order'] == 1 and info['merge_passes'] == 0 and info['masked'] == 1 and info['hidden_sites'] == 101
    text += b'chr1\t1100\tCT\t1\nchr1\t1100\tTC\t1\n'                   # in order; without site 1100 they are 1101 T, 1101 C: not in order
    assert run(text, [(3000, 3100)], 1, 4001, info=info) == text and info['order'] == 1
    assert run(text, [(1100, 1101)], 1, 4001, info=info) == KR.mask_pat(text, [(1100, 1101)], 1, 4001) != text
    assert info['order'] == 2 and text.endswith(b'TC\t1\n') and KR.mask_pat(text, [(1100, 1101)], 1, 4001).endswith(b'chr1\t1101\tC\t1\nchr1\t1101\tT\t1\n')


def test_lines_that_become_equal_through_the_mask_collapse():
    big = 2 ** 31 - 1
    text = KC.lines_text([(5, b'CT', 3), (5, b'CC', 4), (5, b'C', big), (5, b'CTC', big), (6, b'TCT', 1), (7, b'CC', big), (7, b'CT', 2)])
    blocks = [(6, 7)]
    want = b'chr1\t5\tC\t%d\nchr1\t5\tC.C\t%d\nchr1\t7\tCC\t%d\nchr1\t7\tCT\t3\n' % (big + 7, big, big)
    assert KR.mask_pat(text, blocks, 1, 100) == want
    assert run(text, blocks, 1, 100) == want
    assert run(text, None, 1, 100).count(b'\n') == 7


def test_an_interval_selects_on_the_unmasked_read(golden):
    text, blocks, (s, e), want = case('sites_interval', golden)
    assert (s, e) == (1200, 1230)
    assert run(text, blocks, s, e) == want
    assert run(text, blocks, s, e, how='bgzf', initial_records=8) == want
    # a read that reaches s with a site that is hidden stays, cut to what lies in front of the interval; one that starts at e - 1 stays
    # although its start moves to e
    reads = KC.lines_text([(1195, b'CCCCCT', 1), (1196, b'CCCC', 1), (1229, b'CT', 2), (1230, b'C', 1)])
    hide = [(1200, 1201), (1229, 1230)]
    want = b'chr1\t1195\tCCCCC\t1\nchr1\t1230\tT\t2\n'
    assert KR.mask_pat(reads, hide, 1200, 1230) == want
    assert run(reads, hide, 1200, 1230) == want
    name = 'region'
    text, blocks, (s, e), want = case(name, golden)
    assert run(text, blocks, s, e) == want


def test_whole_genome_golden_and_deflate_on_the_device(golden):
    text, blocks, (s, e), want = case('wg_short', golden)
    info = {}
    assert run(text, blocks, s, e, info=info) == want
    assert info['hidden_sites'] == golden['wg_short']['loaded']
    packed = run(text, blocks, s, e, deflate=True)
    assert packed.endswith(BGZF_EOF) and packed[:4] == b'\x1f\x8b\x08\x04' and gzip.decompress(packed) == want


def test_the_other_flags_with_a_mask():
    """the mask lies between --strict and the strip: without STRIP a wholly hidden read stays as dots, NO_GAPS sees the hidden sites"""
    text = KC.lines_text(KC.WORKED_READS)
    hidden = KR.Hidden(KC.WORKED_BLOCKS)
    for kw in (dict(strip=False), dict(strip=False, strict=True), dict(strict=True), dict(no_gaps=True), dict(strict=True, min_len=2)):
        for s, e in ((1, 100), (7, 11)):
            lines = []
            for chrom, rs, pat, count in VR.reads_of(text):
                c = KR.cut(rs, pat, hidden, s, e, **dict(dict(strip=True), **kw))
                if c:
                    lines.append((chrom, c[0], c[1], count))
            want = b''.join(b'%s\t%d\t%s\t%d\n' % r for r in VR.collapse(sorted(lines, key=VR.sort_key)))
            assert run(text, KC.WORKED_BLOCKS, s, e, **kw) == want, (kw, s, e)


# ---- the ABI ----
def test_set_mask_states_and_refusals():
    good = b'chr1\t4\tCC\t1\nchr1\t9\tT\t2\n'
    with _lib.PatView(1, 100, strip=True, sort=True) as v:
        assert v.mask_info() == dict(hidden_sites=0, mask_words=0, masked=0, mask_ms=0.0)
        for blocks, what in ((([], []), r'mask: no blocks \(at least 1\)'), (([5, 0], [9, 4]), r'mask: block 1 starts at site 0 \(sites count from 1\)'),
                             (([5, 9], [9, 9]), r'mask: block 1 = sites \[9, 9\) is empty'), (([5], [2 ** 31]), r'mask: block 0 ends at site 2147483648')):
            with pytest.raises(_lib.SegmentorError, match=what) as err:
                v.set_mask(*blocks)
            assert err.value.code == _lib.E_ARG
        assert v.mask_info()['masked'] == 0                            # a refused mask leaves none
        v.set_mask([9, 3], [10, 5])
        assert {k: v.mask_info()[k] for k in ('hidden_sites', 'mask_words', 'masked')} == dict(hidden_sites=3, mask_words=1, masked=1)
        with pytest.raises(_lib.SegmentorError, match='patview_set_mask: called twice') as err:
            v.set_mask([1], [2])
        assert err.value.code == _lib.E_STATE
        v.feed(good)
        assert v.finish() == (1, len(b'chr1\t5\tC\t1\n')) and v.read() == b'chr1\t5\tC\t1\n'
    for feed in ('text', 'bgzf'):
        with _lib.PatView(1, 100, sort=True) as v:
            if feed == 'text':
                v.feed(good)
            else:
                v.feed_bgzf(bgzf_bytes(good))
            with pytest.raises(_lib.SegmentorError, match='patview_set_mask: called after the first feed') as err:
                v.set_mask([1], [2])
            assert err.value.code == _lib.E_STATE
            assert v.finish()[0] == 2 and v.mask_info()['masked'] == 0
    with pytest.raises(_lib.SegmentorError, match='mask: block 0 = sites'):
        _lib.PatView(1, 100, mask=([5], [5]))


def test_a_count_below_one_is_refused_only_with_a_mask():
    good = b'chr1\t4\tCC\t1\nchr1\t9\tT\t2\n'
    for low in (b'0', b'-3'):
        text = good + b'chr1\t9\tT\t' + low + b'\nchr1\t12\tC\t1\n'
        assert run(text, None, 1, 100).startswith(b'chr1\t4\tCC\t1\n')                     # no mask: summed, as ever
        for how in ('text', 'bgzf'):
            with pytest.raises(_lib.SegmentorError) as err:
                run(text, [(50, 51)], 1, 100, how=how)
            assert err.value.code == _lib.E_ARG and err.value.msg == 'failed in view: count < 1 at byte %d' % len(good)
        with pytest.raises(KR.Refused) as ref:
            KR.mask_pat(text, [(50, 51)], 1, 100)
        assert (ref.value.kind, ref.value.offset) == ('low', len(good))
    for bad, what in ((b'chr1\t9\tCT\n', 'failed in view: invalid line at byte offset %d of the input' % len(good)),
                      (b'chr1\t9\tCT\t1\tx\n', 'failed in view: invalid line at byte offset %d of the input' % len(good)),
                      (b'chr1\t8\tC\t1\n', 'failed in view: the pat file is not sorted')):
        with pytest.raises(_lib.SegmentorError) as err:                # the other refusals are as without a mask, and come first
            run(good + bad + b'chr1\t12\tC\t0\n', [(50, 51)], 1, 100)
        assert err.value.code == _lib.E_ARG and err.value.msg.startswith(what)


# ---- the command end to end ----
def test_cli(golden, genome, tmp_path, capfd):
    text, blocks, _, want = case('wg_short', golden)
    pat, bed, pre = str(tmp_path / 'in.pat.gz'), str(tmp_path / 'snp.bed'), str(tmp_path / 'out')
    homog.write_bgzf(pat, text, 1)
    with open(bed, 'w') as f:
        f.write(KC.table_text(blocks, header=True, comments=True))
    argv = ['wgbstools', 'mask_pat', pat, '-p', pre, '-b', bed, '--genome', genome]
    assert wgbs_tools.main(argv) == 0
    err = capfd.readouterr().err
    assert '[mask_pat] loaded %d sites' % golden['wg_short']['loaded'] in err and 'no .csi index is written' in err
    with open(pre + '.pat.gz', 'rb') as f:
        data = f.read()
    assert data.endswith(BGZF_EOF) and gzip.decompress(data) == want
    assert wgbs_tools.main(argv) == 0 and 'already exists. Skipping it.' in capfd.readouterr().err
    # --beta: this build's pat2beta on the output, into its directory; a hidden site has coverage 0
    assert wgbs_tools.main(argv + ['-f', '--beta', '--inflate', 'device']) == 0
    capfd.readouterr()
    with open(pre + '.pat.gz', 'rb') as f:
        assert gzip.decompress(f.read()) == want
    with _lib.PatBeta(1, KC.N_SITES + 1) as pb:
        pb.feed(want)
        rows = pb.finish()
    got = np.fromfile(pre + '.beta', dtype=np.uint8).reshape(-1, 2)
    assert got.shape == (KC.N_SITES, 2) and np.array_equal(got, rows) and got[:, 1].sum() > 1000
    hidden = KR.Hidden(blocks)
    assert all(got[site - 1, 1] == 0 for a, b in hidden.intervals for site in range(a, b))
    with _lib.PatBeta(1, KC.N_SITES + 1) as pb:
        pb.feed(text)
        assert any(pb.finish()[site - 1, 1] > 0 for a, b in hidden.intervals for site in range(a, b))      # (they were covered before)
    # an interval, --lbeta; a refused input leaves no output behind
    text, blocks, _, want = case('sites_interval', golden)
    homog.write_bgzf(pat, text, 1)
    with open(bed, 'w') as f:
        f.write(KC.table_text(blocks))
    pre2 = str(tmp_path / 'cut')
    assert wgbs_tools.main(['wgbstools', 'mask_pat', pat, '-p', pre2, '-b', bed, '--genome', genome, '--lbeta'] + golden['sites_interval']['where']) == 0
    capfd.readouterr()
    with open(pre2 + '.pat.gz', 'rb') as f:
        assert gzip.decompress(f.read()) == want
    assert np.fromfile(pre2 + '.lbeta', dtype=np.uint16).reshape(-1, 2)[:, 1].sum() == sum(
        int(ln.split(b'\t')[3]) * (len(ln.split(b'\t')[2]) - ln.split(b'\t')[2].count(b'.')) for ln in want.splitlines())
    homog.write_bgzf(pat, text + b'chr1\t1300\tC\t0\n', 1)
    pre3 = str(tmp_path / 'refused')
    assert wgbs_tools.main(['wgbstools', 'mask_pat', pat, '-p', pre3, '-b', bed, '--genome', genome]) == 1
    assert f'{pat}: failed in view: count < 1 at byte {len(text)}' in capfd.readouterr().err
    assert not op.exists(pre3 + '.pat.gz') and [p for p in tmp_path.iterdir() if '.tmp' in p.name] == []
