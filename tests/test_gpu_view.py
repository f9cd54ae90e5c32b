"""`wgbstools view` / `cview` on the GPU (the kernels of csrc/view_kernels.h behind wgbsseg_patview_*): every golden of the reference's
tools through the command line, from BGZF inflated on the device and from plain gzip; the edges of the text; the order with and
without the sort; the sort itself (several LDS runs and merge passes, prefixes, late differences, repeats); the collapse across tiles
and feeds; chunking; growth of the two buffers; the refusals and their byte offsets; BGZF output deflated on the device; a time-boxed
random comparison against the restatement tests/view_ref.py."""
import gzip
import json
import os.path as op
import time

import numpy as np
import pytest

import view_cases as VC
import view_ref as VR
from wgbs_tools_amd import _lib, homog, wgbs_tools

pytestmark = pytest.mark.gpu
ROOT = op.dirname(op.dirname(op.abspath(__file__)))
RUN = 512                                                          # csrc/view_plan.h WG_VIEW_RUN (tests/test_view_cpu.py checks it)
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


@pytest.fixture(scope='module')
def golden():
    with open(op.join(ROOT, 'tests', 'golden', 'view_cases.json')) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def genome(tmp_path_factory):
    return VC.genome_dir(str(tmp_path_factory.mktemp('view_genome')))[0]


def bgzf_bytes(text, member=65280):
    return b''.join(homog._bgzf_member(text[p:p + member]) for p in range(0, len(text), member)) + homog._bgzf_member(b'')


def run(text, s, e, cuts=None, bgzf=False, initial_records=0, deflate=False, info=None, **flags):
    """the device's output for `text`; cuts: byte offsets (line ends) at which the text is cut into feeds (equal offsets: an empty
    feed); bgzf: fed as BGZF bytes (a text without its last newline must go this way); info: a dict that receives PatView.info()"""
    with _lib.PatView(s, e, initial_records=initial_records, **flags) as v:
        if bgzf:
            data = bgzf_bytes(text, 3000)
            assert v.feed_bgzf(data) == len(data)
        else:
            pos = 0
            for cut in list(cuts or []) + [len(text)]:
                v.feed(text[pos:cut])
                pos = cut
        lines, nbytes = v.finish(deflate=deflate)
        out = v.read()
        assert len(out) == nbytes
        if not deflate:
            assert out.count(b'\n') == lines
            assert b''.join(v.chunks(1000)) == out and v.read(nbytes, 0) == b''
        if info is not None:
            info.update(v.info(), lines=lines)
        return out


def passes_of(n):
    runs, k = -(-n // RUN), 0
    while runs > 1:
        runs, k = (runs + 1) // 2, k + 1
    return k


# ---- the reference's output through the command line ----
@pytest.mark.parametrize('how', ['bgzf_device', 'gzip'])
@pytest.mark.parametrize('name', sorted(VC.CASES))
def test_cli_matches_reference(name, how, golden, genome, tmp_path, capfd):
    rec = golden[name]
    text = VC.case_pat(VC.CASES[name])
    pat = str(tmp_path / 'smp.pat.gz')
    if how == 'gzip':
        with gzip.open(pat, 'wb') as f:
            f.write(text)
    else:
        homog.write_bgzf(pat, text, 4)
    cmd = 'view' if how == 'gzip' else 'cview'
    argv = ['wgbstools', cmd, pat, '--genome', genome] + rec['where'] + rec['flags'] + (['--inflate', 'device'] if how == 'bgzf_device' else [])
    assert wgbs_tools.main(argv) == 0
    assert capfd.readouterr().out == rec['stdout'], name
    out = str(tmp_path / 'out.pat')
    assert wgbs_tools.main(argv + ['-o', out]) == 0
    assert capfd.readouterr().out == ''
    with open(out, 'rb') as f:
        assert f.read().decode() == rec['stdout']


# ---- the edges of the text ----
def test_text_edges():
    long_read = b'chr1\t38\t' + b'CT.H' * 375 + b'\t3\n'              # 1,500 CpGs: longer than the spill behind a tile
    lines = [b'chr1\t%d\t%s\t%d\n' % (10 + i // 7, b'CTH.'[:1 + i % 4] * (1 + i % 5), 1 + i % 9) for i in range(600)]
    text = b'\n\n' + b''.join(lines[:200]) + b'\n' + long_read + b'\n\n\n' + b''.join(lines[200:]) + b'\n'
    assert len(text) > 2 * 4096                                       # lines straddle two tile edges
    for s, e in ((1, 2000), (50, 90), (60, 1400), (1000, 1001)):
        for flags in (dict(), dict(strict=True, sort=True), dict(strict=True, strip=True, min_len=2, sort=True), dict(no_gaps=True, sort=True),
                      dict(strip=True)):
            want = VR.view(text, s, e, **flags)
            assert run(text, s, e, **flags) == want, (s, e, flags)
            assert run(text.rstrip(b'\n'), s, e, bgzf=True, **flags) == want, (s, e, flags)      # a last line without its newline
    got = run(text, 60, 1400, strict=True).splitlines()               # the long read, clipped at both ends
    assert b'chr1\t60\t' + (b'CT.H' * 375)[22:22 + 1340] + b'\t3' in got


def test_order_with_and_without_the_sort(tmp_path, capfd, genome):
    text = b'chr1\t10\t..C\t4\nchr1\t11\tT\t5\n'
    moved, other = b'chr1\t12\tC\t4\n', b'chr1\t11\tT\t5\n'
    assert run(text, 5, 50, strip=True, sort=True) == other + moved
    assert run(text, 5, 50, strip=True, sort=False) == moved + other
    assert run(text, 1, VC.N_SITES + 1, strip=True) == moved + other
    pat = str(tmp_path / 'o.pat.gz')
    homog.write_bgzf(pat, text, 1)
    for extra, want in ((['-s', '5-50'], other + moved), (['-s', '5-50', '--no_sort'], moved + other), ([], moved + other)):
        assert wgbs_tools.main(['wgbstools', 'view', pat, '--genome', genome, '--strip'] + extra) == 0
        assert capfd.readouterr().out.encode() == want


# ---- the sort ----
def _amplicon(rng, s):
    """~5,000 reads that all start before s and reach past it: cut under --strict they all start at s, their patterns in random order"""
    base = VC.random_pattern(rng, 90, 0.1).encode()
    pool = [base[:k] for k in (1, 2, 3, 30, 64, 65, 80, 90)]                      # prefixes of one another
    pool += [base[:70] + t for t in (b'C', b'T', b'CC', b'CT', b'H')]             # first differ beyond byte 64
    pool += [VC.random_pattern(rng, int(rng.integers(1, 12)), 0.2).encode() for _ in range(1500)]
    tails = [pool[i] for i in rng.integers(0, len(pool), 4900)]                  # exact repeats
    starts = np.sort(rng.integers(s - 30, s, len(tails)))
    lines = [(b'chr1', int(a), b'H' * (s - int(a)) + t, int(rng.integers(1, 9))) for a, t in zip(starts, tails)]
    first_before = next(i for i, ln in enumerate(lines) if ln[1] == s - 1)
    lines.insert(first_before, (b'chr1', s - 1, b'CCT', 7))                       # CCT at s - 1 and CT at s: equal only after the clip,
    lines.append((b'chr1', s, b'CT', 11))                                        # and far apart in the input
    return lines


def test_sort_many_equal_starts():
    rng = np.random.default_rng(20261103)
    s, e = 1000, 1200
    lines = _amplicon(rng, s)
    text = b''.join(b'%s\t%d\t%s\t%d\n' % ln for ln in lines)
    n = len(lines)
    assert n > RUN and passes_of(n) >= 3
    info = {}
    got = run(text, s, e, strict=True, sort=True, info=info)
    want = VR.view(text, s, e, strict=True, sort=True)
    assert got == want
    assert info['records'] == n and info['order'] == 2 and info['merge_passes'] == passes_of(n)
    both = [ln for ln in want.splitlines() if ln.startswith(b'chr1\t1000\tCT\t')]
    assert len(both) == 1 and int(both[0].split(b'\t')[3]) >= 18                  # 7 + 11 collapsed (+ whatever else cut to CT)
    assert run(text, s, e, strict=True, sort=False) == VR.view(text, s, e, strict=True, sort=False) != want
    # the same survivors, already in order: whatever path that takes, the same answer
    ordered = sorted(VR.survivors(text, s, e, strict=True), key=VR.sort_key)
    text2 = b''.join(b'%s\t%d\t%s\t%d\n' % ln for ln in ordered)
    info2 = {}
    assert run(text2, s, e, strict=True, sort=True, info=info2) == want
    assert info2['records'] == n and info2['order'] == 1 and info2['merge_passes'] == 0
    # one record out of place at the very end: sorted again
    text3 = text2 + b'chr1\t%d\tC\t1\n' % s
    assert run(text3, s, e, strict=True, sort=True, info=info2) == VR.view(text3, s, e, strict=True, sort=True)
    assert info2['order'] == 2


@pytest.mark.parametrize('n', [1, 2, RUN - 1, RUN, RUN + 1, 2 * RUN, 2 * RUN + 1, 3 * RUN + 17, 4 * RUN + 1])
def test_sort_sizes_around_the_run_length(n):
    rng = np.random.default_rng(n)
    lines = [(b'chr1', 5, VC.random_pattern(rng, int(rng.integers(1, 9)), 0.0).encode() + b'.', 1 + i % 3) for i in range(n)]
    text = b''.join(b'%s\t%d\t%s\t%d\n' % ln for ln in lines)
    info = {}
    assert run(text, 1, 100, sort=True, info=info) == VR.view(text, 1, 100, sort=True)
    assert info['records'] == n and info['merge_passes'] == (passes_of(n) if info['order'] == 2 else 0)


# ---- the collapse ----
def test_collapse():
    same = b'chr1\t5\tCCT\t1\n'
    text = same * 700                                                 # one run over three tiles
    assert len(text) > 2 * 4096
    assert run(text, 1, 100) == b'chr1\t5\tCCT\t700\n'
    assert run(text, 1, 100, cuts=[len(same) * 3, len(same) * 3, len(same) * 400]) == b'chr1\t5\tCCT\t700\n'      # and over feeds
    assert run(text + b'chr1\t5\tCCT.\t2\n' + same, 1, 100) == b'chr1\t5\tCCT\t700\nchr1\t5\tCCT.\t2\nchr1\t5\tCCT\t1\n'   # adjacent lines only
    assert run(text + b'chr1\t5\tCCT.\t2\n' + same, 1, 100, sort=True) == b'chr1\t5\tCCT\t701\nchr1\t5\tCCT.\t2\n'
    zero = b'chr1\t7\tC\t3\nchr1\t7\tC\t-3\n'
    assert run(zero, 1, 100) == b''
    assert run(b'chr1\t6\tT\t1\n' + zero + b'chr1\t7\tC\t-1\nchr1\t7\tCC\t0\nchr1\t8\tT\t2\n', 1, 100) == b'chr1\t6\tT\t1\nchr1\t8\tT\t2\n'
    big = b'chr1\t9\tTT\t2147483647\n' * 3
    assert run(big, 1, 100) == b'chr1\t9\tTT\t%d\n' % (3 * (2 ** 31 - 1))
    with pytest.raises(_lib.SegmentorError, match='failed in view: a collapsed count of 10\\^15 or more'):
        run(b'chr1\t9\tTT\t2147483647\n' * 465662, 1, 100)
    assert run(b'chr1\t9\tTT\t2147483647\n' * 465661, 1, 100) == b'chr1\t9\tTT\t%d\n' % (465661 * (2 ** 31 - 1))


def test_no_output_at_all(tmp_path, capfd, genome):
    info = {}
    assert run(b'chr1\t7\tC\t3\nchr1\t7\tC\t-3\n', 1, 100, info=info) == b'' and info['lines'] == 0 and info['records'] == 2
    assert run(b'', 1, 100, info=info) == b'' and info['lines'] == 0 and info['records'] == 0
    assert run(b'\n\n', 1, 100, sort=True) == b''
    pat = str(tmp_path / 'none.pat.gz')
    homog.write_bgzf(pat, b'chr1\t7\tC\t3\nchr1\t7\tC\t-3\nchr1\t900\tC\t1\n', 1)
    assert wgbs_tools.main(['wgbstools', 'view', pat, '--genome', genome, '-s', '1-100']) == 0
    assert capfd.readouterr().out == ''


# ---- chunking and growth ----
def _forty_kb():
    rng = np.random.default_rng(5)
    st = np.sort(rng.integers(1, 900, 2000))
    text = b''.join(b'chr%d\t%d\t%s\t%d\n' % (1 + (st[i] > 450), st[i], VC.random_pattern(rng, int(rng.integers(1, 12))).encode(), i % 30 - 2) for i in range(2000))
    assert 8 * 4096 < len(text) <= 12 * 4096
    return text


def _line_ends(text):
    return [i + 1 for i, c in enumerate(text) if c == 10]


def test_chunking():
    text = _forty_kb()
    rng = np.random.default_rng(6)
    ends = _line_ends(text)
    for flags in (dict(), dict(sort=True, strict=True, strip=True), dict(strip=True, min_len=2)):
        for s, e in ((1, 1000), (300, 340)):
            whole = run(text, s, e, **flags)
            assert whole == VR.view(text, s, e, **flags)
            for _ in range(3):
                cuts = sorted(rng.choice(ends, int(rng.integers(1, 12))).tolist() * int(rng.integers(1, 3)))      # (doubled: empty feeds between)
                assert run(text, s, e, cuts=cuts, **flags) == whole
    with _lib.PatView(1, 100) as v:
        v.feed(b'chr1\t5\tC\t1\n')
        with pytest.raises(_lib.SegmentorError, match='feed and feed_bgzf cannot be mixed'):
            v.feed_bgzf(bgzf_bytes(b'chr1\t6\tC\t1\n'))
        with pytest.raises(_lib.SegmentorError, match='a chunk must end with a complete line'):
            v.feed(b'chr1\t6\tC\t1')


def test_growth():
    text = _forty_kb()
    ends = _line_ends(text)
    cuts = [ends[k] for k in range(len(ends) // 7, len(ends) - 1, len(ends) // 7)]
    s, e = 1, 1000
    cap_r, cap_a, n_r, n_a, grown_r, grown_a, pos = 8, 8 * 16, 0, 0, 0, 0, 0      # the plan's growth rule over these feeds
    for cut in cuts + [len(text)]:
        feed = text[pos:cut]
        pos = cut
        need_r, need_a = n_r + len(feed) // 7 + 1, n_a + len(feed)
        if need_r > cap_r:
            cap_r, grown_r = max(need_r, 2 * cap_r), grown_r + 1
        if need_a > cap_a:
            cap_a, grown_a = max(need_a, 2 * cap_a), grown_a + 1
        kept = VR.survivors(feed, s, e, strip=True)
        n_r, n_a = n_r + len(kept), n_a + sum(len(c) + len(p) for c, _, p, _ in kept)
    assert grown_r >= 2 and grown_a >= 2
    info = {}
    got = run(text, s, e, cuts=cuts, initial_records=8, strip=True, sort=True, info=info)
    assert got == run(text, s, e, strip=True, sort=True) == VR.view(text, s, e, strip=True, sort=True)
    assert (info['grown_records'], info['grown_arena'], info['records'], info['arena_bytes']) == (grown_r, grown_a, n_r, n_a)
    assert n_a <= len(text)                                           # the arena never holds more than the text fed


# ---- refusals ----
def _refusal(text, s=1, e=5000, **kw):
    with pytest.raises(_lib.SegmentorError) as err:
        run(text, s, e, **kw)
    assert err.value.code == _lib.E_ARG and err.value.msg.startswith('failed in view: ')
    kind = 'bad' if 'invalid line' in err.value.msg else 'desc' if 'not sorted' in err.value.msg else '?'
    return kind, int(err.value.msg.split('byte offset ')[1].split()[0])


def test_refusals_name_the_offset():
    good = b''.join(b'chr1\t%d\tCCTT\t1\n' % (10 + i) for i in range(40))
    tail = b'chr1\t900\tC\t1\n'
    for bad in (b'chr1\t905\tCT\n', b'chr1\tx\tCT\t3\n', b'chr1\t905\tCT\t3\t9\n', b'chr1\t905\tCT\t3\r\n', b'chr1\t905\t\t3\n', b'chr1\t905\tCT\t\n'):
        assert _refusal(good + bad + tail) == ('bad', len(good)), bad
        assert _refusal(good + bad + tail, bgzf=True) == ('bad', len(good)), bad
    assert _refusal(good + b'chr1\t905\tCT\t3\r', bgzf=True) == ('bad', len(good))   # (a CRLF file's last line without its newline)
    # a descending read inside a tile — also for the whole genome, also where it would not be selected
    assert _refusal(good + b'chr1\t20\tC\t1\n' + tail) == ('desc', len(good))
    assert _refusal(good + b'chr1\t20\tC\t1\n' + tail, s=2000, e=2001, sort=True) == ('desc', len(good))
    # across a tile edge: the first line of the second tile starts before the last line of the first
    fill = b''.join(b'chr1\t%d\tCCTTCCTT\t1\n' % (1000 + i) for i in range(400))
    at = max(p for p in [0] + [i + 1 for i, c in enumerate(fill) if c == 10] if p <= 4096)
    while at < 4096:                                                  # pad the line in front so that the next one begins at the edge
        fill = fill[:at - 3] + b'T' + fill[at - 3:]
        at += 1
    assert at == 4096 and fill[at - 1:at] == b'\n'
    text = fill[:at] + b'chr1\t999\tC\t1\n' + fill[at:]
    assert _refusal(text) == ('desc', 4096)
    # across feeds, with an empty feed and empty lines between
    assert _refusal(good + b'\n\nchr1\t20\tC\t1\n' + tail, cuts=[len(good), len(good), len(good) + 1]) == ('desc', len(good) + 2)
    # the lowest offset is named, and a malformed line before a descending one wherever they lie
    assert _refusal(good + b'chr1\t20\tC\t1\n' + b'chr1\t19\tC\t1\n' + tail) == ('desc', len(good))
    assert _refusal(good + b'chr1\t20\tC\t1\n' + b'chr1\t21\tC\n' + b'chr1\t22\t\t1\n') == ('bad', len(good) + 12)
    assert _refusal(text + b'chr1\t2000\tCT\n') == ('bad', len(text))


# ---- BGZF out ----
def test_deflate_on_the_device(tmp_path, capfd, genome, golden):
    rec = golden['region_strict_strip']
    pat = str(tmp_path / 'smp.pat.gz')
    homog.write_bgzf(pat, VC.case_pat(VC.CASES['region_strict_strip']), 4)
    out = str(tmp_path / 'out.pat.gz')
    argv = ['wgbstools', 'view', pat, '--genome', genome] + rec['where'] + rec['flags'] + ['--inflate', 'device', '-o', out]
    assert wgbs_tools.main(argv + ['--deflate', 'device']) == 0
    with open(out, 'rb') as f:
        data = f.read()
    assert data.endswith(BGZF_EOF) and data[:4] == b'\x1f\x8b\x08\x04' and len(data) < len(rec['stdout'])
    assert gzip.decompress(data).decode() == rec['stdout']
    assert wgbs_tools.main(argv) == 0                                 # without it: the reference's plain text, whatever the name
    with open(out, 'rb') as f:
        assert f.read().decode() == rec['stdout']
    homog.write_bgzf(pat, b'chr1\t7\tC\t3\nchr1\t7\tC\t-3\n', 1)          # an empty result: the end-of-file member alone
    assert wgbs_tools.main(['wgbstools', 'view', pat, '--genome', genome, '-s', '1-100', '-o', out, '--deflate', 'device']) == 0
    with open(out, 'rb') as f:
        assert f.read() == BGZF_EOF
    rng = np.random.default_rng(8)
    st = np.sort(rng.integers(1, 900, 9000))
    text = b''.join(b'chr1\t%d\t%s\t%d\n' % (st[i], VC.random_pattern(rng, int(rng.integers(1, 40))).encode(), 1 + i % 30) for i in range(9000))
    plain = run(text, 1, 1000)
    packed = run(text, 1, 1000, deflate=True)
    assert packed.endswith(BGZF_EOF) and gzip.decompress(packed) == plain and len(plain) > 2 * 65280
    assert len(plain) % 65280                                         # (the last member is a short one)
    assert packed == _lib.bgzf_deflate(plain)                         # view and the stand-alone call: one member rule, the same kernels
    assert run(b'', 1, 1000, deflate=True) == BGZF_EOF == _lib.bgzf_deflate(b'')
    for deflate in (True, False):                                     # the deflate phase is timed when it runs, and only then
        with _lib.PatView(1, 1000) as v:
            v.feed(text)
            v.finish(deflate=deflate)
            ms = v.phase_ms()[2]
            assert ms > 0 if deflate else ms == 0


# ---- random worlds ----
def test_random_worlds_against_restatement():
    seed = 20261104
    rng = np.random.default_rng(seed)
    t0, worlds = time.monotonic(), 0
    while worlds < 1 or time.monotonic() - t0 < 4.0:
        text, s, e, flags = VC.random_world(rng)
        ends = _line_ends(text)
        no_newline = not text.endswith(b'\n')
        cuts = None if no_newline or len(ends) < 2 else sorted(rng.choice(ends, int(rng.integers(0, 5))).tolist())
        initial = int(rng.choice([0, 3, 100]))
        print('world', worlds, 'seed', seed, 'bytes', len(text), s, e, flags, 'cuts', cuts, 'bgzf', no_newline, 'initial_records', initial)
        try:
            want = VR.view(text, s, e, **flags)
        except VR.Refused as r:
            assert r.kind == 'sum'
            continue
        assert run(text, s, e, cuts=cuts, bgzf=no_newline, initial_records=initial, **flags) == want
        worlds += 1
    assert worlds >= 1
