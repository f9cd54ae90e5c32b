"""BGZF members inflated on the GPU (k_bgzf_inflate behind wgbsseg_bgzf_inflate and wgbsseg_*_feed_bgzf): the decoder against zlib
byte for byte on the valid list of tests/inflate_cases.py; the corrupt list — the one tests/test_inflate_cpu.py runs through the
sanitised host build of the same decoder — refused where the host twin refuses it, with the same file offset and reason; the three pat
engines fed BGZF bytes in members of 300 B, 4 KB and 65280 B, one member per call, in random groups and whole, against the same
engines fed the text; the three commands with --inflate device against their default; a time-boxed random comparison with zlib."""
import gzip
import hashlib
import os.path as op
import time
import zlib

import numpy as np
import pytest

import bimodal_cases as BC
import homog_cases as HC
import inflate_cases as IC
from test_inflate_cpu import L, twin, walk_restated          # noqa: F401
from test_pat2beta_cpu import pat_golden                      # noqa: F401
from wgbs_tools_amd import _lib, homog, synth, test_bimodal, wgbs_tools

pytestmark = pytest.mark.gpu
PREFIX = 'Invalid gzip data: BGZF member at file offset %d: %s'


# ---- the decoder on the device ---------------------------------------------------------------------------------------------------------
def test_valid_members_match_zlib():
    cases = IC.valid_cases()
    for name, payload, text in cases:
        assert _lib.bgzf_inflate(IC.member(payload, len(text))) == (text, len(payload) + 26), name
    # all of them in one call, with the end-of-file member among and behind them
    data = b''.join(IC.member(payload, len(text)) + (IC.EOF_MEMBER if k % 3 == 0 else b'') for k, (_n, payload, text) in enumerate(cases)) + IC.EOF_MEMBER
    assert _lib.bgzf_inflate(data) == (b''.join(text for _n, _p, text in cases), len(data))


def test_members_per_call_and_consumed():
    rng = np.random.default_rng(1)
    text = IC.pat_text(rng, 200000)
    data = IC.bgzf(text, block=300)
    rows, used = walk_restated(data)
    assert len(rows) > 600 and used == len(data)
    assert _lib.bgzf_inflate(data) == (text, len(data))                         # several hundred members in one call
    one = IC.bgzf(text[:300], block=300, eof=False)
    assert _lib.bgzf_inflate(one) == (text[:300], len(one))                     # one member
    assert _lib.bgzf_inflate(IC.EOF_MEMBER) == (b'', len(IC.EOF_MEMBER))        # the end-of-file member alone
    assert _lib.bgzf_inflate(b'') == (b'', 0)
    ends = [r[0] + r[1] + 8 for r in rows]
    for cut in (1, 17, ends[0] - 1, ends[0], ends[0] + 1, ends[4] + 12, ends[4] + 18, ends[200] - 9, len(data) - 1):
        whole = max([e for e in ends if e <= cut], default=0)
        want = b''.join(zlib.decompress(data[r[0]:r[0] + r[1]], -15) for r in rows if r[0] + r[1] + 8 <= cut)
        assert _lib.bgzf_inflate(data[:cut]) == (want, whole), cut
    # members of 4 KB and of 65280 B, at every alignment of their slots in the text buffer
    for block in (4096, 65280):
        shifted = IC.bgzf(text[:7], block=7, eof=False) + IC.bgzf(text[7:], block=block)
        assert _lib.bgzf_inflate(shifted) == (text, len(shifted)), block
    for lead in range(1, 17):
        shifted = IC.bgzf(text[:lead], block=lead, eof=False) + IC.bgzf(text[lead:40000], block=16500)
        assert _lib.bgzf_inflate(shifted) == (text[:40000], len(shifted)), lead


def test_corrupt_members_are_refused_like_the_host_twin(L):                      # noqa: F811
    """every case of the corpus behind a good member: the device refuses exactly what the twin refuses, naming the member's offset and
    the twin's reason, and returns the twin's text where it accepts"""
    good = IC.member(IC.deflate(b'chr1\t1\tCT\t1\n'), 12)
    refused = 0
    for name, payload, isize in IC.corpus():
        if len(payload) + 26 > 65536:
            continue
        rc, text = twin(L, payload, isize)
        got, used, msg = _lib.bgzf_inflate(good + IC.member(payload, isize), refusal=True)
        assert used == len(good) + len(payload) + 26, name
        if rc == IC.OK:
            assert msg is None and got == b'chr1\t1\tCT\t1\n' + text, name
        else:
            assert msg == PREFIX % (len(good), IC.WHAT[rc]), name
            assert len(got) == 12 + isize and got[:12] == b'chr1\t1\tCT\t1\n', name
            refused += 1
    assert refused > 150
    assert {why for _n, _p, _i, why, _a in IC.handmade_cases()} == set(range(16))


def test_first_corrupt_member_of_a_call_wins_and_its_slot_is_defined(L):        # noqa: F811
    rng = np.random.default_rng(2)
    text = IC.pat_text(rng, 30000)
    members = [IC.member(IC.deflate(text[p:p + 1000]), len(text[p:p + 1000])) for p in range(0, len(text), 1000)]
    bad = {7: IC.TRUNCATED, 19: IC.BLOCK_TYPE}
    cut = bytearray(members[7])
    members[7] = IC.member(bytes(cut[18:-8])[:200], 1000)                        # the stream stops in the middle
    members[19] = IC.member(b'\x07', 1000)
    data = b''.join(members)
    offsets = np.cumsum([0] + [len(m) for m in members])
    got, used, msg = _lib.bgzf_inflate(data, refusal=True)
    assert used == len(data) and msg == PREFIX % (offsets[7], IC.WHAT[bad[7]])
    rc, part = twin(L, bytes(cut[18:-8])[:200], 1000)
    assert rc == IC.TRUNCATED
    for k in range(len(members)):
        piece = got[1000 * k:1000 * (k + 1)]
        if k == 19:
            assert piece == b'\n' * 1000
        elif k == 7:                                                             # what was decoded, then newlines
            stop = len(piece.rstrip(b'\n'))
            assert 0 < stop < 1000 and piece[:stop] == text[7000:7000 + stop] and piece[stop:] == b'\n' * (1000 - stop)
        else:
            assert piece == text[1000 * k:1000 * (k + 1)], k


def test_time_boxed_random_comparison_with_zlib():
    seed = int(time.time())
    print('seed', seed)
    rng = np.random.default_rng(seed)
    t0, ran = time.time(), 0
    while time.time() - t0 < 5.0:
        n = int(rng.choice([0, 1, 500, 70000, 300000]))
        text = IC.pat_text(rng, n)[:n] if rng.random() < 0.6 else rng.integers(0, int(rng.choice([2, 4, 256])), n, dtype=np.uint8).tobytes()
        block = int(rng.choice([1, 300, 4096, 65280])) if n <= 70000 else int(rng.choice([300, 4096, 65280]))
        if n > 500 and block == 1:
            block = 37
        level = int(rng.choice([0, 1, 6, 9]))
        strategy = int(rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY, zlib.Z_FILTERED]))
        data = IC.bgzf(text, block=block, level=level, strategy=strategy)
        assert _lib.bgzf_inflate(data) == (text, len(data)), (seed, ran, n, block, level, strategy)
        ran += 1
    assert ran >= 1


# ---- the engines -----------------------------------------------------------------------------------------------------------------------
LONG_LINE = b'chr1\t2500\t' + b'CTC.T' * 1000 + b'\t3\n'                         # longer than a 4 KB member


def _patbeta_world():
    lines = synth.synth_pat_lines(11, 3000, 20000)
    text = ('\n'.join(lines) + '\n').encode()
    at = text.find(b'\n', len(text) // 2) + 1
    return text[:at] + LONG_LINE + text[at:], lambda: _lib.PatBeta(1, 3001), lambda e: e.finish(lbeta=True).tobytes()


def _homog_world(name):
    case = HC.CASES[name]
    s, e, _ = HC.case_blocks(case['blocks'])
    o = np.lexsort((e, s))
    rlen = int(case['args'][case['args'].index('-l') + 1]) if '-l' in case['args'] else 3
    edges = homog.parse_range(homog.range_text(rlen))
    return HC.case_pat(case['pat']), lambda: _lib.Homog(s[o], e[o], edges, rlen), lambda h: h.finish().tobytes()


def _bimodal_world():
    case = BC.CASES['L_strict']
    text, _, _ = BC.case_inputs(case)
    s, e = BC.case_blocks(case['blocks'])

    def result(b):
        ll, cnt = b.finish()
        return ll.tobytes() + cnt.tobytes()
    return text, lambda: _lib.Bimodal(s, e, True, 1), result


WORLDS = {'patbeta': _patbeta_world, 'homog long_reads_signed': lambda: _homog_world('long_reads_signed'), 'homog nested': lambda: _homog_world('nested'),
          'bimodal': _bimodal_world}
_world_cache = {}


def _world(name):
    """(text, engine maker, result reader, the result of feeding the text) — made once per world"""
    if name not in _world_cache:
        text, make, result = WORLDS[name]()
        with make() as eng:
            eng.feed(text)
            want = result(eng)
        _world_cache[name] = (text, make, result, want)
    return _world_cache[name]


def _feed_bgzf(eng, data, cuts):
    """data in calls that end at `cuts`, the bytes a call did not take in front of the next one"""
    tail = b''
    for a, b in zip([0] + cuts, cuts + [len(data)]):
        buf = tail + data[a:b]
        tail = buf[eng.feed_bgzf(buf):]
    assert tail == b''


def _cuts(rng, data, mode):
    ends = [r[0] + r[1] + 8 for r in walk_restated(data)[0]]
    if mode == 'whole':
        return []
    if mode == 'one':
        return ends[:-1]
    if mode == 'groups':
        return sorted(set(rng.choice(ends, max(1, len(ends) // 4)).tolist()) - {len(data)})
    return sorted(set(rng.integers(1, len(data), 6).tolist()))                  # 'anywhere': calls that end inside a member


@pytest.mark.parametrize('block', [300, 4096, 65280])
@pytest.mark.parametrize('name', sorted(WORLDS))
def test_feeding_bgzf_equals_feeding_text(name, block):
    text, make, result, want = _world(name)
    rng = np.random.default_rng(block)
    data = IC.bgzf(text, block=block, level=1)
    for mode in ('one', 'groups', 'whole', 'anywhere'):
        with make() as eng:
            _feed_bgzf(eng, data, _cuts(rng, data, mode))
            assert result(eng) == want, mode
            assert eng.inflate_ms() > 0 and eng.kernel_ms() > 0
    if block == 4096:                                                            # a file without a final newline: finish() feeds the last line
        open_end = IC.bgzf(text[:-1], block=block, level=1)
        for mode in ('groups', 'whole'):
            with make() as eng:
                _feed_bgzf(eng, open_end, _cuts(rng, open_end, mode))
                assert result(eng) == want, mode


def _refusal(eng, result):
    with pytest.raises(_lib.SegmentorError) as e:
        result(eng)
    return e.value.msg


@pytest.mark.parametrize('name', ['patbeta', 'homog nested', 'bimodal'])
def test_text_refusals_name_the_same_offsets(name):
    text, make, result, _want = _world(name)
    at = text.find(b'\n', len(text) // 3) + 1
    broken = {'malformed': text[:at] + b'chr1\t77\tCT\n' + text[at:]}
    if name != 'patbeta':
        broken['unsorted'] = text + b'chr1\t1\tCCCC\t1\n'
        broken['unsorted, no final newline'] = text + b'chr1\t1\tCCCC\t1'
    rng = np.random.default_rng(4)
    for what, bad in broken.items():
        with make() as eng:
            eng.feed(bad if bad.endswith(b'\n') else bad + b'\n')
            want = _refusal(eng, result)
        assert 'byte offset %d ' % (at if what == 'malformed' else len(text)) in want
        for block in (300, 65280):
            data = IC.bgzf(bad, block=block, level=1)
            for mode in ('groups', 'whole'):
                with make() as eng:
                    _feed_bgzf(eng, data, _cuts(rng, data, mode))
                    assert _refusal(eng, result) == want, (what, block, mode)


def test_inflate_refusal_comes_first_and_mixing_is_refused():
    text, make, result, _want = _world('homog nested')
    at = text.find(b'\n', 5000) + 1
    bad_text = text[:at] + b'chr1\t77\tCT\n' + text[at:]                        # a malformed line in member 1 ...
    members = [IC.member(IC.deflate(bad_text[p:p + 4096]), len(bad_text[p:p + 4096])) for p in range(0, len(bad_text), 4096)]
    members[40] = IC.member(b'\x07', 4096)                                      # ... and a corrupt member far behind it
    offset = sum(len(m) for m in members[:40])
    with make() as eng:
        _feed_bgzf(eng, b''.join(members), [])
        assert _refusal(eng, result) == PREFIX % (offset, IC.WHAT[IC.BLOCK_TYPE])
    with make() as eng:                                                          # the corrupt member is the call's last: the plan meets it
        with pytest.raises(_lib.SegmentorError) as e:
            eng.feed_bgzf(b''.join(members[:41]))
        assert e.value.msg == PREFIX % (offset, IC.WHAT[IC.BLOCK_TYPE])
    with make() as eng:
        eng.feed(text[:at])
        with pytest.raises(_lib.SegmentorError, match='cannot be mixed'):
            eng.feed_bgzf(members[0])
    with make() as eng:
        eng.feed_bgzf(members[0])
        with pytest.raises(_lib.SegmentorError, match='cannot be mixed'):
            eng.feed(text[:at])
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    with make() as eng:
        with pytest.raises(_lib.SegmentorError, match='at file offset %d is gzip but not BGZF' % len(members[0])):
            eng.feed_bgzf(members[0] + c.compress(text[:1000]) + c.flush())


# ---- the commands ------------------------------------------------------------------------------------------------------------------------
def test_pat2beta_cli_device_inflate(pat_golden, tmp_path, capfd):              # noqa: F811
    spec = pat_golden['small']['spec']
    lines = synth.synth_pat_lines(spec['seed'], spec['n_sites'], spec['n_reads'])
    ref = synth.write_genome(str(tmp_path / 'references' / 'g'), ['chr1'], [spec['n_sites']], (np.arange(spec['n_sites']) * 37 + 100).astype(np.uint32))
    text = ('\n'.join(lines) + '\n\n').encode()
    pat = str(tmp_path / 'smp.pat.gz')
    homog.write_bgzf(pat, text, 4)
    out = {}
    for mode in ('host', 'device'):
        d = tmp_path / mode
        d.mkdir()
        assert wgbs_tools.main(['wgbstools', 'pat2beta', pat, '-o', str(d), '--genome', ref, '-f', '--inflate', mode]) == 0
        out[mode] = open(str(d / 'smp.beta'), 'rb').read()
    assert out['device'] == out['host'] and len(out['host']) == 2 * spec['n_sites']
    assert hashlib.sha1(out['device']).hexdigest() == pat_golden['small']['beta_sha1']
    assert 'not BGZF' not in capfd.readouterr().err
    # a plain-gzip file takes the host path and says so
    plain = str(tmp_path / 'plain.pat.gz')
    with gzip.open(plain, 'wb') as f:
        f.write(text)
    assert wgbs_tools.main(['wgbstools', 'pat2beta', plain, '-o', str(tmp_path), '--genome', ref, '-f', '--inflate', 'device']) == 0
    assert open(str(tmp_path / 'plain.beta'), 'rb').read() == out['host']
    err = capfd.readouterr().err
    assert err.count('is not BGZF: --inflate device does not apply, inflating on the host') == 1
    # a truncated file is refused with the offset of the member that is cut
    data = open(pat, 'rb').read()
    cut = str(tmp_path / 'cut.pat.gz')
    with open(cut, 'wb') as f:
        f.write(data[:len(data) - 40])
    last = [r[4] for r in walk_restated(data)[0]][-2]
    assert wgbs_tools.main(['wgbstools', 'pat2beta', cut, '-o', str(tmp_path), '--genome', ref, '-f', '--inflate', 'device']) == 1
    assert 'truncated (the BGZF member at file offset %d is incomplete)' % last in capfd.readouterr().err
    assert not op.exists(str(tmp_path / 'cut.beta'))


def test_homog_cli_device_inflate(tmp_path):
    case = HC.CASES['long_reads_signed']
    pat = str(tmp_path / 'smp.pat.gz')
    homog.write_bgzf(pat, HC.case_pat(case['pat']), 4)
    blocks = tmp_path / 'blocks.bed'
    blocks.write_text(HC.case_blocks(case['blocks'])[2])
    out = {}
    for mode in ('host', 'device'):
        d = tmp_path / mode
        d.mkdir()
        assert wgbs_tools.main(['wgbstools', 'homog', pat, '-b', str(blocks), '-o', str(d), '--binary', '--inflate', mode] + case['args']) == 0
        out[mode] = open(str(d / 'smp.uxm'), 'rb').read()
    assert out['device'] == out['host'] and any(out['host'])


def test_bimodal_cli_device_inflate(tmp_path, capsys):
    case = BC.CASES['L_default']
    pat_text, bed_text, args = BC.case_inputs(case)
    g = str(tmp_path / 'g')
    BC.write_genome(g)
    pat = str(tmp_path / 'smp.pat.gz')
    homog.write_bgzf(pat, pat_text, 4)
    bed = tmp_path / 'blocks.bed'
    bed.write_text(bed_text)
    out = {}
    for mode in ('host', 'device'):
        capsys.readouterr()
        assert wgbs_tools.main(['wgbstools', 'test_bimodal', pat, '--genome', g, '-L', str(bed), '--inflate', mode] + args) == 0
        out[mode] = capsys.readouterr().out
    assert out['device'] == out['host'] and out['host'].count('\n') > 3
