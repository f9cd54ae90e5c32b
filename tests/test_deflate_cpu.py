"""The DEFLATE encoder and the BGZF write plan without a GPU: csrc/deflate_core.h's serial host twin against zlib — every member of
tests/deflate_cases.py inflates to its text by zlib.decompress(payload, -15), by gzip and by the project's own decoder, CRC32 and ISIZE
are zlib's, no member passes its stored form, and BED lines come within 10 % of zlib level 1 — then the length builder alone, the CRC
shares, csrc/deflate_plan.h's cut, bound and refusals, and the command lines' refusals.  The case list then runs through a stand-alone
program (tests/native/san_deflate.cpp) built plain and with AddressSanitizer + UndefinedBehaviorSanitizer.
tests/test_gpu_deflate.py asks the device for the same bytes."""
import ctypes as C
import gzip
import heapq
import os.path as op
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import deflate_cases as DC
import inflate_cases as IC

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(HERE)
CSRC = op.join(ROOT, 'wgbs_tools_amd', 'csrc')
SRC = op.join(HERE, 'native', 'deflate_host.cpp')
LIB = op.join(HERE, 'native', 'libdeflate_host.so')
DEPS = [SRC, op.join(ROOT, 'include', 'wgbsseg.h')] + [op.join(CSRC, h) for h in ('deflate_core.h', 'deflate_plan.h', 'inflate_core.h', 'block_plan.h')]
OK, E_ARG, E_CAPACITY = 0, -1, -6


@pytest.fixture(scope='module')
def L():
    """tests/native/libdeflate_host.so (built when missing or older than its sources)"""
    if not op.isfile(LIB) or op.getmtime(LIB) < max(op.getmtime(d) for d in DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', SRC, '-o', LIB])
    lib = C.CDLL(LIB)
    lib.deflate_twin.argtypes = [C.c_char_p, C.c_uint32, C.c_char_p]
    lib.deflate_twin.restype = C.c_uint32
    lib.deflate_inflate_twin.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_uint32]
    lib.deflate_crc_shares.argtypes = [C.c_char_p, C.c_uint32, C.c_int]
    lib.deflate_crc_shares.restype = C.c_uint32
    lib.deflate_plan.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_char_p, C.c_size_t]
    lib.deflate_lengths.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.deflate_lengths.restype = None
    for f in (lib.deflate_bound, lib.deflate_members):
        f.argtypes, f.restype = [C.c_int64], C.c_int64
    lib.deflate_member_len.argtypes, lib.deflate_member_len.restype = [C.c_int64, C.c_int64], C.c_uint32
    lib.deflate_eof.argtypes = [C.c_char_p]
    lib.deflate_first_block_depth.argtypes = [C.c_char_p, C.c_int64, C.c_int]
    return lib


def twin(L, text):
    """the host twin's member of a text"""
    out = C.create_string_buffer(len(text) + 31)
    n = L.deflate_twin(text, len(text), out)
    assert n <= len(text) + 31
    return out.raw[:n]


@pytest.fixture(scope='module')
def members(L):
    """name -> (text, member), encoded once"""
    return {name: (text, twin(L, text)) for name, text in DC.cases()}


# ---- the host twin against zlib -------------------------------------------------------------------------------------------------------------
def test_every_case_inflates_to_its_text(L, members):
    assert len(members) == len(DC.cases()) >= 30
    eof = C.create_string_buffer(28)
    L.deflate_eof(eof)
    assert eof.raw == IC.EOF_MEMBER and gzip.decompress(eof.raw) == b''
    for name, (text, member) in members.items():
        payload, crc, isize = DC.split(member)
        assert zlib.decompress(payload, -15) == text, name
        assert (crc, isize) == (zlib.crc32(text), len(text)), name
        assert gzip.decompress(member + eof.raw) == text, name
        back = C.create_string_buffer(max(len(text), 1))
        assert L.deflate_inflate_twin(payload, len(payload), back, len(text)) == IC.OK and back.raw[:len(text)] == text, name
        assert len(payload) <= len(text) + 5, name                               # never larger than its stored form
    everything = b''.join(m for _t, m in members.values()) + eof.raw
    assert gzip.decompress(everything) == b''.join(t for t, _m in members.values())
    assert [DC.split(m)[2] for m in DC.walk(everything)] == [len(t) for t, _m in members.values()] + [0]


def test_shapes_the_cases_are_there_for(L, members):
    size = {name: len(m) - 26 for name, (_t, m) in members.items()}
    for n in (65279, 65280):
        assert size['%d random bytes' % n] == n + 5                              # the stored fallback, and 18 + 65285 + 8 <= 65536
    assert size['one byte x 65280'] < 400 and size['period 2'] < 100 and size['period 3'] < 100      # chains of the longest match
    assert size['0 bytes'] == 2 and size['1 bytes'] == 3
    # the string 32768 back is matched, the one 32769 back is not (its 100 bytes are coded as literals): zlib, which refuses a distance
    # beyond the window, has inflated both
    assert size['repeat at 32769, run filler'] > size['repeat at 32768, run filler'] + 60
    text, member = members['code-length code past 7 bits']
    payload = DC.split(member)[0]
    cl, freq = DC.code_length_counts(payload)
    assert _huffman_cost(freq)[1] > 7 and max(cl) == 7                           # Huffman alone would go deeper: the code-length code sits at its cap
    assert L.deflate_first_block_depth(payload, len(payload), 1) == 7
    for name in ('fibonacci over 22 symbols', 'fibonacci over 17 symbols'):
        payload = DC.split(members[name][1])[0]
        assert 9 <= L.deflate_first_block_depth(payload, len(payload), 0) <= 15, name


def test_size_condition_on_bed_lines(L):
    """The twin's total payload over BED lines cut at 65280 is at most 1.10 x zlib level 1's over the same cut (the condition comes from a
    serial restatement of the rule, which gave 0.357 of the text against zlib level 1's 0.365 on synthetic beta2bed lines; the margin covers
    real Huffman codes against entropy and another text)."""
    text = DC.bed_text()
    assert len(text) >= 2 * 1000 * 1000
    ours = ref = 0
    for p in range(0, len(text), DC.MEMBER):
        piece = text[p:p + DC.MEMBER]
        member = twin(L, piece)
        assert zlib.decompress(DC.split(member)[0], -15) == piece
        ours += len(member) - 26
        ref += len(DC.zlib1(piece))
    print('twin %d bytes, zlib level 1 %d bytes, ratio %.4f, of the text %.4f' % (ours, ref, ours / ref, ours / len(text)))
    assert ours <= 1.10 * ref


# ---- the length builder -----------------------------------------------------------------------------------------------------------------------
def _lengths(L, freq, limit, two=False):
    f = np.ascontiguousarray(freq, dtype=np.uint32)
    lens = np.full(f.size, 99, dtype=np.uint8)
    L.deflate_lengths(f.ctypes.data, f.size, limit, lens.ctypes.data, int(two))
    return lens


def _huffman_cost(freq):
    """the bits of an unlimited Huffman code, and its depth"""
    heap = [(int(f), 0) for f in freq if f]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return cost, heap[0][1]


def test_length_builder_limits_and_stays_complete(L):
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    rng = np.random.default_rng(3)
    tried = [(fib[:22], 15), (fib[:17], 15), (fib[:16], 15), (fib[:19], 7), (fib[:9], 7), (fib[:8], 7), ([5] * 286, 15), ([1] * 19, 7)]
    tried += [(rng.integers(0, 50, 286).tolist(), 15) for _ in range(5)] + [((rng.integers(0, 3, 30) * rng.integers(1, 4000, 30)).tolist(), 15) for _ in range(5)]
    tried += [(rng.permutation(fib[:20] + [0] * 200).tolist(), 15), (rng.permutation(fib[:15] + [0] * 4).tolist(), 7)]
    limited = 0
    for freq, limit in tried:
        lens = _lengths(L, freq, limit)
        f = np.asarray(freq)
        assert ((lens > 0) == (f > 0)).all() and lens.max() <= limit
        assert sum(2.0 ** -int(l) for l in lens if l) == 1.0                     # complete: neither over-subscribed nor with a code to spare
        best, depth = _huffman_cost(freq)
        cost = int((f * lens).sum())
        if depth <= limit:
            assert cost == best                                                  # Huffman's own lengths where they fit
        else:
            limited += 1
            assert best < cost <= 1.05 * best + 8
    assert limited >= 4
    assert _lengths(L, [0, 0, 7, 0], 15).tolist() == [0, 0, 1, 0]               # one symbol alone: one bit (an incomplete code the decoder allows)
    assert _lengths(L, [0, 0, 7, 0], 7, two=True).tolist() == [1, 0, 1, 0]      # the code-length code gets the other 1-bit code too
    assert _lengths(L, [7, 0, 0, 0], 7, two=True).tolist() == [1, 1, 0, 0]
    assert _lengths(L, [0, 0, 0], 15).tolist() == [0, 0, 0]


def test_crc_of_64_shares_is_zlibs(L):
    rng = np.random.default_rng(4)
    for n in (0, 1, 63, 64, 65, 1000, 4099, 65279, 65280):
        text = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for lanes in (1, 2, 64):
            assert L.deflate_crc_shares(text, n, lanes) == zlib.crc32(text), (n, lanes)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
def _plan(L, n, cap, waves=3):
    info = np.full(4, -7, dtype=np.int64)
    msg = C.create_string_buffer(400)
    rc = L.deflate_plan(n, cap, waves, info.ctypes.data, msg, 400)
    return rc, msg.value.decode(), info.tolist()


def test_cut_bound_and_refusals(L):
    for n in (0, 1, 65279, 65280, 65281, 2 * 65280, 10 ** 6, 791 * 10 ** 6):
        members = -(-n // 65280)
        assert L.deflate_members(n) == members
        lens = [L.deflate_member_len(n, i) for i in {0, 1, members - 2, members - 1, members} if i >= 0]
        assert all(0 <= x <= 65280 for x in lens)
        assert sum(L.deflate_member_len(n, i) for i in range(min(members, 40))) == min(n, 40 * 65280)
        assert L.deflate_member_len(n, members) == 0 and (members == 0 or L.deflate_member_len(n, members - 1) == n - (members - 1) * 65280)
        bound = n + 31 * members + 28
        assert L.deflate_bound(n) == bound
        assert _plan(L, n, bound) == (OK, '', [members, members * 65344, bound, -(-members // 3)])
        rc, msg, _info = _plan(L, n, bound - 1)
        assert rc == E_CAPACITY and msg == 'bgzf_deflate: room for %d bytes, %d bytes of text may need %d (wgbsseg_bgzf_deflate_bound)' % (bound - 1, n, bound)
    assert _plan(L, -1, 100)[:2] == (E_ARG, 'bad arguments to bgzf_deflate')
    assert _plan(L, 10, -1)[:2] == (E_ARG, 'bad arguments to bgzf_deflate')
    assert 65344 % 64 == 0 and 65344 >= 18 + 65280 + 5 + 8 + 20


def test_command_lines_refuse_what_they_cannot_do(tmp_path, capsys):
    from wgbs_tools_amd import beta2bed, homog
    from wgbs_tools_amd.genome import IllegalArgumentError
    for opath in (None, '/dev/stdout', str(tmp_path / 'x.bed')):
        with pytest.raises(IllegalArgumentError, match='--deflate device compresses the output on the GPU: give -o a path that ends in .gz'):
            beta2bed.check_deflate('device', opath)
    beta2bed.check_deflate('device', str(tmp_path / 'x.bed.gz'))
    beta2bed.check_deflate('host', None)
    with pytest.raises(IllegalArgumentError, match="deflate must be 'host' or 'device'"):
        beta2bed.check_deflate('gpu', 'x.gz')
    assert beta2bed.parse_args(['a.beta']).deflate == 'host' and beta2bed.parse_args(['a.beta', '--deflate', 'device']).deflate == 'device'
    with pytest.raises(SystemExit):
        beta2bed.parse_args(['a.beta', '--deflate', 'gpu'])
    with pytest.raises(IllegalArgumentError, match="deflate must be 'host' or 'device'"):
        homog.write_bgzf(str(tmp_path / 'y.gz'), b'abc', deflate='gpu')
    # the default of homog's writer is what it was: zlib's members
    homog.write_bgzf(str(tmp_path / 'y.gz'), b'abc\n' * 30000)
    assert gzip.open(str(tmp_path / 'y.gz')).read() == b'abc\n' * 30000
    capsys.readouterr()


# ---- the shared core under the sanitizers ------------------------------------------------------------------------------------------------
def _have_sanitizers():
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null', '-fsanitize=address,undefined'], input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason='no g++ with sanitizer runtimes')
def test_case_list_under_sanitizers(L, members, tmp_path):
    """plain and sanitised builds print the same lines, which are the library's answers; exit status 0 and an empty stderr say that no
    read or write left its array"""
    path = str(tmp_path / 'texts.bin')
    DC.write_texts(path, [t for t, _m in members.values()])
    outs = {}
    for name, flags in (('plain', []), ('asan_ubsan', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exe = str(tmp_path / ('san_deflate_' + name))
        subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-I', CSRC, op.join(HERE, 'native', 'san_deflate.cpp'), '-o', exe] + flags)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env={'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'})
        assert r.returncode == 0 and r.stderr == '', r.stderr[-3000:]
        outs[name] = r.stdout
    assert outs['plain'] == outs['asan_ubsan']
    lines = outs['plain'].splitlines()
    assert lines[-1] == 'records: %d, back: %d' % (len(members), len(members))
    for k, (text, member) in enumerate(members.values()):
        assert lines[k].startswith('%d: %d -> %d ' % (k, len(text), len(member))) and lines[k].endswith(' back 1')
