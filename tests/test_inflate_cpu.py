"""The DEFLATE decoder and the BGZF plan without a GPU: csrc/inflate_core.h's serial host twin against zlib.decompress(payload, -15) —
the valid list, one hand-made stream per rule of the decoder's list, random single-byte corruptions — and csrc/inflate_plan.h's member
walk and line rule against a Python restatement, both through their host build (tests/native/inflate_host.cpp).  The corrupt corpus
then runs through a stand-alone program (tests/native/san_inflate.cpp) built with AddressSanitizer + UndefinedBehaviorSanitizer: the
core shared with the device reads and writes inside its bounds.  tests/test_gpu_inflate.py asks the device for the same answers."""
import ctypes as C
import os.path as op
import shutil
import subprocess
import time
import zlib

import numpy as np
import pytest

import inflate_cases as IC
from wgbs_tools_amd import homog

HERE = op.dirname(op.abspath(__file__))
ROOT = op.dirname(HERE)
CSRC = op.join(ROOT, 'wgbs_tools_amd', 'csrc')
SRC = op.join(HERE, 'native', 'inflate_host.cpp')
LIB = op.join(HERE, 'native', 'libinflate_host.so')
DEPS = [SRC, op.join(ROOT, 'include', 'wgbsseg.h')] + [op.join(CSRC, h) for h in ('inflate_core.h', 'inflate_plan.h', 'block_plan.h')]
OK, E_ARG = 0, -1
P = C.c_void_p


@pytest.fixture(scope='module')
def L():
    """tests/native/libinflate_host.so (built when missing or older than its sources)"""
    if not op.isfile(LIB) or op.getmtime(LIB) < max(op.getmtime(d) for d in DEPS):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', SRC, '-o', LIB])
    lib = C.CDLL(LIB)
    lib.inflate_twin.argtypes = [C.c_char_p, C.c_int64, C.c_char_p, C.c_uint32]
    lib.inflate_what.restype = C.c_char_p
    lib.inflate_first_block_depth.argtypes = [C.c_char_p, C.c_int64]
    lib.inflate_walk.argtypes = [C.c_char_p, C.c_int64, C.c_uint64, P, C.c_int64, P, P, C.c_char_p, C.c_size_t]
    lib.inflate_plan.argtypes = [C.c_char_p, C.c_int64, C.c_uint64, C.c_char_p, C.c_int64, P, C.c_int64, P, C.c_char_p, C.c_int64, C.c_char_p, C.c_size_t]
    return lib


def twin(L, payload, isize):
    """(reason, text) of the host twin"""
    out = C.create_string_buffer(max(isize, 1))
    rc = L.inflate_twin(payload, len(payload), out, isize)
    return rc, out.raw[:isize]


# ---- the host twin against zlib -------------------------------------------------------------------------------------------------------
def test_twin_inflates_what_zlib_wrote(L):
    cases = IC.valid_cases()
    assert len(cases) >= 17
    for name, payload, text in cases:
        assert twin(L, payload, len(text)) == (IC.OK, text), name
    fib = [payload for name, payload, _t in cases if name == '15-bit literal code'][0]
    assert L.inflate_first_block_depth(fib, len(fib)) == 15                 # the member does reach the deepest code DEFLATE allows


def test_reason_texts(L):
    assert [L.inflate_what(c).decode() for c in range(16)] == IC.WHAT


def test_every_rule_broken_once(L):
    cases = IC.handmade_cases()
    assert {why for _n, _p, _i, why, _a in cases} == set(range(16))          # every reason of the decoder is met, and "no error" on the accepted sides
    for name, payload, isize, why, accepted in cases:
        rc, text = twin(L, payload, isize)
        assert rc == why, (name, rc, IC.WHAT[rc])
        z = IC.zlib_text(payload)
        assert (z is not None) == accepted, name
        if rc == IC.OK:
            assert text == z, name
        elif accepted:
            assert rc in (IC.OUT_BIG, IC.OUT_SMALL) and len(z) != isize, name    # zlib takes the stream; the member's ISIZE is wrong


def _against_zlib(L, payload, isize):
    """the twin refuses, or returns what zlib returns; it refuses wherever zlib raises.  True when it accepted."""
    z = IC.zlib_text(payload)
    rc, text = twin(L, payload, isize)
    if z is None:
        assert rc != IC.OK, payload[:40]
        return False
    if rc == IC.OK:
        assert text == z
        return True
    assert rc in (IC.OUT_BIG, IC.OUT_SMALL) and len(z) != isize, (rc, payload[:40])
    return False


def test_corpus_against_zlib(L):
    took = sum(_against_zlib(L, payload, isize) for _name, payload, isize in IC.corpus())
    assert took > 50                                                         # (corruptions that only change the text)


def test_random_corruptions_for_a_few_seconds(L):
    seed = int(time.time())
    print('seed', seed)
    rng = np.random.default_rng(seed)
    texts = [IC.pat_text(rng, 20000), rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), IC.fibonacci_bytes()[:9000], b'\n' * 600 + b'abc' * 500]
    t0, ran, took = time.time(), 0, 0
    while time.time() - t0 < 3.0:
        text = texts[int(rng.integers(0, len(texts)))][:int(rng.choice([40, 700, 20000]))]
        payload = bytearray(IC.deflate(text, int(rng.choice([0, 1, 6, 9])), int(rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY]))))
        for _ in range(int(rng.choice([1, 1, 2]))):
            payload[int(rng.integers(0, min(len(payload), rng.choice([6, 60, 10 ** 6]))))] = int(rng.integers(0, 256))
        if rng.random() < 0.1:
            del payload[int(rng.integers(1, len(payload) + 1)):]
        z = IC.zlib_text(bytes(payload))
        took += _against_zlib(L, bytes(payload), min(65536, len(text) if z is None else len(z)))
        ran += 1
    assert ran > 100 and took > 0


# ---- the member walk and the line rule -------------------------------------------------------------------------------------------------
def walk(L, data, base=0):
    rows = np.full((max(1, len(data) // 26 + 1), 5), -7, dtype=np.int64)
    n, used = C.c_int64(-7), C.c_int64(-7)
    msg = C.create_string_buffer(600)
    rc = L.inflate_walk(data, len(data), base, rows.ctypes.data, rows.shape[0], C.addressof(n), C.addressof(used), msg, 600)
    return rc, msg.value.decode(), rows[:n.value].tolist(), used.value


def walk_restated(data, base=0):
    """rows of (in_off, in_len, isize, out_off, file_off) of the whole members of data, and the bytes they take"""
    rows, pos, out = [], 0, 0
    while len(data) - pos >= 12:
        xlen = int.from_bytes(data[pos + 10:pos + 12], 'little')
        extra = data[pos + 12:pos + 12 + xlen]
        if len(extra) < xlen:
            break
        q, size = 0, None
        while q + 4 <= xlen:
            slen = int.from_bytes(extra[q + 2:q + 4], 'little')
            if extra[q:q + 2] == b'BC' and slen == 2:
                size = int.from_bytes(extra[q + 4:q + 6], 'little') + 1
                break
            q += 4 + slen
        if size is None or pos + size > len(data):
            break
        isize = int.from_bytes(data[pos + size - 4:pos + size], 'little')
        rows.append([pos + 12 + xlen, size - 12 - xlen - 8, isize, out, base + pos])
        out += isize
        pos += size
    return rows, pos


def _sized_member(rng, n):
    text = IC.pat_text(rng, n + 100)[:n]
    return IC.member(IC.deflate(text), len(text)), text


def test_walk_matches_restatement(L, tmp_path):
    rng = np.random.default_rng(5)
    text = IC.pat_text(rng, 200000)
    path = str(tmp_path / 'a.pat.gz')
    homog.write_bgzf(path, text)
    files = [open(path, 'rb').read(), IC.bgzf(text[:5000], block=300), IC.EOF_MEMBER, b'']
    parts = [_sized_member(rng, n) for n in (300, 4096, 65280)]
    files.append(b''.join(m for m, _t in parts) + IC.EOF_MEMBER)
    # other subfields around BC: before it, after it, both; an odd-sized one; one that is called BC but is not 2 bytes long
    t = text[:700]
    files.append(IC.member(IC.deflate(t), len(t), extra_before=IC.subfield(65, 66, b'xyz')) + IC.member(IC.deflate(t), len(t), extra_after=IC.subfield(1, 2, b'')) +
                 IC.member(IC.deflate(t), len(t), extra_before=IC.subfield(66, 67, b'abc') + IC.subfield(9, 9, b'1234567'), extra_after=IC.subfield(7, 7, b'\x00' * 40)))
    for data in files:
        want_rows, want_used = walk_restated(data, 1000)
        assert walk(L, data, 1000) == (OK, '', want_rows, want_used)
        assert want_used == len(data)
        for row in want_rows:                                                   # the payloads are where the table says
            assert zlib.decompress(data[row[0]:row[0] + row[1]], -15) is not None and row[2] <= 65536
    # a trailing partial member is left to the caller, wherever the bytes end
    whole = files[4]
    sizes = np.cumsum([0] + [len(m) for m, _t in parts] + [len(IC.EOF_MEMBER)])
    for cut in sorted({1, 2, 11, 12, 17, 18, 30, len(whole) - 1} | {int(s) + d for s in sizes for d in (-1, 0, 1, 5, 12, 18) if 0 < int(s) + d <= len(whole)}):
        rc, msg, rows, used = walk(L, whole[:cut])
        want_rows, want_used = walk_restated(whole[:cut])
        assert (rc, msg, rows, used) == (OK, '', want_rows, want_used), cut
        assert used == max(int(s) for s in sizes if s <= cut)


def test_walk_refusals_name_the_file_offset(L):
    rng = np.random.default_rng(6)
    good, text = _sized_member(rng, 500)
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    plain = c.compress(text) + c.flush()                                         # gzip, not BGZF: no extra field
    assert walk(L, good + plain, 7000)[:2] == (E_ARG, 'Invalid gzip data: the member at file offset %d is gzip but not BGZF (no extra field)' % (7000 + len(good)))
    other = bytearray(good)
    other[12:14] = b'XY'                                                         # an extra field without BC
    assert walk(L, good + bytes(other), 0)[:2] == (E_ARG, 'Invalid gzip data: the member at file offset %d is gzip but not BGZF (no BC subfield)' % len(good))
    assert walk(L, good + b'junk' * 10, 50)[:2] == (E_ARG, 'Invalid gzip data: no gzip member at file offset %d' % (50 + len(good)))
    small = bytearray(good)
    small[16:18] = (20).to_bytes(2, 'little')                                    # BSIZE points inside the member's own header and trailer
    assert walk(L, good + bytes(small) + good, 0)[:2] == (E_ARG, 'Invalid gzip data: BGZF member at file offset %d: BSIZE 20 is less than its header and trailer' % len(good))
    big = bytearray(good)
    big[-4:] = (65537).to_bytes(4, 'little')
    assert walk(L, good + bytes(big), 9)[:2] == (E_ARG, 'Invalid gzip data: BGZF member at file offset %d: ISIZE 65537 > 65536' % (9 + len(good)))
    edge = bytearray(good)
    edge[-4:] = (65536).to_bytes(4, 'little')
    assert walk(L, bytes(edge), 0)[0] == OK


def plan(L, data, carry=b'', base=0):
    rows = np.full((max(1, len(data) // 26 + 1), 5), -7, dtype=np.int64)
    info = np.full(8, -7, dtype=np.int64)
    new = C.create_string_buffer(len(data) * 0 + 70000 * max(1, rows.shape[0]) + len(carry) + 1)
    msg = C.create_string_buffer(600)
    rc = L.inflate_plan(data, len(data), base, carry, len(carry), rows.ctypes.data, rows.shape[0], info.ctypes.data, new, len(new), msg, 600)
    keys = ('members', 'consumed', 'n_dev', 'comp_bytes', 'carry_in', 'text_cap', 'n_text')
    return rc, msg.value.decode(), dict(zip(keys, info[:7].tolist())), rows[:max(info[0], 0)].tolist(), new.raw[:max(info[7], 0)]


def feed_restated(L, data, cuts):
    """the chunks an engine's kernels see when `data` is fed in pieces cut at `cuts`: per call the plan, the device's text (carry + the
    text of the first n_dev members, by zlib) up to n_text, and the carry kept; at the end the carry with a newline"""
    chunks, carry, tail, base = [], b'', b'', 0
    for a, b in zip([0] + cuts, cuts + [len(data)]):
        buf = tail + data[a:b]
        rc, msg, info, rows, new = plan(L, buf, carry, base)
        assert (rc, msg) == (OK, '')
        device = carry + b''.join(zlib.decompress(buf[r[0]:r[0] + r[1]], -15) for r in rows[:info['n_dev']])
        assert info['carry_in'] == len(carry)
        if info['n_dev']:
            assert info['text_cap'] == len(device) and len(carry) < info['n_text'] <= len(device)
        else:                                                                   # no newline in the call: nothing goes to the device
            assert info['text_cap'] == 0 and info['n_text'] == 0
        assert [r[3] for r in rows[:info['n_dev']]] == [len(carry) + sum(q[2] for q in rows[:i]) for i in range(info['n_dev'])]
        assert [r[4] for r in rows] == [base + r[0] - 18 for r in rows]          # (18-byte headers in these files)
        if info['n_dev']:
            last = rows[info['n_dev'] - 1]
            assert info['comp_bytes'] == last[0] + last[1] + 8
        chunk = device[:info['n_text']]
        assert chunk == b'' or chunk.endswith(b'\n')
        assert b'\n' not in new
        rest = b''.join(zlib.decompress(buf[r[0]:r[0] + r[1]], -15) for r in rows[info['n_dev']:])
        assert device[info['n_text']:] + rest == new if info['n_dev'] else carry + rest == new
        if chunk:
            chunks.append(chunk)
        carry, tail, base = new, buf[info['consumed']:], base + info['consumed']
    assert tail == b''
    if carry:
        chunks.append(carry + b'\n')
    return chunks


def test_carry_rule_over_lines_that_straddle_members_and_calls(L):
    rng = np.random.default_rng(8)
    long_line = b'chr1\t5\t' + b'CT' * 400 + b'\t1\n'                           # longer than a 300-byte member
    texts = {'pat': IC.pat_text(rng, 30000), 'long line': IC.pat_text(rng, 2000) + long_line + IC.pat_text(rng, 2000),
             'no final newline': IC.pat_text(rng, 5000)[:-1], 'no newline at all': b'x' * 1000, 'empty': b'', 'newlines only': b'\n' * 700}
    for name, text in texts.items():
        for block in (300, 4096, 65280):
            data = IC.bgzf(text, block=block)
            sizes = np.cumsum([r[1] + 26 for r in walk_restated(data)[0]]).tolist()
            for mode in ('whole', 'one member per call', 'random', 'anywhere'):
                if mode == 'whole':
                    cuts = []
                elif mode == 'one member per call':
                    cuts = sizes[:-1]
                elif mode == 'random':
                    cuts = sorted(set(rng.choice(sizes, max(1, len(sizes) // 3)).tolist()) - {len(data)})
                else:
                    cuts = sorted(set(rng.integers(1, len(data), 5).tolist()))  # calls that end inside a member
                chunks = feed_restated(L, data, cuts)
                want = text if text.endswith(b'\n') or not text else text + b'\n'
                assert b''.join(chunks) == want, (name, block, mode)


def test_plan_refuses_a_corrupt_member_it_inflates_itself(L):
    rng = np.random.default_rng(9)
    text = IC.pat_text(rng, 3000)
    good = IC.bgzf(text, block=1000, eof=False)
    rows = walk_restated(good)[0]
    bad = bytearray(good)
    bad[rows[-1][0]] = 0x07                                                      # the last member's first byte: block type 3
    rc, msg = plan(L, bytes(bad), b'', 400)[:2]
    assert (rc, msg) == (E_ARG, 'Invalid gzip data: BGZF member at file offset %d: invalid block type' % (400 + rows[-1][4]))


# ---- the shared core under the sanitizers ------------------------------------------------------------------------------------------------
def _have_sanitizers():
    if not shutil.which('g++'):
        return False
    r = subprocess.run(['g++', '-x', 'c++', '-', '-o', '/dev/null', '-fsanitize=address,undefined'], input='int main(){return 0;}', text=True, capture_output=True)
    return r.returncode == 0


@pytest.mark.skipif(not _have_sanitizers(), reason='no g++ with sanitizer runtimes')
def test_corrupt_corpus_under_sanitizers(L, tmp_path):
    """the corpus of test_gpu_inflate.py's corrupt list, the valid list appended: plain and sanitised builds print the same lines, which are
    the library's answers; exit status 0 and an empty stderr say that no read or write left its array"""
    cases = IC.corpus() + [(name, payload, len(text)) for name, payload, text in IC.valid_cases()]
    path = str(tmp_path / 'corpus.bin')
    IC.write_corpus(path, cases)
    outs = {}
    for name, flags in (('plain', []), ('asan_ubsan', ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])):
        exe = str(tmp_path / ('san_inflate_' + name))
        subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-I', CSRC, op.join(HERE, 'native', 'san_inflate.cpp'), '-o', exe] + flags)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env={'ASAN_OPTIONS': 'detect_leaks=1', 'PATH': '/usr/bin:/bin'})
        assert r.returncode == 0 and r.stderr == '', r.stderr[-3000:]
        outs[name] = r.stdout
    assert outs['plain'] == outs['asan_ubsan']
    lines = outs['plain'].splitlines()
    assert lines[-1].startswith('records: %d, refused: ' % len(cases))
    for k, (name, payload, isize) in enumerate(cases):
        rc, _text = twin(L, payload, isize)
        assert lines[k].startswith('%d: %d %s ' % (k, rc, IC.WHAT[rc])), name
        assert lines[k].endswith(' walked 1') or len(payload) + 26 > 65536, name


# ---- the option of a command that does not declare it itself ---------------------------------------------------------------------------
def test_dispatcher_takes_inflate_for_test_bimodal(monkeypatch):
    from wgbs_tools_amd import pat2beta, wgbs_tools
    assert wgbs_tools._take_inflate(['x.pat.gz', '--inflate', 'device', '-L', 'b.bed']) == (['x.pat.gz', '-L', 'b.bed'], 'device')
    assert wgbs_tools._take_inflate(['--inflate=host', 'x.pat.gz']) == (['x.pat.gz'], 'host')
    assert wgbs_tools._take_inflate(['x.pat.gz', '--strict']) == (['x.pat.gz', '--strict'], None)
    seen = []
    import types
    fake = types.SimpleNamespace(main=lambda args: seen.append((list(args), pat2beta._default_inflate)))
    import importlib
    real = importlib.import_module
    monkeypatch.setattr(importlib, 'import_module', lambda name, package=None: fake if name == '.test_bimodal' else real(name, package))
    assert wgbs_tools.main(['wgbstools', 'test_bimodal', 'x.pat.gz', '--inflate', 'device', '--strict']) == 0
    assert wgbs_tools.main(['wgbstools', 'test_bimodal', 'x.pat.gz', '--strict']) == 0
    assert seen == [(['x.pat.gz', '--strict'], 'device'), (['x.pat.gz', '--strict'], 'host')]
    assert pat2beta._default_inflate == 'host'                                  # (the block's choice ends with the block)
    assert wgbs_tools.main(['wgbstools', 'test_bimodal', 'x.pat.gz', '--inflate', 'gpu']) == 1
    assert wgbs_tools.main(['wgbstools', 'test_bimodal', 'x.pat.gz', '--inflate']) == 1
    with pytest.raises(Exception, match="inflate must be 'host' or 'device'"):
        with pat2beta.default_inflate('gpu'):
            pass
