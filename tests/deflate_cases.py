"""Texts for the DEFLATE encoder (csrc/deflate_core.h: the host twin in tests/test_deflate_cpu.py, k_bgzf_deflate in
tests/test_gpu_deflate.py): the smallest shapes at which an encoder goes wrong.  Every text is at most one member (65280 bytes).  The list
is built once per process and never changed."""
import functools
import zlib

import numpy as np

import bed_cases as BC
import bed_ref as BR
import inflate_cases as IC

MEMBER = 65280
HEAD, TAIL = 18, 8
SEED = 20261020


def far_repeat(dist, filler):
    """a 100-byte string at byte 0 and again `dist` bytes on.  filler 'random': random bytes between and behind (by then the table's slots
    of the string have been taken by nearer positions, mostly); 'run': one byte repeated, which takes one slot only, so the second copy's
    candidates ARE the first copy, `dist` back: matched at 32768, and at 32769 only a check of the distance keeps them out."""
    rng = np.random.default_rng(SEED + dist)
    s = rng.integers(1, 256, 100, dtype=np.uint8).tobytes()
    fill = (lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()) if filler == 'random' else (lambda n: b'\x00' * n)
    return s + fill(dist - 100) + s + fill(700)


def skewed(depths, rng):
    """a shuffled text in which as many byte values as depths[d] occur 2^(top - d) times: a Huffman code gives them d bits"""
    top = max(depths)
    values = rng.permutation(256)
    out, k = [], 0
    for d, count in sorted(depths.items()):
        for _ in range(count):
            out.append(bytes([int(values[k])]) * (1 << (top - d)))
            k += 1
    return bytes(rng.permutation(np.frombuffer(b''.join(out), dtype=np.uint8)))


def fibonacci_text(n_symbols, rng):
    a, b, out = 1, 1, []
    for v in range(n_symbols):
        out.append(bytes([65 + v]) * a)
        a, b = b, a + b
    return bytes(rng.permutation(np.frombuffer(b''.join(out), dtype=np.uint8)))


def bed_text():
    """BED lines of the synthetic genomes of tests/bed_cases.py by tests/bed_ref.py, a little over 2 MB"""
    w = BC.worlds()
    parts = []
    for world, f, opts in (('every_pair', 'every_pair.beta', dict(keep_na=True)), ('every_pair', 'every_pair.beta', dict(mean=True, keep_na=True)),
                           ('small', 'small.beta', dict()), ('small', 'small.lbeta', dict(mean=True, min_cov=2)), ('ties', 'ties.lbeta', dict(keep_na=True))):
        x = w[world]
        parts.append(BR.text_of(x['names'], x['sizes'], x['loci'], x['files'][f], 0, len(x['loci']), **opts))
    return b''.join(parts)


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, text)]"""
    rng = np.random.default_rng(SEED)
    noise = rng.integers(0, 256, MEMBER, dtype=np.uint8).tobytes()
    word = rng.integers(0, 256, 300, dtype=np.uint8).tobytes()
    out = [('%d bytes' % n, bytes(rng.integers(97, 123, n, dtype=np.uint8))) for n in (0, 1, 3, 4, 5, 63, 64, 65)]
    out += [('one byte x %d' % n, b'a' * n) for n in (258, 259, MEMBER)]
    out += [('period 2', b'ab' * 3000), ('period 3', b'abc' * 2101 + b'a')]
    out += [('%d random bytes' % n, noise[:n]) for n in (MEMBER - 1, MEMBER)]
    out += [('repeat at %d, %s filler' % (d, f), far_repeat(d, f)) for d in (32768, 32769) for f in ('random', 'run')]
    out += [('match up to the end', noise[:1000] + word + noise[1000:1500] + word[:137]),
            ('match cut by the end', b'xyzw' * 40 + noise[:64] + b'xyzw' * 3 + b'xy')]
    out += [('fibonacci over 22 symbols', IC.fibonacci_bytes()), ('fibonacci over 17 symbols', fibonacci_text(17, rng))]
    # values whose numbers per code length follow Fibonacci from 5 bits on: the code-length code sees those lengths with Fibonacci counts
    # (beside 0, the short lengths and the zero runs).  For this seed an unlimited Huffman code over the first block's code-length
    # symbols is 8 bits deep (code_length_counts below; tests/test_deflate_cpu.py asserts it), so the cap of 7 is at work.
    out += [('code-length code past 7 bits', skewed({1: 1, 2: 1, 3: 1, 5: 1, 6: 1, 7: 2, 8: 3, 9: 5, 10: 8, 11: 13, 12: 21, 13: 34}, np.random.default_rng(SEED + 10)))]
    out += [('one literal, no match', b'q' * 3), ('no distance code', bytes(rng.permutation(200).astype(np.uint8))),
            ('all 256 values', bytes(range(256))), ('all 256 values, twice', bytes(range(256)) * 2)]
    pat = IC.pat_text(rng, MEMBER + 500)
    bed = bed_text()
    out += [('pat text', pat[:MEMBER]), ('pat text, short', pat[:777]), ('bed lines', bed[:MEMBER]), ('bed lines, mean', bed[-MEMBER:]), ('bed lines, short', bed[:4099])]
    assert all(len(t) <= MEMBER for _n, t in out)
    return out


def split(member):
    """a BGZF member -> (payload, crc32, isize), its framing checked"""
    assert member[:16] == b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00'
    assert int.from_bytes(member[16:18], 'little') == len(member) - 1 and len(member) <= 65536
    return member[HEAD:-TAIL], int.from_bytes(member[-8:-4], 'little'), int.from_bytes(member[-4:], 'little')


def walk(data):
    """the members of a BGZF byte string, by their BSIZE; the walk must end at the last byte"""
    out, pos = [], 0
    while pos < len(data):
        size = int.from_bytes(data[pos + 16:pos + 18], 'little') + 1
        out.append(data[pos:pos + size])
        pos += size
    assert pos == len(data)
    return out


def code_length_counts(payload):
    """(the code-length code's lengths, how often the first block uses each of its 19 symbols) of a payload whose first block is dynamic"""
    bits = ''.join(format(b, '08b')[::-1] for b in payload[:900])
    pos = [0]

    def get(n):
        v = int(bits[pos[0]:pos[0] + n][::-1], 2) if n else 0
        pos[0] += n
        return v
    assert get(3) >> 1 == 2
    nl, nd, nc = get(5) + 257, get(5) + 1, get(4) + 4
    cl = [0] * 19
    for i in range(nc):
        cl[IC.CL_ORDER[i]] = get(3)
    codes, code = {}, 0
    for l in range(1, 8):
        for sym in range(19):
            if cl[sym] == l:
                codes[format(code, '0%db' % l)] = sym
                code += 1
        code <<= 1
    freq, n = [0] * 19, 0
    while n < nl + nd:
        c = ''
        while c not in codes:
            c += bits[pos[0]]
            pos[0] += 1
        sym = codes[c]
        freq[sym] += 1
        n += 1 if sym < 16 else 3 + get(2) if sym == 16 else 3 + get(3) if sym == 17 else 11 + get(7)
    return cl, freq


def zlib1(text):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    return c.compress(text) + c.flush()


def write_texts(path, texts):
    """records of {u32 bytes, text}: what tests/native/san_deflate.cpp reads"""
    with open(path, 'wb') as f:
        for t in texts:
            f.write(len(t).to_bytes(4, 'little') + t)
