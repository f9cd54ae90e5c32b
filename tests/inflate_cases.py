"""DEFLATE streams and BGZF members for the inflate tests (tests/test_inflate_cpu.py, tests/test_gpu_inflate.py): a list of valid
streams that zlib wrote, hand-made streams that break one rule of RFC 1951 each (or sit exactly on the accepted side of one), and
a deterministic list of single-byte corruptions.  A case is (name, payload, isize): a raw DEFLATE stream and the ISIZE its member
claims.  The yardstick for a payload is zlib.decompress(payload, -15)."""
import struct
import zlib

import numpy as np

# inflate_core.h's reasons
(OK, BLOCK_TYPE, STORED_LEN, TOO_MANY, CLEN_CODE, REPEAT_FIRST, REPEAT_OVER, NO_EOB, LIT_SET, DIST_SET, LIT_CODE, DIST_CODE, FAR, TRUNCATED,
 OUT_BIG, OUT_SMALL) = range(16)
WHAT = ['no error', 'invalid block type', 'invalid stored block lengths', 'too many length or distance symbols', 'invalid code lengths set',
        'invalid bit length repeat (no length before it)', 'invalid bit length repeat (past the last length)', 'invalid code -- missing end-of-block',
        'invalid literal/lengths set', 'invalid distances set', 'invalid literal/length code', 'invalid distance code', 'invalid distance too far back',
        'the compressed data end before the stream does', "more text than the member's ISIZE", "less text than the member's ISIZE"]


def zlib_text(payload):
    """what zlib makes of a raw DEFLATE stream: its text, or None where it raises"""
    try:
        return zlib.decompress(payload, -15)
    except zlib.error:
        return None


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=()):
    """raw DEFLATE of data; flushes: (offset, mode) pairs — zlib.Z_SYNC_FLUSH / Z_FULL_FLUSH after data[:offset]"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out, at = b'', 0
    for off, mode in flushes:
        out += c.compress(data[at:off]) + c.flush(mode)
        at = off
    return out + c.compress(data[at:]) + c.flush()


def member(payload, isize, extra_before=b'', extra_after=b'', crc=0):
    """a BGZF member around a raw DEFLATE stream: the 'BC' subfield, other subfields around it when asked for"""
    xlen = len(extra_before) + 6 + len(extra_after)
    size = 12 + xlen + len(payload) + 8
    assert size <= 65536
    return (b'\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff' + struct.pack('<H', xlen) + extra_before + b'BC\x02\x00' + struct.pack('<H', size - 1) +
            extra_after + payload + struct.pack('<II', crc, isize))


def subfield(a, b, data):
    return bytes([a, b]) + struct.pack('<H', len(data)) + data


EOF_MEMBER = member(b'\x03\x00', 0)


def bgzf(text, block=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, eof=True):
    """text as a BGZF byte string with `block` bytes of text per member"""
    out = [member(deflate(text[p:p + block], level, strategy), len(text[p:p + block]), crc=zlib.crc32(text[p:p + block])) for p in range(0, len(text), block)]
    return b''.join(out) + (EOF_MEMBER if eof else b'')


def pat_text(rng, n_bytes):
    """pat-like lines, about n_bytes of them (ends with a newline)"""
    lines, size, site = [], 0, 1
    while size < n_bytes:
        site += int(rng.integers(0, 40))
        k = int(rng.integers(1, 30))
        pattern = ''.join('CT.'[i] for i in rng.choice(3, k, p=[0.55, 0.35, 0.1]))
        line = 'chr%d\t%d\t%s\t%d\n' % (1 + site // 50000, site, pattern, int(rng.integers(1, 20)))
        lines.append(line)
        size += len(line)
    return ''.join(lines).encode()


def fibonacci_bytes():
    """bytes whose values have Fibonacci frequencies: a Huffman code over them is as deep as it can be.  22 values take 46367 bytes, and a
    code for them would be 21 bits deep; DEFLATE caps a code at 15 bits, so zlib's Z_HUFFMAN_ONLY member of this text uses the cap.
    (inflate_first_block_depth of the host twin reads 15 for it: tests/test_inflate_cpu.py asserts that.)"""
    a, b, out = 1, 1, []
    for v in range(22):
        out.append(bytes([65 + v]) * a)
        a, b = b, a + b
    text = b''.join(out)
    rng = np.random.default_rng(15)
    return bytes(rng.permutation(np.frombuffer(text, dtype=np.uint8)))


def valid_cases():
    """(name, payload, text) of streams zlib wrote"""
    rng = np.random.default_rng(20261019)
    pat = pat_text(rng, 65280)[:65280]
    noise = rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()
    half = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    out = []
    for level in (0, 1, 6, 9):
        out.append(('pat level %d' % level, deflate(pat, level), pat))
    for name, strategy in (('Z_FIXED', zlib.Z_FIXED), ('Z_RLE', zlib.Z_RLE), ('Z_HUFFMAN_ONLY', zlib.Z_HUFFMAN_ONLY)):
        out.append(('pat ' + name, deflate(pat, 6, strategy), pat))
    out.append(('sync and full flushes', deflate(pat, 6, flushes=[(1000, zlib.Z_SYNC_FLUSH), (1000, zlib.Z_SYNC_FLUSH), (30000, zlib.Z_FULL_FLUSH),
                                                                 (30001, zlib.Z_SYNC_FLUSH), (65000, zlib.Z_FULL_FLUSH)]), pat))
    out.append(('65280 random bytes', deflate(noise, 6), noise))
    out.append(('65280 random bytes stored', deflate(noise, 0), noise))
    out.append(('run of one byte', deflate(b'x' * 65280, 9), b'x' * 65280))
    out.append(('run of one byte, 300', deflate(b'\n' * 300, 6), b'\n' * 300))
    out.append(('second half repeats the first at 32768', far_repeat(half), half + half))
    fib = fibonacci_bytes()
    out.append(('15-bit literal code', deflate(fib, 6, zlib.Z_HUFFMAN_ONLY), fib))
    out.append(('empty', deflate(b''), b''))
    out.append(('one byte', deflate(b'a'), b'a'))
    out.append(('short periods', deflate(b''.join(bytes([97 + d]) + b'abcdefghijklmnopqrstuvwxyz'[:d] * 40 for d in range(1, 27)), 9),
                b''.join(bytes([97 + d]) + b'abcdefghijklmnopqrstuvwxyz'[:d] * 40 for d in range(1, 27))))
    for name, payload, text in out:
        assert zlib_text(payload) == text, name
    return out


# ---- hand-made streams --------------------------------------------------------------------------------------------------------------
class Bits:
    """a DEFLATE bit string: fields lowest bit first, Huffman codes highest bit first"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, bits):
        self.acc |= (value & ((1 << bits) - 1)) << self.n
        self.n += bits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, code, length):
        for i in range(length - 1, -1, -1):
            self.put((code >> i) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)
        return self

    def raw(self, data):
        self.align()
        self.out += data
        return self

    def bytes(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b'')


def canonical(lens):
    """{symbol: (code, length)} of the canonical Huffman code with these lengths (RFC 1951 3.2.2)"""
    out, code = {}, 0
    for length in range(1, 16):
        for sym, l in enumerate(lens):
            if l == length:
                out[sym] = (code, length)
                code += 1
        code <<= 1
    return out


# the code-length code the hand-made dynamic headers use: complete, and every length 0 .. 15 and every repeat has a code
CL_LENS = [5] * 16 + [2, 3, 3]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_header(b, lit_lens, dist_lens, final=1, hlit=None, hdist=None, cl_lens=None, symbols=None):
    """a dynamic block header into b.  symbols: the code-length symbols to send in place of one per length — (symbol, extra bits' value)"""
    cl = CL_LENS if cl_lens is None else cl_lens
    b.put(final, 1).put(2, 2)
    b.put((len(lit_lens) if hlit is None else hlit) - 257, 5).put((len(dist_lens) if hdist is None else hdist) - 1, 5).put(19 - 4, 4)
    for sym in CL_ORDER:
        b.put(cl[sym], 3)
    codes = canonical(cl)
    if symbols is None:
        symbols = [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    for sym, extra in symbols:
        b.code(*codes[sym])
        if sym >= 16:
            b.put(extra, {16: 2, 17: 3, 18: 7}[sym])
    return b


def lit_lens_of(pairs, n=257):
    lens = [0] * n
    for sym, l in pairs:
        lens[sym] = l
    return lens


def fixed_lit(b, v):
    if v < 144:
        return b.code(0x30 + v, 8)
    if v < 256:
        return b.code(0x190 + v - 144, 9)
    if v < 280:
        return b.code(v - 256, 7)
    return b.code(0xc0 + v - 280, 8)


def handmade_cases():
    """(name, payload, isize, the twin's reason, whether zlib accepts the payload): every rule of the decoder's list broken once, and the
    accepted side of the rules that have one"""
    out = []
    # a reference block: literals 'a', 'b' and the end of block with 2-bit codes; one distance code of 1 bit
    lits = lit_lens_of([(97, 2), (98, 2), (256, 2), (257, 2)], 258)               # complete: four codes of 2 bits
    lc = canonical(lits)
    ok = dynamic_header(Bits(), lits, [1]).code(*lc[97]).code(*lc[98]).code(*lc[257]).code(0, 1).code(*lc[256])
    out.append(('dynamic block, one distance code of 1 bit', ok.bytes(), 5, OK, True))                       # a b + (len 3, dist 1): abbbb
    out.append(('block type 3', Bits().put(1, 1).put(3, 2).bytes(), 0, BLOCK_TYPE, False))
    out.append(('stored LEN is not the complement of NLEN', Bits().put(1, 1).put(0, 2).align().put(3, 16).put(0xfffd, 16).raw(b'abc').bytes(), 3, STORED_LEN, False))
    out.append(('stored block, accepted', Bits().put(1, 1).put(0, 2).align().put(3, 16).put(0xfffc, 16).raw(b'abc').bytes(), 3, OK, True))
    out.append(('stored block cut short', Bits().put(1, 1).put(0, 2).align().put(3, 16).put(0xfffc, 16).raw(b'ab').bytes(), 3, TRUNCATED, False))
    out.append(('HLIT 287', dynamic_header(Bits(), lits, [1], hlit=287).bytes(), 0, TOO_MANY, False))
    out.append(('HDIST 31', dynamic_header(Bits(), lits, [1], hdist=31).bytes(), 0, TOO_MANY, False))
    out.append(('code-length code over-subscribed', dynamic_header(Bits(), lits, [1], cl_lens=[1, 1, 1] + [0] * 16).bytes(), 0, CLEN_CODE, False))
    out.append(('code-length code incomplete', dynamic_header(Bits(), lits, [1], cl_lens=[1] + [0] * 18, symbols=[]).bytes(), 0, CLEN_CODE, False))
    out.append(('repeat 16 with nothing before it', dynamic_header(Bits(), lits, [1], symbols=[(16, 0)]).bytes(), 0, REPEAT_FIRST, False))
    out.append(('repeat that overflows', dynamic_header(Bits(), lits, [1], symbols=[(0, 0), (18, 127), (18, 127)]).bytes(), 0, REPEAT_OVER, False))
    out.append(('no symbol 256', dynamic_header(Bits(), lit_lens_of([(97, 1), (98, 1)]), [1]).bytes(), 0, NO_EOB, False))
    out.append(('literal/length code over-subscribed', dynamic_header(Bits(), lit_lens_of([(97, 1), (98, 1), (256, 1)]), [1]).bytes(), 0, LIT_SET, False))
    out.append(('literal/length code incomplete, 2 bits', dynamic_header(Bits(), lit_lens_of([(97, 2), (256, 2)]), [1]).bytes(), 0, LIT_SET, False))
    one = lit_lens_of([(256, 1)])
    out.append(('literal/length code incomplete, 1 bit: accepted', dynamic_header(Bits(), one, [0]).code(0, 1).bytes(), 0, OK, True))
    out.append(('the unused code of a 1-bit literal/length code', dynamic_header(Bits(), one, [0]).code(1, 1).put(0, 16).bytes(), 0, LIT_CODE, False))
    out.append(('distance code over-subscribed', dynamic_header(Bits(), lits, [1, 1, 1]).bytes(), 0, DIST_SET, False))
    out.append(('distance code incomplete, 2 bits', dynamic_header(Bits(), lits, [2, 2]).bytes(), 0, DIST_SET, False))
    nodist = dynamic_header(Bits(), lits, [0]).code(*lc[97]).code(*lc[98])
    out.append(('no distance code, no match: accepted', _clone(nodist).code(*lc[256]).bytes(), 2, OK, True))
    out.append(('no distance code, a match', _clone(nodist).code(*lc[257]).put(0, 16).bytes(), 5, DIST_CODE, False))
    out.append(('symbol 286 of the fixed code', fixed_lit(Bits().put(1, 1).put(1, 2), 286).put(0, 16).bytes(), 0, LIT_CODE, False))
    far = fixed_lit(fixed_lit(Bits().put(1, 1).put(1, 2), 97), 257)
    out.append(('distance code 30 of the fixed code', _clone(far).code(30, 5).put(0, 16).bytes(), 4, DIST_CODE, False))
    out.append(('distance before the first byte', fixed_lit(_clone(far).code(1, 5), 256).bytes(), 4, FAR, False))
    out.append(('distance to the first byte: accepted', fixed_lit(_clone(far).code(0, 5), 256).bytes(), 4, OK, True))
    pat = b'chr1\t100\tCCTC\t3\nchr1\t104\tTTC.C\t1\n' * 40
    good = deflate(pat)
    out.append(('input ends before the final block', good[:-1], len(pat), TRUNCATED, False))
    out.append(('input ends in the header', good[:1], len(pat), TRUNCATED, False))
    out.append(('no input at all', b'', 0, TRUNCATED, False))
    out.append(('more text than ISIZE', good, len(pat) - 1, OUT_BIG, True))
    out.append(('less text than ISIZE', good, len(pat) + 1, OUT_SMALL, True))
    out.append(('bytes behind the final block: accepted', good + b'\xff\x00junk', len(pat), OK, True))
    for name, payload, isize, why, accepted in out:
        assert (zlib_text(payload) is not None) == accepted, name
    return out


def _clone(b):
    c = Bits()
    c.out, c.acc, c.n = bytearray(b.out), b.acc, b.n
    return c


def far_repeat(half):
    """half + half as a stored block and a fixed-code block of matches at distance 32768, the longest DEFLATE has (zlib itself never looks
    back further than 32506)"""
    assert len(half) == 32768
    b = Bits().put(0, 1).put(0, 2).align().put(32768, 16).put(32767, 16).raw(half).put(1, 1).put(1, 2)
    for _ in range(126):                                                        # 126 x 258 + 2 x 130 = 32768
        fixed_lit(b, 285).code(29, 5).put(8191, 13)
    for _ in range(2):
        fixed_lit(b, 280).put(15, 4).code(29, 5).put(8191, 13)
    return fixed_lit(b, 256).bytes()


def random_corruptions(n=300, seed=20261019):
    """(name, payload, isize): valid members of several makes with one byte changed, some also cut short.  isize: the length of zlib's text
    where zlib accepts the payload, of the original text otherwise."""
    rng = np.random.default_rng(seed)
    texts = [pat_text(rng, 6000), rng.integers(0, 256, 700, dtype=np.uint8).tobytes(), b'ab' * 900 + b'\n', fibonacci_bytes()[:4000]]
    out = []
    for k in range(n):
        text = texts[int(rng.integers(0, len(texts)))][:int(rng.choice([60, 300, 6000]))]
        payload = bytearray(deflate(text, int(rng.choice([0, 1, 6, 9])), int(rng.choice([zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY]))))
        at = int(rng.integers(0, min(len(payload), rng.choice([8, 40, 10 ** 6]))))
        payload[at] ^= int(rng.integers(1, 256))
        if rng.random() < 0.15:
            del payload[int(rng.integers(1, len(payload) + 1)):]
        payload = bytes(payload)
        got = zlib_text(payload)
        out.append(('corruption %d' % k, payload, len(text) if got is None else len(got)))
    return out


def corpus():
    """every stream the decoders are asked to refuse or accept byte for byte: (name, payload, isize), the hand-made ones first.  ISIZE is
    at most 65536 throughout (zlib's text of a corrupted stream can be longer than the original; such a case claims 65536)."""
    cases = [(name, payload, isize) for name, payload, isize, _why, _acc in handmade_cases()] + random_corruptions()
    return [(name, payload, min(isize, 65536)) for name, payload, isize in cases]


def write_corpus(path, cases):
    with open(path, 'wb') as f:
        for _name, payload, isize in cases:
            f.write(struct.pack('<II', len(payload), isize) + payload)
