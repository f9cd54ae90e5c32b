// inflate_core.h — the DEFLATE decoder (RFC 1951) of one BGZF member, once, for the host and the device (like bed_fmt.h and
// exact_log2.h): the bit reader, the stored / fixed / dynamic block headers, the code-length code, the canonical Huffman tables, the
// symbol decode, the length / distance tables and every validity check.  It accepts a stream where zlib's inflate with wbits = -15
// accepts it (zlib.decompress(payload, -15)): bytes behind the final block are ignored, CRC32 is not looked at.  On top of zlib's
// rules the text must be exactly ISIZE bytes long.
//
// What moves bytes is the caller's: an input `In` and an output `Out`.
//   In::word(w)            the payload's bytes [4 w, 4 w + 4) as a little-endian word, 0 for the bytes at and behind its end
//   In::byte(i)            payload byte i (asked for i < its length only)
//   In::lane(), lanes()    who runs this copy of the decoder and how many run it together (the host: 0 of 1; the device: a lane of its
//                          wave); only the fill of the lookup tables is shared out among them, and In::sync() follows it
//   In::uni(v)             v, which every copy running together holds alike (the device moves it to a scalar register, so that
//                          what is computed from it is scalar work and every branch on it is taken by the wave as a whole)
//   Out::pos()             bytes written so far
//   Out::lit(b)            one byte; Out::copy(dist, len): len bytes from dist back (dist <= pos()); Out::stored(in, off, len): len
//                          bytes of the payload from byte off.  Each returns 0, or WG_INF_OUT_BIG without writing when the text
//                          would pass ISIZE.
// inflate_member_host() below is the serial host twin; k_bgzf_inflate (inflate_kernels.h) is the device's.
//
// Bounds, by construction and not by trust in the data:
//   reads    the payload is read through In only; word() and byte() never touch a byte at or behind the payload's end, and every
//            bit handed out has been charged against 8 * n_in by drop() first.
//   writes   Out refuses whatever would pass ISIZE before writing it.
//   loops    every turn of a loop here drops at least one bit of the payload (a block header 3, a symbol >= 1, a code length >= 1) or
//            is counted by a field of at most 16 bits (a stored block's LEN, a repeat), so 8 * n_in + ISIZE bounds the work.
#pragma once
#include <cstdint>
#include <cstring>

#ifndef WG_HD                          // (bed_fmt.h and exact_log2.h have the same lines)
#if defined(__HIPCC__)
#define WG_HD __host__ __device__ __forceinline__
#else
#define WG_HD static inline
#endif
#endif
#ifndef WG_HDM                         // the same for a member function
#if defined(__HIPCC__)
#define WG_HDM __host__ __device__ __forceinline__
#else
#define WG_HDM inline
#endif
#endif

// why a member is refused (the texts: wg_inflate_what, inflate_plan.h)
enum {
    WG_INF_OK = 0,
    WG_INF_BLOCK_TYPE = 1,       // block type 3
    WG_INF_STORED_LEN = 2,       // LEN is not the complement of NLEN
    WG_INF_TOO_MANY = 3,         // HLIT > 286 or HDIST > 30
    WG_INF_CLEN_CODE = 4,        // the code-length code is over-subscribed or incomplete
    WG_INF_REPEAT_FIRST = 5,     // repeat code 16 with no length before it
    WG_INF_REPEAT_OVER = 6,      // a repeat that passes HLIT + HDIST
    WG_INF_NO_EOB = 7,           // the literal/length code has no symbol 256
    WG_INF_LIT_SET = 8,          // the literal/length code is over-subscribed, or incomplete with a code longer than 1 bit
    WG_INF_DIST_SET = 9,         // the distance code, the same
    WG_INF_LIT_CODE = 10,        // bits that are no literal/length code, or symbol 286 / 287
    WG_INF_DIST_CODE = 11,       // bits that are no distance code, or distance code 30 / 31
    WG_INF_FAR = 12,             // a distance that reaches before the member's first byte
    WG_INF_TRUNCATED = 13,       // the payload ends before the final block does
    WG_INF_OUT_BIG = 14,         // more text than ISIZE
    WG_INF_OUT_SMALL = 15,       // less text than ISIZE
    WG_INF_CODES = 16
};

// one member of a BGZF byte string, as the host plan hands it to the decoders
struct wg_bgzf_member {
    uint64_t in_off;             // of the DEFLATE payload in the compressed bytes
    uint32_t in_len;             // its length
    uint32_t isize;              // the member's ISIZE: the length of its text
    uint64_t out_off;            // of its text in the text buffer
    uint64_t file_off;           // of the member's first header byte in the file (messages)
};

#define WG_INF_LIT_BITS 10               // a literal/length code of up to 10 bits is one table read, a longer one is walked bit by bit
#define WG_INF_DIST_BITS 9               // the same for a distance code (the code-length code, at most 7 bits, is always one read)

// the tables of the block being decoded (7200 bytes; the device keeps one per wave in LDS)
struct WgInflateTables {
    uint16_t lcnt[16], lsym[288];        // literal/length code: codes of each length, symbols in canonical order
    uint16_t dcnt[16], dsym[32];         // distance code (and, while a dynamic header is read, the code-length code)
    uint16_t offs[16];
    uint8_t lens[320];
    uint32_t lfast[1 << WG_INF_LIT_BITS];        // the next bits -> what the code they begin with means (wg_inf_entry), 0: no code that short
    uint32_t dfast[1 << WG_INF_DIST_BITS];
};

template <class In>
struct WgBits {
    In& in;
    uint64_t hold = 0;           // the next n bits of the payload, the first one lowest (bits behind the payload's end read 0)
    int n = 0;
    int64_t w = 0;               // the next word to fetch
    int64_t pos = 0, total;      // bits dropped so far, bits the payload has
    WG_HDM WgBits(In& i, int64_t n_in) : in(i), total(8 * n_in) { seek(0); }
    WG_HDM void seek(int64_t bitpos)
    {
        pos = bitpos; w = bitpos >> 5;
        const int s = (int)(bitpos & 31);
        hold = (uint64_t)in.word(w++) >> s; n = 32 - s;
    }
    WG_HDM uint32_t peek(int k)                                   // k <= 32
    {
        if (n < k) { hold |= (uint64_t)in.word(w++) << n; n += 32; }
        return (uint32_t)(hold & ((1ull << k) - 1));
    }
    WG_HDM bool drop(int k)                                       // after peek(>= k); false: the payload has no k bits left
    {
        if (pos + k > total) return false;
        hold >>= k; n -= k; pos += k;
        return true;
    }
    WG_HDM int bits(int k)                                        // k <= 16; -1: the payload has no k bits left
    {
        const uint32_t v = peek(k);
        return drop(k) ? (int)v : -1;
    }
};

// lens[0 .. n) -> cnt[1 .. 15], sym in canonical order.  Returns what the code leaves unused of the 15-bit code space (0: complete,
// > 0: incomplete), -1 when it is over-subscribed; *max_len: the longest code (0: no code at all).
WG_HD int wg_inf_build(const uint8_t* lens, int n, uint16_t* cnt, uint16_t* sym, uint16_t* offs, int* max_len)
{
    for (int l = 0; l < 16; l++) cnt[l] = 0;
    for (int i = 0; i < n; i++) cnt[lens[i]] = (uint16_t)(cnt[lens[i]] + 1);
    int left = 1, mx = 0;
    for (int l = 1; l < 16; l++) {
        left = (left << 1) - (int)cnt[l];
        if (left < 0) return -1;
        if (cnt[l]) mx = l;
    }
    offs[1] = 0;
    for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + cnt[l]);
    for (int i = 0; i < n; i++)
        if (lens[i]) { sym[offs[lens[i]]] = (uint16_t)i; offs[lens[i]] = (uint16_t)(offs[lens[i]] + 1); }
    *max_len = mx;
    return left;
}

// the symbol whose code the bits of v begin with (the first bit lowest; 15 bits), *len its length: -1 when they begin with no code (an
// incomplete code only)
template <bool Uniform, class In>
WG_HD int wg_inf_walk(In& in, uint32_t v, const uint16_t* cnt, const uint16_t* sym, int* len_out)
{
    int code = 0, first = 0, index = 0;
    for (int len = 1; len < 16; len++) {
        code |= (int)(v & 1); v >>= 1;
        const int count = Uniform ? (int)in.uni(cnt[len]) : (int)cnt[len];
        if (code - count < first) { *len_out = len; return Uniform ? (int)in.uni(sym[index + (code - first)]) : (int)sym[index + (code - first)]; }
        index += count; first = (first + count) << 1; code <<= 1;
    }
    return -1;
}

// What a decoded symbol means, in one word: code length | extra bits << 4 | base << 8 | kind << 24.  A lookup table holds these, so that a
// code of at most the table's bits costs one read, its length / distance base and extra-bit count included.
enum { WG_INF_PLAIN = 0, WG_INF_LITLEN = 1, WG_INF_DIST = 2 };                  // which code a symbol belongs to
enum { WG_INF_K_VALUE = 1, WG_INF_K_END = 2, WG_INF_K_LENGTH = 3, WG_INF_K_BAD = 4 };  // value: a literal, a distance, a plain symbol (in base)
WG_HD uint32_t wg_inf_entry(int mode, int s, int len)
{
    static constexpr uint16_t lbase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static constexpr uint8_t lext[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static constexpr uint16_t dbase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static constexpr uint8_t dext[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    uint32_t kind = WG_INF_K_VALUE, base = (uint32_t)s, extra = 0;
    if (mode == WG_INF_LITLEN && s >= 256) {
        if (s == 256) { kind = WG_INF_K_END; base = 0; }
        else if (s < 286) { kind = WG_INF_K_LENGTH; base = lbase[s - 257]; extra = lext[s - 257]; }
        else { kind = WG_INF_K_BAD; base = 0; }                  // symbols 286 / 287
    } else if (mode == WG_INF_DIST) {
        if (s < 30) { base = dbase[s]; extra = dext[s]; }
        else { kind = WG_INF_K_BAD; base = 0; }                  // distance codes 30 / 31
    }
    return (uint32_t)len | (extra << 4) | (base << 8) | (kind << 24);
}

// fast[j] for every j of `bits` bits: the entry of the code j begins with, 0 when none of at most `bits` bits does
template <class In>
WG_HD void wg_inf_fast(In& in, const uint16_t* cnt, const uint16_t* sym, uint32_t* fast, int bits, int mode)
{
    for (int j = in.lane(); j < (1 << bits); j += in.lanes()) {
        int len = 0;
        const int s = wg_inf_walk<false>(in, (uint32_t)j, cnt, sym, &len);
        fast[j] = s >= 0 && len <= bits ? wg_inf_entry(mode, s, len) : 0;
    }
    in.sync();
}

// the next symbol of a canonical code as its entry (its bits dropped): 0 when the bits are no code (an incomplete code only), 1 when the
// payload ends inside it (no entry is 0 or 1: a code has a length, and a kind above bit 24)
template <class In>
WG_HD uint32_t wg_inf_symbol(WgBits<In>& b, const uint16_t* cnt, const uint16_t* sym, const uint32_t* fast, int bits, int mode)
{
    const uint32_t v = b.peek(15);
    uint32_t e = b.in.uni(fast[v & ((1u << bits) - 1)]);
    if (!e) {
        int len = 0;
        const int s = wg_inf_walk<true>(b.in, v, cnt, sym, &len);
        if (s < 0) return 0;
        e = wg_inf_entry(mode, s, len);
    }
    return b.drop((int)(e & 15)) ? e : 1;
}

// the dynamic block header: HLIT, HDIST, HCLEN, the code-length code, the lengths, both tables
template <class In>
WG_HD int wg_inf_dynamic(WgBits<In>& b, WgInflateTables& t)
{
    static constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    const int h = b.bits(14);
    if (h < 0) return WG_INF_TRUNCATED;
    const int nlen = (h & 31) + 257, ndist = ((h >> 5) & 31) + 1, ncode = ((h >> 10) & 15) + 4;
    if (nlen > 286 || ndist > 30) return WG_INF_TOO_MANY;
    for (int i = 0; i < 19; i++) t.lens[i] = 0;
    for (int i = 0; i < ncode; i++) {
        const int v = b.bits(3);
        if (v < 0) return WG_INF_TRUNCATED;
        t.lens[order[i]] = (uint8_t)v;
    }
    int mx = 0;
    if (wg_inf_build(t.lens, 19, t.dcnt, t.dsym, t.offs, &mx) != 0) return WG_INF_CLEN_CODE;      // (zlib: an incomplete one is an error here, whatever its depth)
    wg_inf_fast(b.in, t.dcnt, t.dsym, t.dfast, 7, WG_INF_PLAIN);
    int index = 0;
    while (index < nlen + ndist) {                               // every turn drops a bit and writes a length
        const uint32_t ce = wg_inf_symbol(b, t.dcnt, t.dsym, t.dfast, 7, WG_INF_PLAIN);
        if (ce < 2) return ce ? WG_INF_TRUNCATED : WG_INF_CLEN_CODE;
        const int s = (int)((ce >> 8) & 0xffff);
        if (s < 16) { t.lens[index++] = (uint8_t)s; continue; }
        int prev = 0, rep;
        if (s == 16) {
            if (index == 0) return WG_INF_REPEAT_FIRST;
            prev = (int)b.in.uni(t.lens[index - 1]);
            rep = b.bits(2); if (rep < 0) return WG_INF_TRUNCATED;
            rep += 3;
        } else if (s == 17) {
            rep = b.bits(3); if (rep < 0) return WG_INF_TRUNCATED;
            rep += 3;
        } else {
            rep = b.bits(7); if (rep < 0) return WG_INF_TRUNCATED;
            rep += 11;
        }
        if (index + rep > nlen + ndist) return WG_INF_REPEAT_OVER;
        while (rep--) t.lens[index++] = (uint8_t)prev;
    }
    if (b.in.uni(t.lens[256]) == 0) return WG_INF_NO_EOB;
    int left = wg_inf_build(t.lens, nlen, t.lcnt, t.lsym, t.offs, &mx);
    if (left < 0 || (left > 0 && mx != 1)) return WG_INF_LIT_SET;
    left = wg_inf_build(t.lens + nlen, ndist, t.dcnt, t.dsym, t.offs, &mx);
    if (left < 0 || (left > 0 && mx > 1)) return WG_INF_DIST_SET;      // (no distance code at all is accepted: a block without a match)
    wg_inf_fast(b.in, t.lcnt, t.lsym, t.lfast, WG_INF_LIT_BITS, WG_INF_LITLEN);
    wg_inf_fast(b.in, t.dcnt, t.dsym, t.dfast, WG_INF_DIST_BITS, WG_INF_DIST);
    return WG_INF_OK;
}

// the fixed codes (RFC 1951 3.2.6); symbols 286 / 287 and distance codes 30 / 31 take part in the codes and are refused where they turn up
template <class In>
WG_HD void wg_inf_fixed(In& in, WgInflateTables& t)
{
    int i = 0, mx = 0;
    for (; i < 144; i++) t.lens[i] = 8;
    for (; i < 256; i++) t.lens[i] = 9;
    for (; i < 280; i++) t.lens[i] = 7;
    for (; i < 288; i++) t.lens[i] = 8;
    for (; i < 320; i++) t.lens[i] = 5;
    (void)wg_inf_build(t.lens, 288, t.lcnt, t.lsym, t.offs, &mx);
    (void)wg_inf_build(t.lens + 288, 32, t.dcnt, t.dsym, t.offs, &mx);
    wg_inf_fast(in, t.lcnt, t.lsym, t.lfast, WG_INF_LIT_BITS, WG_INF_LITLEN);
    wg_inf_fast(in, t.dcnt, t.dsym, t.dfast, WG_INF_DIST_BITS, WG_INF_DIST);
}

// the symbols of one block up to its end-of-block
template <class In, class Out>
WG_HD int wg_inf_codes(WgBits<In>& b, Out& out, const WgInflateTables& t)
{
    for (;;) {                                                   // every turn drops a bit
        const uint32_t e = wg_inf_symbol(b, t.lcnt, t.lsym, t.lfast, WG_INF_LIT_BITS, WG_INF_LITLEN);
        if (e < 2) return e ? WG_INF_TRUNCATED : WG_INF_LIT_CODE;
        const uint32_t kind = e >> 24;
        if (kind == WG_INF_K_VALUE) {
            const int rc = out.lit((uint8_t)(e >> 8));
            if (rc) return rc;
            continue;
        }
        if (kind == WG_INF_K_END) return WG_INF_OK;
        if (kind == WG_INF_K_BAD) return WG_INF_LIT_CODE;
        const int le = b.bits((int)((e >> 4) & 15));
        if (le < 0) return WG_INF_TRUNCATED;
        const uint32_t len = ((e >> 8) & 0xffff) + (uint32_t)le;
        const uint32_t d = wg_inf_symbol(b, t.dcnt, t.dsym, t.dfast, WG_INF_DIST_BITS, WG_INF_DIST);
        if (d < 2) return d ? WG_INF_TRUNCATED : WG_INF_DIST_CODE;
        if ((d >> 24) == WG_INF_K_BAD) return WG_INF_DIST_CODE;
        const int de = b.bits((int)((d >> 4) & 15));
        if (de < 0) return WG_INF_TRUNCATED;
        const uint32_t dist = ((d >> 8) & 0xffff) + (uint32_t)de;
        if (dist > out.pos()) return WG_INF_FAR;
        const int rc = out.copy(dist, len);
        if (rc) return rc;
    }
}

// One member: the payload's n_in bytes through `in`, its text through `out` (which knows ISIZE), `t` for the tables.  WG_INF_OK or why not.
template <class In, class Out>
WG_HD int wg_inflate_member(In& in, int64_t n_in, Out& out, uint32_t isize, WgInflateTables& t)
{
    WgBits<In> b(in, n_in);
    for (;;) {                                                   // every turn drops the 3 header bits
        const int h = b.bits(3);
        if (h < 0) return WG_INF_TRUNCATED;
        const int type = h >> 1;
        int rc = WG_INF_OK;
        if (type == 0) {
            int64_t at = (b.pos + 7) >> 3;                       // LEN and NLEN begin at the next byte boundary
            if (at + 4 > n_in) return WG_INF_TRUNCATED;
            b.seek(at * 8);
            const uint32_t v = b.peek(32);
            (void)b.drop(32);
            const uint32_t len = v & 0xffff;
            if ((len ^ 0xffff) != (v >> 16)) return WG_INF_STORED_LEN;
            at += 4;
            if (at + (int64_t)len > n_in) return WG_INF_TRUNCATED;
            rc = out.stored(in, at, len);
            b.seek((at + (int64_t)len) * 8);
        } else if (type == 3) {
            return WG_INF_BLOCK_TYPE;
        } else {
            if (type == 1) wg_inf_fixed(in, t);
            else rc = wg_inf_dynamic(b, t);
            if (rc == WG_INF_OK) rc = wg_inf_codes(b, out, t);
        }
        if (rc) return rc;
        if (h & 1) break;
    }
    return out.pos() == isize ? WG_INF_OK : WG_INF_OUT_SMALL;
}

// ---- the serial host twin -----------------------------------------------------------------------------------------------------------------
struct WgHostIn {
    const uint8_t* p;
    int64_t n;
    uint32_t word(int64_t w) const
    {
        uint32_t v = 0;
        const int64_t at = 4 * w;
        if (at + 4 <= n) { memcpy(&v, p + at, 4); return v; }
        for (int k = 0; k < 4; k++)
            if (at + k < n) v |= (uint32_t)p[at + k] << (8 * k);
        return v;
    }
    uint8_t byte(int64_t i) const { return p[i]; }
    uint32_t uni(uint32_t v) const { return v; }
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() const {}
};

struct WgHostOut {
    uint8_t* p;
    uint32_t isize, at = 0;
    WgHostOut(uint8_t* out, uint32_t n) : p(out), isize(n) {}
    uint32_t pos() const { return at; }
    int lit(uint8_t b)
    {
        if (at >= isize) return WG_INF_OUT_BIG;
        p[at++] = b;
        return 0;
    }
    int copy(uint32_t dist, uint32_t len)
    {
        if (len > isize - at) return WG_INF_OUT_BIG;
        for (uint32_t i = 0; i < len; i++, at++) p[at] = p[at - dist];
        return 0;
    }
    int stored(const WgHostIn& in, int64_t off, uint32_t len)
    {
        if (len > isize - at) return WG_INF_OUT_BIG;
        for (uint32_t i = 0; i < len; i++) p[at++] = in.byte(off + i);
        return 0;
    }
};

// payload[0 .. n_in) -> out[0 .. isize): WG_INF_OK, or why the member is refused (out then holds what was decoded before)
inline int inflate_member_host(const uint8_t* payload, int64_t n_in, uint8_t* out, uint32_t isize)
{
    WgInflateTables t;
    WgHostIn in{payload, n_in};
    WgHostOut o(out, isize);
    return wg_inflate_member(in, n_in, o, isize, t);
}
