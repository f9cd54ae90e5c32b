// deflate_core.h — the DEFLATE encoder (RFC 1951) of one BGZF member, once, for the host and the device (the mirror of inflate_core.h):
// at most WG_DEF_MEMBER bytes of text become the member's 18-byte header, a raw DEFLATE stream, CRC32 and ISIZE.
//
// The rule, stated so that its result does not depend on how many lanes run it:
//   matching   LZ77 over a table of last positions, indexed by a 13-bit hash of the next 4 bytes.  Positions are taken in fixed groups of
//              64.  A position's one candidate is what its slot held BEFORE the group; it is a match when it lies at most 32768 back (a
//              member is longer than the window, so this is checked) and at least 4 bytes agree (at most 258, never past the member's
//              end).  Then the group's positions enter the table; where two of them hit one slot the highest stays (Ex::amax).
//   selection  one greedy left-to-right pick, carried across groups: at the first position not yet covered, its match if it has one,
//              else its byte as a literal.
//   coding     tokens collect until another group might not fit WG_DEF_TOKENS; they become one DEFLATE block, dynamic or fixed Huffman,
//              whichever is fewer bits (the dynamic one on a tie never: it must be strictly smaller).  Code lengths are Huffman's,
//              limited to 15 (7 for the code-length code) by halving the counts (rounding up) and building again until they fit.
//              A member whose stream would pass its stored form (one stored block: n + 5 bytes) is stored instead.
// So a member never exceeds 18 + n + 5 + 8 bytes: 65311 for n = 65280, and BSIZE fits.
//
// What runs the rule is the caller's: an executor `Ex` and an output `Out`.
//   Ex::lane(), lanes()    who runs this copy and how many run together (the host: 0 of 1; the device: a lane of its wave).  Loops written
//                          `for (i = lane(); i < n; i += lanes())` are shared out; everything else every copy computes alike.
//   Ex::sync()             what the copies wrote before is visible to all of them behind it
//   Ex::uni(v)             v, which every copy holds alike (the device: a scalar register)
//   Ex::mask64(m)          bit i set where m[i] != 0, i < 64
//   Ex::amax(p, v)         *p = max(*p, v), Ex::add(p, v): *p += v — whichever copies call them together
//   Ex::scan(v, &total)    the sum of v over the copies before this one, and over all of them (called by all copies together)
//   Ex::fold_xor(v)        v of all copies xor-ed
//   Out::bits(at, v, nb)   nb <= 48 bits of v at bit `at` of the member (bit 0: the lowest bit of its first byte); any copy, any order
//   Out::settle(at)        every bit below `at` has been put; at most 8192 bits are put between two calls
//   Out::finish(at)        the same at the member's end (a whole number of bytes)
//   Out::patch16(byte, v)  two bytes over what was put there before (BSIZE)
//   Out::stored(text, n, crc)   the whole member in its stored form, over whatever was put before
// The text is read where it lies, through a plain pointer.  deflate_member_host() below is the serial host twin; k_bgzf_deflate
// (deflate_kernels.h) is the device's.  Both produce the same bytes for the same text.
//
// Bounds, by construction:
//   reads    text[p] for p < n only: 4-byte reads are asked for p + 4 <= n, a comparison stops at min(258, n - p) bytes.
//   writes   a block is put only when its exact cost, computed before, keeps the stream within the stored form's n + 5 bytes; else the
//            encoder stops and stores.  Tokens: a group adds at most 64, and a block is closed while 64 more still fit.
//   loops    every loop counts positions of the member, tokens of a block, symbols of an alphabet, or the 32 halvings of a count.
#pragma once
#include <cstdint>
#include <cstring>

#ifndef WG_HD                          // (inflate_core.h, bed_fmt.h and exact_log2.h have the same lines)
#if defined(__HIPCC__)
#define WG_HD __host__ __device__ __forceinline__
#else
#define WG_HD static inline
#endif
#endif
#ifndef WG_HDM
#if defined(__HIPCC__)
#define WG_HDM __host__ __device__ __forceinline__
#else
#define WG_HDM inline
#endif
#endif

#define WG_DEF_MEMBER 65280              // bytes of text per member (htslib's cut; its stored form still fits BSIZE)
#define WG_DEF_HEAD 18                   // the BGZF header
#define WG_DEF_TAIL 8                    // CRC32, ISIZE
#define WG_DEF_STORED_MAX (WG_DEF_HEAD + WG_DEF_MEMBER + 5 + WG_DEF_TAIL)      // 65311: the largest member
#define WG_DEF_HASH_BITS 13
#define WG_DEF_GROUP 64
#define WG_DEF_TOKENS 2560               // tokens of one DEFLATE block at most
#define WG_DEF_MIN_MATCH 4
#define WG_DEF_MAX_MATCH 258
#define WG_DEF_WINDOW 32768

// the encoder's working set (the device keeps one per wave in LDS: 52 KB)
struct WgDeflateState {
    uint32_t head[1 << WG_DEF_HASH_BITS];        // hash -> last position + 1, 0: none
    uint32_t tok[WG_DEF_TOKENS];                 // a literal: byte << 9; a match: length | (distance - 1) << 9
    uint32_t m[WG_DEF_GROUP];                    // the group's matches as tokens, 0: none
    uint32_t lfreq[288], dfreq[32], clfreq[20];
    uint16_t lcode[288], dcode[32], clcode[20];  // codes, bit-reversed: the first bit lowest
    uint8_t llen[288], dlen[32], cllen[20];
    uint16_t seq[320];                           // the code lengths as code-length symbols: symbol | extra value << 5
    uint32_t f[288], w[576];                     // the length builder: counts as halved so far; node weights, then depths
    uint16_t parent[576], order[288];
    uint16_t count[16], next[16];
};

WG_HD uint32_t wg_def_load32(const uint8_t* p)
{
    uint32_t v;
#if defined(__HIPCC__)
    __builtin_memcpy(&v, p, 4);
#else
    memcpy(&v, p, 4);
#endif
    return v;
}

WG_HD uint32_t wg_def_hash(uint32_t v) { return (v * 2654435761u) >> (32 - WG_DEF_HASH_BITS); }

// how many bytes agree at c and p (c < p), up to max_len; p + max_len <= n
WG_HD uint32_t wg_def_match_len(const uint8_t* text, uint32_t c, uint32_t p, uint32_t max_len)
{
    uint32_t k = 0;
    while (k + 4 <= max_len) {
        const uint32_t x = wg_def_load32(text + c + k) ^ wg_def_load32(text + p + k);
        if (x) return k + ((uint32_t)__builtin_ctz(x) >> 3);
        k += 4;
    }
    while (k < max_len && text[c + k] == text[p + k]) k++;
    return k;
}

// ---- CRC32 (zlib's polynomial, reflected) ---------------------------------------------------------------------------------------------------
#define WG_DEF_CRC_POLY 0xedb88320u

WG_HD uint32_t wg_def_crc_entry(uint32_t i)
{
    for (int k = 0; k < 8; k++) i = (i & 1) ? (i >> 1) ^ WG_DEF_CRC_POLY : i >> 1;
    return i;
}

// a * b modulo the polynomial (x^0 is bit 31)
WG_HD uint32_t wg_def_crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ WG_DEF_CRC_POLY : b >> 1;
    }
    return p;
}

// the register r after k more zero bytes: r * x^(8 k)
WG_HD uint32_t wg_def_crc_shift(uint32_t r, uint32_t k)
{
    if (k == 0) return r;
    uint32_t p = 0x80000000u, b = 0x00800000u;                   // x^0, x^8
    for (int i = 0; i < 32 && k; i++, k >>= 1) {
        if (k & 1) p = wg_def_crc_mul(p, b);
        b = wg_def_crc_mul(b, b);
    }
    return wg_def_crc_mul(p, r);
}

// Lane `lane` of `lanes` takes a contiguous share of the text and returns its register moved to the text's end; the shares xor-ed, and
// the whole inverted, are the text's CRC32 (lane 0 starts from ~0, the others from 0: the register is linear in its start value).
WG_HD uint32_t wg_def_crc_share(const uint8_t* text, uint32_t n, int lane, int lanes, const uint32_t* tab)
{
    const uint32_t per = (n + (uint32_t)lanes - 1) / (uint32_t)lanes;
    uint32_t lo = (uint32_t)lane * per, hi;
    if (lo > n) lo = n;
    hi = lo + per > n ? n : lo + per;
    uint32_t r = lane == 0 ? 0xffffffffu : 0u;
    for (uint32_t i = lo; i < hi; i++) r = tab[(r ^ text[i]) & 255] ^ (r >> 8);
    return wg_def_crc_shift(r, n - hi);
}

// ---- symbols ----------------------------------------------------------------------------------------------------------------------------------
// a match length 3 .. 258 -> its symbol - 257, extra bits, extra value
WG_HD void wg_def_len_sym(uint32_t len, uint32_t* sym, uint32_t* ebits, uint32_t* eval)
{
    const uint32_t l = len - 3;
    if (l < 8) { *sym = l; *ebits = 0; *eval = 0; return; }
    if (len == 258) { *sym = 28; *ebits = 0; *eval = 0; return; }
    const uint32_t msb = 31u - (uint32_t)__builtin_clz(l);       // >= 3
    *sym = 4 * (msb - 1) + ((l >> (msb - 2)) & 3);
    *ebits = msb - 2;
    *eval = l & ((1u << (msb - 2)) - 1);
}

// a distance 1 .. 32768 -> its symbol, extra bits, extra value
WG_HD void wg_def_dist_sym(uint32_t dist, uint32_t* sym, uint32_t* ebits, uint32_t* eval)
{
    const uint32_t d = dist - 1;
    if (d < 4) { *sym = d; *ebits = 0; *eval = 0; return; }
    const uint32_t msb = 31u - (uint32_t)__builtin_clz(d);       // >= 2
    *sym = 2 * msb + ((d >> (msb - 1)) & 1);
    *ebits = msb - 1;
    *eval = d & ((1u << (msb - 1)) - 1);
}

WG_HD uint32_t wg_def_lext(uint32_t s) { return s < 265 || s == 285 ? 0u : (s - 261) >> 2; }      // extra bits of literal/length symbol s
WG_HD uint32_t wg_def_dext(uint32_t d) { return d < 4 ? 0u : (d - 2) >> 1; }                       // of distance symbol d
WG_HD uint32_t wg_def_fixed_llen(uint32_t s) { return s < 144 ? 8u : s < 256 ? 9u : s < 280 ? 7u : 8u; }

// ---- code lengths -----------------------------------------------------------------------------------------------------------------------------
// freq[0 .. n) -> lens[0 .. n): Huffman's lengths, at most `limit`; a symbol that does not occur gets 0.  One symbol alone gets 1 bit; with
// `two` a second symbol (0 or 1) gets the other 1-bit code, for the code-length code, which may not be incomplete.
template <class Ex>
WG_HD void wg_def_lengths(Ex& ex, const uint32_t* freq, int n, int limit, uint8_t* lens, WgDeflateState& s, bool two)
{
    for (int i = ex.lane(); i < n; i += ex.lanes()) { s.f[i] = freq[i]; lens[i] = 0; }
    ex.sync();
    for (int round = 0; round < 32; round++) {                   // a count is below 2^17: all are 1 after 17 halvings, and 288 equal counts are 9 deep
        uint32_t mine = 0, used = 0;
        for (int i = ex.lane(); i < n; i += ex.lanes()) mine += s.f[i] != 0;
        (void)ex.scan(mine, &used);
        const int m = (int)ex.uni(used);
        if (m == 0) return;
        if (m == 1) {
            for (int i = ex.lane(); i < n; i += ex.lanes()) lens[i] = s.f[i] ? 1 : 0;
            ex.sync();
            if (two) lens[s.f[0] ? 1 : 0] = 1;
            ex.sync();
            return;
        }
        // the symbols that occur, by (count, symbol): every one finds its own rank
        for (int i = ex.lane(); i < n; i += ex.lanes()) {
            const uint32_t fi = s.f[i];
            if (!fi) continue;
            int rank = 0;
            for (int t = 0; t < n; t++) {
                const uint32_t ft = s.f[t];
                rank += ft && (ft < fi || (ft == fi && t < i));
            }
            s.order[rank] = (uint16_t)i;
            s.w[rank] = fi;
        }
        ex.sync();
        // Huffman's tree over two queues: the leaves w[0 .. m), the inner nodes w[m .. 2 m - 1) in the order they are made (a leaf first on a tie)
        int li = 0, ni = m;
        for (int k = m; k < 2 * m - 1; k++) {
            uint32_t sum = 0;
            for (int pick = 0; pick < 2; pick++) {
                int a;
                if (li < m && (ni >= k || ex.uni(s.w[li]) <= ex.uni(s.w[ni]))) a = li++;
                else a = ni++;
                sum += ex.uni(s.w[a]);
                s.parent[a] = (uint16_t)k;
            }
            s.w[k] = sum;
        }
        // depths, from the root down, in place of the weights
        uint32_t deepest = 0;
        s.w[2 * m - 2] = 0;
        for (int k = 2 * m - 3; k >= 0; k--) {
            const uint32_t d = ex.uni(s.w[ex.uni(s.parent[k])]) + 1;
            s.w[k] = d;
            if (k < m && d > deepest) deepest = d;
        }
        ex.sync();
        if (deepest <= (uint32_t)limit) {
            for (int r = ex.lane(); r < m; r += ex.lanes()) lens[s.order[r]] = (uint8_t)s.w[r];
            ex.sync();
            return;
        }
        for (int i = ex.lane(); i < n; i += ex.lanes()) s.f[i] = s.f[i] ? (s.f[i] + 1) >> 1 : 0;
        ex.sync();
    }
}

// canonical codes of lens[0 .. n), bit-reversed (every copy computes all of them)
WG_HD void wg_def_codes(const uint8_t* lens, int n, uint16_t* codes, uint16_t* cnt, uint16_t* next)
{
    for (int l = 0; l < 16; l++) cnt[l] = 0;
    for (int i = 0; i < n; i++) cnt[lens[i]] = (uint16_t)(cnt[lens[i]] + 1);
    uint32_t code = 0;
    cnt[0] = 0;
    for (int l = 1; l < 16; l++) { code = (code + cnt[l - 1]) << 1; next[l] = (uint16_t)code; }
    for (int i = 0; i < n; i++) {
        const int l = lens[i];
        if (!l) { codes[i] = 0; continue; }
        uint32_t c = next[l], r = 0;
        next[l] = (uint16_t)(c + 1);
        for (int b = 0; b < l; b++) { r = (r << 1) | (c & 1); c >>= 1; }
        codes[i] = (uint16_t)r;
    }
}

// ---- one block ----------------------------------------------------------------------------------------------------------------------------------
// the bits of one token under the block's codes
WG_HD uint64_t wg_def_token_bits(const WgDeflateState& s, uint32_t tok, uint32_t* nbits)
{
    const uint32_t len = tok & 0x1ff;
    if (!len) { const uint32_t b = tok >> 9; *nbits = s.llen[b]; return s.lcode[b]; }
    uint32_t ls, lx, lv, ds, dx, dv;
    wg_def_len_sym(len, &ls, &lx, &lv);
    wg_def_dist_sym((tok >> 9) + 1, &ds, &dx, &dv);
    uint64_t v = s.lcode[257 + ls];
    uint32_t nb = s.llen[257 + ls];
    v |= (uint64_t)lv << nb; nb += lx;
    v |= (uint64_t)s.dcode[ds] << nb; nb += s.dlen[ds];
    v |= (uint64_t)dv << nb; nb += dx;
    *nbits = nb;
    return v;
}

// The tokens tok[0 .. ntok) and the counts in lfreq / dfreq (without the end-of-block) as one block at *bitpos.  false, with nothing put,
// when the block would carry the stream past `limit` bits.  Leaves the counts zero.
template <class Ex, class Out>
WG_HD bool wg_def_block(Ex& ex, Out& out, WgDeflateState& s, uint32_t ntok, bool final, uint64_t* bitpos, uint64_t limit)
{
    static constexpr uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    ex.sync();
    s.lfreq[256] = ex.uni(s.lfreq[256]) + 1;
    ex.sync();
    wg_def_lengths(ex, s.lfreq, 286, 15, s.llen, s, false);
    wg_def_lengths(ex, s.dfreq, 30, 15, s.dlen, s, false);
    s.llen[286] = s.llen[287] = 0; s.dlen[30] = s.dlen[31] = 0;
    int nl = 286, nd = 30;
    while (nl > 257 && ex.uni(s.llen[nl - 1]) == 0) nl--;
    while (nd > 1 && ex.uni(s.dlen[nd - 1]) == 0) nd--;
    // the nl + nd lengths as code-length symbols: 16 repeats the length before 3 .. 6 times, 17 / 18 are 3 .. 10 / 11 .. 138 zeros
    for (int i = ex.lane(); i < 20; i += ex.lanes()) s.clfreq[i] = 0;
    ex.sync();
    const int tot = nl + nd;
    int nseq = 0;
    uint32_t clextra = 0;                                        // extra bits of the 16 / 17 / 18 symbols
    for (int i = 0; i < tot;) {
        const uint32_t v = ex.uni(i < nl ? s.llen[i] : s.dlen[i - nl]);
        int run = 1;
        while (i + run < tot && ex.uni(i + run < nl ? s.llen[i + run] : s.dlen[i + run - nl]) == v) run++;
        i += run;
        if (v != 0) { s.seq[nseq++] = (uint16_t)v; s.clfreq[v] = ex.uni(s.clfreq[v]) + 1; run--; }
        while (run > 0) {
            uint32_t sym, val;
            int take;
            if (run < 3) { sym = v; val = 0; take = 1; }
            else if (v != 0) { take = run < 6 ? run : 6; sym = 16; val = (uint32_t)take - 3; clextra += 2; }
            else if (run <= 10) { take = run; sym = 17; val = (uint32_t)take - 3; clextra += 3; }
            else { take = run < 138 ? run : 138; sym = 18; val = (uint32_t)take - 11; clextra += 7; }
            s.seq[nseq++] = (uint16_t)(sym | (val << 5));
            s.clfreq[sym] = ex.uni(s.clfreq[sym]) + 1;
            run -= take;
        }
    }
    ex.sync();
    wg_def_lengths(ex, s.clfreq, 19, 7, s.cllen, s, true);
    int nc = 19;
    while (nc > 4 && ex.uni(s.cllen[order[nc - 1]]) == 0) nc--;
    // the exact cost either way
    uint32_t dyn = 0, fix = 0;
    for (int i = ex.lane(); i < 286; i += ex.lanes()) {
        const uint32_t fq = s.lfreq[i], x = i > 256 ? wg_def_lext((uint32_t)i) : 0u;
        dyn += fq * (s.llen[i] + x); fix += fq * (wg_def_fixed_llen((uint32_t)i) + x);
    }
    for (int i = ex.lane(); i < 30; i += ex.lanes()) {
        const uint32_t fq = s.dfreq[i], x = wg_def_dext((uint32_t)i);
        dyn += fq * (s.dlen[i] + x); fix += fq * (5 + x);
    }
    for (int i = ex.lane(); i < 19; i += ex.lanes()) dyn += s.clfreq[i] * s.cllen[i];
    uint32_t dyn_all = 0, fix_all = 0;
    (void)ex.scan(dyn, &dyn_all);
    (void)ex.scan(fix, &fix_all);
    dyn_all = ex.uni(dyn_all) + 3 + 14 + 3 * (uint32_t)nc + clextra;
    fix_all = ex.uni(fix_all) + 3;
    const bool use_dyn = dyn_all < fix_all;
    uint64_t at = *bitpos;
    if (at + (use_dyn ? dyn_all : fix_all) > limit) return false;
    if (!use_dyn) {
        for (int i = ex.lane(); i < 288; i += ex.lanes()) s.llen[i] = (uint8_t)wg_def_fixed_llen((uint32_t)i);
        for (int i = ex.lane(); i < 32; i += ex.lanes()) s.dlen[i] = 5;
        ex.sync();
    }
    wg_def_codes(s.llen, 288, s.lcode, s.count, s.next);
    wg_def_codes(s.dlen, 32, s.dcode, s.count, s.next);
    const bool first = ex.lane() == 0;
    if (first) out.bits(at, (final ? 1u : 0u) | (use_dyn ? 4u : 2u), 3);
    at += 3;
    if (use_dyn) {
        wg_def_codes(s.cllen, 19, s.clcode, s.count, s.next);
        if (first) out.bits(at, (uint32_t)(nl - 257) | ((uint32_t)(nd - 1) << 5) | ((uint32_t)(nc - 4) << 10), 14);
        at += 14;
        for (int i = 0; i < nc; i++, at += 3)
            if (first) out.bits(at, s.cllen[order[i]], 3);
        for (int i = 0; i < nseq; i++) {
            const uint32_t e = ex.uni(s.seq[i]), sym = e & 31, val = e >> 5;
            const uint32_t cl = ex.uni(s.cllen[sym]), xb = sym == 16 ? 2u : sym == 17 ? 3u : sym == 18 ? 7u : 0u;
            if (first) out.bits(at, (uint64_t)s.clcode[sym] | ((uint64_t)val << cl), (int)(cl + xb));
            at += cl + xb;
        }
    }
    ex.sync();
    out.settle(at);
    // the tokens, `lanes` at a time: the lengths prefix-summed, every copy puts its own token's bits
    for (uint32_t t0 = 0; t0 < ntok; t0 += (uint32_t)ex.lanes()) {
        const uint32_t t = t0 + (uint32_t)ex.lane();
        uint32_t nb = 0, all = 0;
        uint64_t v = 0;
        if (t < ntok) v = wg_def_token_bits(s, s.tok[t], &nb);
        const uint32_t before = ex.scan(nb, &all);
        if (nb) out.bits(at + before, v, (int)nb);
        at += ex.uni(all);
        ex.sync();
        out.settle(at);
    }
    if (first) out.bits(at, s.lcode[256], s.llen[256]);
    at += ex.uni(s.llen[256]);
    ex.sync();
    out.settle(at);
    for (int i = ex.lane(); i < 288; i += ex.lanes()) s.lfreq[i] = 0;
    for (int i = ex.lane(); i < 32; i += ex.lanes()) s.dfreq[i] = 0;
    ex.sync();
    *bitpos = at;
    return true;
}

// ---- one member ---------------------------------------------------------------------------------------------------------------------------------
// text[0 .. n), n <= WG_DEF_MEMBER -> the member through `out`; returns its size in bytes (at most 18 + n + 5 + 8).  crctab: wg_def_crc_entry
// of 0 .. 255.
template <class Ex, class Out>
WG_HD uint32_t wg_deflate_member(Ex& ex, const uint8_t* text, uint32_t n, Out& out, WgDeflateState& s, const uint32_t* crctab)
{
    for (int i = ex.lane(); i < (1 << WG_DEF_HASH_BITS); i += ex.lanes()) s.head[i] = 0;
    for (int i = ex.lane(); i < 288; i += ex.lanes()) s.lfreq[i] = 0;
    for (int i = ex.lane(); i < 32; i += ex.lanes()) s.dfreq[i] = 0;
    ex.sync();
    const uint32_t crc = ex.fold_xor(wg_def_crc_share(text, n, ex.lane(), ex.lanes(), crctab)) ^ 0xffffffffu;
    static constexpr uint8_t head[WG_DEF_HEAD] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0, 0};      // BSIZE comes last
    if (ex.lane() == 0)
        for (int i = 0; i < WG_DEF_HEAD; i++) out.bits(8u * (uint32_t)i, head[i], 8);
    uint64_t at = 8 * WG_DEF_HEAD;
    const uint64_t limit = at + 8ull * (n + 5);
    ex.sync();
    out.settle(at);
    uint32_t ntok = 0, cursor = 0;
    bool fits = true;
    for (uint32_t g0 = 0; g0 < n && fits; g0 += WG_DEF_GROUP) {
        const uint32_t cnt = n - g0 < WG_DEF_GROUP ? n - g0 : WG_DEF_GROUP;
        if (cursor < g0 + cnt) {
            // every position's candidate from the table as the groups before left it
            for (uint32_t i = (uint32_t)ex.lane(); i < WG_DEF_GROUP; i += (uint32_t)ex.lanes()) {
                const uint32_t p = g0 + i;
                uint32_t tok = 0;
                if (p + WG_DEF_MIN_MATCH <= n) {
                    const uint32_t c1 = s.head[wg_def_hash(wg_def_load32(text + p))];
                    if (c1 && p - (c1 - 1) <= WG_DEF_WINDOW) {
                        const uint32_t room = n - p < WG_DEF_MAX_MATCH ? n - p : WG_DEF_MAX_MATCH;
                        const uint32_t len = wg_def_match_len(text, c1 - 1, p, room);
                        if (len >= WG_DEF_MIN_MATCH) tok = len | ((p - c1) << 9);
                    }
                }
                s.m[i] = tok;
            }
            ex.sync();
            // the greedy pick: which positions begin a match, which are literals
            const uint64_t have = ex.mask64(s.m);
            uint64_t taken = 0, lits = 0;
            uint32_t p = cursor > g0 ? cursor - g0 : 0;
            while (p < cnt) {                                    // every turn takes a match or ends the group
                const uint64_t rest = have >> p;
                const uint32_t q = rest ? p + (uint32_t)__builtin_ctzll(rest) : cnt;
                if (q > p) lits |= (q - p >= 64 ? ~0ull : ((1ull << (q - p)) - 1)) << p;
                if (q >= cnt) { p = cnt; break; }
                taken |= 1ull << q;
                const uint32_t len = ex.uni(s.m[q]) & 0x1ff;     // >= 4 wherever `have` has a bit
                p = q + (len ? len : 1);
            }
            cursor = g0 + p;
            const uint64_t starts = taken | lits;
            for (uint32_t i = (uint32_t)ex.lane(); i < WG_DEF_GROUP; i += (uint32_t)ex.lanes()) {
                if (!((starts >> i) & 1)) continue;
                const uint32_t at_tok = ntok + (uint32_t)__builtin_popcountll(starts & ((1ull << i) - 1));
                if ((taken >> i) & 1) {
                    const uint32_t tok = s.m[i];
                    uint32_t sym, xb, xv;
                    s.tok[at_tok] = tok;
                    wg_def_len_sym(tok & 0x1ff, &sym, &xb, &xv);
                    ex.add(&s.lfreq[257 + sym], 1);
                    wg_def_dist_sym((tok >> 9) + 1, &sym, &xb, &xv);
                    ex.add(&s.dfreq[sym], 1);
                } else {
                    const uint32_t b = text[g0 + i];
                    s.tok[at_tok] = b << 9;
                    ex.add(&s.lfreq[b], 1);
                }
            }
            ntok += (uint32_t)__builtin_popcountll(starts);
        }
        // the group's positions enter the table
        for (uint32_t i = (uint32_t)ex.lane(); i < WG_DEF_GROUP; i += (uint32_t)ex.lanes()) {
            const uint32_t p = g0 + i;
            if (p + WG_DEF_MIN_MATCH <= n) ex.amax(&s.head[wg_def_hash(wg_def_load32(text + p))], p + 1);
        }
        ex.sync();
        const bool last = g0 + WG_DEF_GROUP >= n;
        if (last || ntok + WG_DEF_GROUP > WG_DEF_TOKENS) {
            fits = wg_def_block(ex, out, s, ntok, last, &at, limit);
            ntok = 0;
        }
    }
    if (n == 0) fits = wg_def_block(ex, out, s, 0, true, &at, limit);
    if (!fits) {
        out.stored(text, n, crc);
        return WG_DEF_HEAD + n + 5 + WG_DEF_TAIL;
    }
    at = (at + 7) & ~7ull;
    if (ex.lane() == 0) { out.bits(at, crc, 32); out.bits(at + 32, n, 32); }
    at += 64;
    ex.sync();
    out.finish(at);
    const uint32_t size = (uint32_t)(at >> 3);
    out.patch16(16, size - 1);
    return size;
}

// ---- the serial host twin -----------------------------------------------------------------------------------------------------------------
struct WgDefHostEx {
    int lane() const { return 0; }
    int lanes() const { return 1; }
    void sync() const {}
    uint32_t uni(uint32_t v) const { return v; }
    uint64_t mask64(const uint32_t* m) const
    {
        uint64_t r = 0;
        for (int i = 0; i < 64; i++) r |= (uint64_t)(m[i] != 0) << i;
        return r;
    }
    void amax(uint32_t* p, uint32_t v) const { if (v > *p) *p = v; }
    void add(uint32_t* p, uint32_t v) const { *p += v; }
    uint32_t scan(uint32_t v, uint32_t* total) const { *total = v; return 0; }
    uint32_t fold_xor(uint32_t v) const { return v; }
};

// the member in out[0 .. 18 + n + 5 + 8), which the caller has zeroed
struct WgDefHostOut {
    uint8_t* p;
    void bits(uint64_t at, uint64_t v, int nb)
    {
        (void)nb;
        v <<= at & 7;                                            // nb + 7 <= 55 bits
        for (uint64_t b = at >> 3; v; b++, v >>= 8) p[b] |= (uint8_t)v;
    }
    void settle(uint64_t) const {}
    void finish(uint64_t) const {}
    void patch16(uint32_t byte, uint32_t v) { p[byte] = (uint8_t)v; p[byte + 1] = (uint8_t)(v >> 8); }
    void stored(const uint8_t* text, uint32_t n, uint32_t crc)
    {
        static const uint8_t head[WG_DEF_HEAD] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0, 0};
        memcpy(p, head, WG_DEF_HEAD);
        patch16(16, WG_DEF_HEAD + n + 5 + WG_DEF_TAIL - 1);
        uint8_t* q = p + WG_DEF_HEAD;
        q[0] = 1; q[1] = (uint8_t)n; q[2] = (uint8_t)(n >> 8); q[3] = (uint8_t)~q[1]; q[4] = (uint8_t)~q[2];
        if (n) memcpy(q + 5, text, n);
        q += 5 + n;
        for (int k = 0; k < 4; k++) { q[k] = (uint8_t)(crc >> (8 * k)); q[4 + k] = (uint8_t)(n >> (8 * k)); }
    }
};

inline const uint32_t* wg_def_crc_table_host()
{
    static const struct Tab { uint32_t t[256]; Tab() { for (uint32_t i = 0; i < 256; i++) t[i] = wg_def_crc_entry(i); } } tab;
    return tab.t;
}

// text[0 .. n), n <= WG_DEF_MEMBER -> the BGZF member in out[0 .. size), size returned; out has room for 18 + n + 5 + 8 bytes
inline uint32_t deflate_member_host(const uint8_t* text, uint32_t n, uint8_t* out)
{
    static thread_local WgDeflateState s;
    memset(out, 0, (size_t)WG_DEF_HEAD + n + 5 + WG_DEF_TAIL);
    WgDefHostEx ex;
    WgDefHostOut o{out};
    return wg_deflate_member(ex, text, n, o, s, wg_def_crc_table_host());
}
