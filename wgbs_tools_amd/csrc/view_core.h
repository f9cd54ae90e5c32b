// view_core.h — the rules of `wgbstools view` / `cview` on pat reads, one set of functions for host and device (like bed_fmt.h and
// deflate_core.h): what is cut from a read (cview.cpp:8-17,:87-167 with one block; patter_utils.cpp:260-280), the order of
// `LC_ALL=C sort -k2,2n -k3,3` over the surviving lines, when two adjacent lines collapse (collapse_pat.pl) and how long an output
// line is; for `wgbstools mix_pat` the counter-based generator, the sample rule and the order of tied, labelled lines (at the end).  No HIP
// needed: g++ compiles it alone (tests/native/view_host.cpp and mix_host.cpp hand it to the tests).
//
// A surviving read is a record: its start after the cut, its count, and where its bytes lie in an arena — the chromosome's name
// followed by the cut pattern.  Everything below reads a record's bytes through a pointer to that arena.
#pragma once
#include <cstdint>
#include "bed_fmt.h"                   // WG_HD, wg_dec_len

#define WG_VIEW_STRICT 1               // flags of the cut rule
#define WG_VIEW_STRIP 2
#define WG_VIEW_NO_GAPS 4
#define WG_VIEW_SORT 8                 // the engine: sort the survivors before the collapse (not part of the cut)
#define WG_VIEW_FLAGS_ALL 15

#define WG_VIEW_MAX_SUM 1000000000000000LL   // a collapsed sum of 10^15 or more is refused: Perl prints it in exponent form

struct wg_view_rec {
    uint64_t off;                      // arena: clen bytes of the chromosome's name, then plen bytes of the cut pattern
    int64_t rs;                        // the first CpG of the cut pattern
    int32_t count;
    uint32_t clen, plen;
    uint32_t line;                     // the rank of the read's label (wgbsseg_patview_set_labels); 0 without labels
};

// what is left of a read
struct wg_view_cut {
    int64_t rs;                        // rs'
    int64_t first;                     // index of the first kept byte in the read's pattern
    int64_t len;                       // kept bytes; 0: the read is dropped
};

// Steps 1-5 on the read `rs, pat[0, plen)` (plen > 0) for the interval [s, e): selection, --strict clip, --strip, --min_len, --no_gaps.
// pat(i) -> byte i of the pattern.
template <class Pat>
WG_HD wg_view_cut wg_view_cut_read(int64_t rs, int64_t plen, Pat&& pat, int64_t s, int64_t e, int flags, int64_t min_len)
{
    wg_view_cut c = {rs, 0, 0};
    if (rs >= e || rs + plen - 1 < s) return c;                    // (the reference stops reading at rs >= e: on ascending reads, a test on the read)
    int64_t a = 0, b = plen;                                        // the kept bytes [a, b)
    if (flags & WG_VIEW_STRICT) {
        if (rs < s) { a = s - rs; c.rs = s; }
        if (b - a > e - c.rs) b = a + (e - c.rs);
    }
    if (flags & WG_VIEW_STRIP) {
        while (b > a && pat(b - 1) == '.') b--;
        if (b == a) return c;
        while (pat(a) == '.') { a++; c.rs++; }
    }
    if (min_len > b - a) return c;
    if (flags & WG_VIEW_NO_GAPS)
        for (int64_t i = a; i < b; i++)
            if (pat(i) == '.') return c;
    c.first = a;
    c.len = b - a;
    return c;
}

// ------------------------------------------------------------------------------------------------------------
// `wgbstools mask_pat` (mask_pat.cpp:78-104): sites hidden from the reads.  The hidden sites are a bitmap of 32-bit words over the sites
// [lo, hi): bit k of word w stands for site lo + 32 w + k; the bits of the last word at or behind hi are 0; a site outside [lo, hi) is
// not hidden.  An empty view (lo == hi) hides nothing.
// ------------------------------------------------------------------------------------------------------------
struct wg_view_mask {
    const uint32_t* words;             // (hi - lo + 31) / 32 of them
    int64_t lo, hi;
};

WG_HD int64_t wg_view_mask_words(int64_t lo, int64_t hi) { return (hi - lo + 31) >> 5; }

WG_HD bool wg_view_hidden(const wg_view_mask& m, int64_t site)
{
    if (site < m.lo || site >= m.hi) return false;
    const int64_t k = site - m.lo;
    return (m.words[k >> 5] >> (k & 31)) & 1u;
}

// the hidden bits of the 64 sites from `site` on (bit i: site + i), from at most three words of the bitmap; `site` may lie anywhere
WG_HD uint64_t wg_view_hidden64(const wg_view_mask& m, int64_t site)
{
    if (site >= m.hi || site + 64 <= m.lo) return 0;                // (sites are below 2^31: no overflow)
    const int64_t k = site - m.lo, w0 = k >> 5, nw = wg_view_mask_words(m.lo, m.hi);    // (>>: the floor, also of a negative k)
    const int sh = (int)(k & 31);
    const uint64_t a = w0 >= 0 && w0 < nw ? m.words[w0] : 0u, b = w0 + 1 >= 0 && w0 + 1 < nw ? m.words[w0 + 1] : 0u;
    const uint64_t low = a | (b << 32);
    if (!sh) return low;
    const uint64_t c = w0 + 2 >= 0 && w0 + 2 < nw ? m.words[w0 + 2] : 0u;
    return (low >> sh) | (c << (64 - sh));
}

// A read's hidden bits, 64 sites at a time: the window that holds byte i of the read is fetched when i leaves the one at hand, so a
// read of a few sites costs one fetch and a read of 1,500 loops over its windows.  at: the window's number in the read (-1: none yet).
struct wg_view_window {
    int64_t at;
    uint64_t bits;
};

// is byte i of the read that starts at site rs hidden?
WG_HD bool wg_view_hidden_at(const wg_view_mask& m, wg_view_window& w, int64_t rs, int64_t i)
{
    const int64_t k = i >> 6;
    if (k != w.at) { w.at = k; w.bits = wg_view_hidden64(m, rs + (k << 6)); }
    return (w.bits >> (i & 63)) & 1u;
}

// byte i of the read as mask_pat leaves it: '.' where the site rs + i is hidden
template <class Pat>
WG_HD char wg_view_masked_byte(const wg_view_mask& m, wg_view_window& w, int64_t rs, int64_t i, Pat&& pat)
{
    return wg_view_hidden_at(m, w, rs, i) ? '.' : pat(i);
}

// The masked cut: wg_view_cut_read on the read as the mask leaves it.  The mask comes after steps 1-2 — selection and --strict look at the
// read's start and length only, which the mask does not change — and before steps 3-5, which see a hidden site as '.'.
template <class Pat>
WG_HD wg_view_cut wg_view_cut_read_masked(int64_t rs, int64_t plen, Pat&& pat, const wg_view_mask& m, int64_t s, int64_t e, int flags, int64_t min_len)
{
    wg_view_window w = {-1, 0};
    return wg_view_cut_read(rs, plen, [&](int64_t i) { return wg_view_masked_byte(m, w, rs, i, pat); }, s, e, flags, min_len);
}

// bytes [0, la) of a against [0, lb) of b as strcmp orders them, a prefix first: < 0, 0, > 0
WG_HD int wg_view_cmp_bytes(const char* a, uint32_t la, const char* b, uint32_t lb)
{
    const uint32_t n = la < lb ? la : lb;
    for (uint32_t i = 0; i < n; i++) {
        const int d = (int)(unsigned char)a[i] - (int)(unsigned char)b[i];
        if (d) return d;
    }
    return la < lb ? -1 : la > lb ? 1 : 0;
}

// `sort -k2,2n -k3,3` in the C locale and its last-resort comparison, as far as it can show: rs', then the pattern, then the
// chromosome; 0 when the lines differ in their count only
WG_HD int wg_view_cmp(const wg_view_rec& x, const wg_view_rec& y, const char* arena)
{
    if (x.rs != y.rs) return x.rs < y.rs ? -1 : 1;
    const char *ax = arena + x.off, *ay = arena + y.off;
    const int d = wg_view_cmp_bytes(ax + x.clen, x.plen, ay + y.clen, y.plen);
    if (d) return d;
    return wg_view_cmp_bytes(ax, x.clen, ay, y.clen);
}

// the same with the label rank (wg_view_rec.line) as the last key, for an engine with labels: lines of two labels never collapse
WG_HD int wg_view_cmp_labelled(const wg_view_rec& x, const wg_view_rec& y, const char* arena)
{
    const int d = wg_view_cmp(x, y, arena);
    if (d) return d;
    return x.line != y.line ? (x.line < y.line ? -1 : 1) : 0;
}

template <bool LABELS>
WG_HD int wg_view_cmp_as(const wg_view_rec& x, const wg_view_rec& y, const char* arena)
{
    if constexpr (LABELS) return wg_view_cmp_labelled(x, y, arena);
    else return wg_view_cmp(x, y, arena);
}

// the strict order of the sort: record ix before record iy (their input positions break the ties that cannot show)
template <bool LABELS = false>
WG_HD bool wg_view_less(const wg_view_rec* recs, uint32_t ix, uint32_t iy, const char* arena)
{
    const int d = wg_view_cmp_as<LABELS>(recs[ix], recs[iy], arena);
    return d ? d < 0 : ix < iy;
}

// does the line y, which follows the line x, begin a new run (collapse_pat.pl: any of chrom, start, pattern differs)?
template <bool LABELS = false>
WG_HD bool wg_view_run_head(const wg_view_rec& x, const wg_view_rec& y, const char* arena) { return wg_view_cmp_as<LABELS>(x, y, arena) != 0; }

// the text of a start (a read that hangs over the genome's front starts below 1, possibly below 0): its length, and its bytes at dst
WG_HD int wg_view_int_len(int64_t v) { return v < 0 ? 1 + wg_dec_len((uint64_t)(-v)) : wg_dec_len((uint64_t)v); }

template <class P>
WG_HD int wg_view_int_put(P dst, int64_t v)
{
    if (v >= 0) return wg_dec_put(dst, (uint64_t)v);
    dst[0] = '-';
    return 1 + wg_dec_put(dst + 1, (uint64_t)(-v));
}

// bytes of the output line "chrom \t rs' \t pattern \t sum \n" of a run; 0 when the run prints nothing (sum <= 0)
WG_HD uint32_t wg_view_line_len(const wg_view_rec& r, int64_t sum)
{
    if (sum <= 0) return 0;
    return r.clen + 1 + (uint32_t)wg_view_int_len(r.rs) + 1 + r.plen + 1 + (uint32_t)wg_dec_len((uint64_t)sum) + 1;
}

// ------------------------------------------------------------------------------------------------------------
// `wgbstools mix_pat`: reads thinned by a binomial draw (src/pat_sampler/sampler.cpp), a label column, and the order `sort -m -k2,2n -k3,3`
// gives lines of several labels that tie in start, pattern and chromosome.  The reference seeds a fresh engine from the clock for every
// line; here the bits come from a counter-based generator keyed by the line's place in its file, so a draw depends on nothing but
// (seed, stream, byte offset of the line, count * reps, T) — not on chunks, tiles, threads or the order of the work.
// ------------------------------------------------------------------------------------------------------------
#define WG_VIEW_MAX_DRAWS (1LL << 20)  // count * reps of one line: more is refused, not looped over
#define WG_VIEW_MAX_T (1u << 30)       // T = floor(p * 2^32) with p <= 0.25
#define WG_VIEW_MAX_LABELS 255

// Philox4x32 with 10 rounds (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): out = the four words of the block
WG_HD void wg_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = counter[0], c1 = counter[1], c2 = counter[2], c3 = counter[3], k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The successes among n = count * reps draws (0 <= n <= WG_VIEW_MAX_DRAWS: the caller refuses more): draw j is word j & 3 of the block
// with counter {off, j >> 2, stream} under the key `seed`, a success when below T.  off: the byte offset of the line in its file's text.
WG_HD int64_t wg_view_sample(int64_t count, int64_t reps, uint32_t T, uint64_t seed, uint32_t stream, uint64_t off)
{
    const int64_t n = count * reps;
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t counter[4] = {(uint32_t)off, (uint32_t)(off >> 32), 0u, stream}, w[4];
    int64_t got = 0;
    for (int64_t j = 0; j < n; j += 4) {
        counter[2] = (uint32_t)(j >> 2);
        wg_philox4x32_10(counter, key, w);
        const int64_t m = n - j < 4 ? n - j : 4;
        for (int64_t k = 0; k < m; k++) got += w[k] < T ? 1 : 0;
    }
    return got;
}

// the decimal texts of two sums (both > 0) as bytes, a prefix first ("1" < "10" < "9"): < 0, 0, > 0
WG_HD int wg_view_cmp_dec_text(int64_t a, int64_t b)
{
    char ta[20], tb[20];
    const int la = wg_dec_put(ta, (uint64_t)a), lb = wg_dec_put(tb, (uint64_t)b);
    return wg_view_cmp_bytes(ta, (uint32_t)la, tb, (uint32_t)lb);
}

// Two collapsed lines that tie in start, pattern and chromosome: sort's last-resort comparison of the whole lines reaches the count's
// text, then the label's bytes (its rank says the same).  Strict: the labels of two such lines differ.
WG_HD bool wg_view_tie_less(int64_t sum_x, uint32_t rank_x, int64_t sum_y, uint32_t rank_y)
{
    const int d = wg_view_cmp_dec_text(sum_x, sum_y);
    return d ? d < 0 : rank_x < rank_y;
}

// the output line of a run with a label of lab_len bytes: "... sum \t label \n"
WG_HD uint32_t wg_view_line_len_labelled(const wg_view_rec& r, int64_t sum, uint32_t lab_len)
{
    const uint32_t plain = wg_view_line_len(r, sum);
    return plain ? plain + 1 + lab_len : 0;
}
