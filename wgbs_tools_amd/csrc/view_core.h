// view_core.h — the rules of `wgbstools view` / `cview` on pat reads, one set of functions for host and device (like bed_fmt.h and
// deflate_core.h): what is cut from a read (cview.cpp:8-17,:87-167 with one block; patter_utils.cpp:260-280), the order of
// `LC_ALL=C sort -k2,2n -k3,3` over the surviving lines, when two adjacent lines collapse (collapse_pat.pl) and how long an output
// line is.  No HIP needed: g++ compiles it alone (tests/native/view_host.cpp hands it to the tests).
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
    uint32_t line;                     // reserved (0)
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

// the strict order of the sort: record ix before record iy (their input positions break the ties that cannot show)
WG_HD bool wg_view_less(const wg_view_rec* recs, uint32_t ix, uint32_t iy, const char* arena)
{
    const int d = wg_view_cmp(recs[ix], recs[iy], arena);
    return d ? d < 0 : ix < iy;
}

// does the line y, which follows the line x, begin a new run (collapse_pat.pl: any of chrom, start, pattern differs)?
WG_HD bool wg_view_run_head(const wg_view_rec& x, const wg_view_rec& y, const char* arena) { return wg_view_cmp(x, y, arena) != 0; }

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
