// bed2beta_core.h — the rules of `wgbstools bed2beta` on one line of BED text, one set of functions for host and device (like view_core.h
// and bed_fmt.h): the walk over the fields of `chr \t start \t end \t #meth \t #total [\t ...]`, the lookup of the chromosome among the
// genome's names, the search of the position among the chromosome's CpG loci, and the word a matched line leaves in the table of its
// site.  No HIP needed: g++ compiles it alone (tests/native/bed2beta_host.cpp and san_bed2beta.cpp hand it to the tests);
// k_bedbeta_scan (bed2beta_kernels.h) calls the same functions on a tile of text in LDS.
//
// The text is read through any `T` with `char at(int64_t i) const` (PatText on the device, wg_bb_host_text below on the host); a line
// begins at byte p of text[0, n) and ends at the first '\n' at or behind p (the feed guarantees one before n).
#pragma once
#include <cstdint>
#include "merge_plan.h"                // wg_merge_site: the exact trim_to_uint8 of one site

#define WG_BB_ADD_ONE 1                // flags: the position is start + 1
#define WG_BB_HEADER 2                 //        the line at byte offset 0 of the file is a header: dropped unread
#define WG_BB_FLAGS_ALL 3

#define WG_BB_MAX_DIGITS 18            // a number of more digits is refused (10^18 - 1 < 2^63)
#define WG_BB_MAX_TOTAL 0x7fffffffLL
#define WG_BB_MAX_FED (1ULL << 47)     // bytes of one file: a word's offset leaves 16 bits for the pair and never makes the empty marker
#define WG_BB_EMPTY (~0ULL)            // the table's word of a site no line has matched

// why a line is refused (the low byte of the report word; the lowest offset wins, whatever its reason)
#define WG_BB_FEW_FIELDS 1             // fewer than five tab-separated fields
#define WG_BB_NOT_NUMBER 2             // start, #meth or #total: not 1 .. 18 decimal digits and nothing else
#define WG_BB_TOTAL_RANGE 3            // #total above 2^31 - 1
#define WG_BB_METH_GT_TOTAL 4          // #meth above #total (numpy would wrap it)

struct wg_bb_host_text {
    const char* p;
    char at(int64_t i) const { return p[i]; }
};

// what the walk finds on a line: the chromosome's bytes [cs, cs + clen) and the three numbers
struct wg_bb_line {
    int64_t cs, clen;
    int64_t start, meth, total;
};

// the field [i, end) as a number: 1 .. WG_BB_MAX_DIGITS bytes, all of them '0' .. '9'
template <class T>
WG_HD bool wg_bb_number(const T& t, int64_t i, int64_t end, int64_t& val)
{
    if (end <= i || end - i > WG_BB_MAX_DIGITS) return false;
    int64_t v = 0;
    for (; i < end; i++) {
        const char ch = t.at(i);
        if (ch < '0' || ch > '9') return false;
        v = v * 10 + (ch - '0');
    }
    val = v;
    return true;
}

// The walk: 0 and `out` filled, or the reason the line is refused.  Field 3 and everything behind field 5 are stepped over unread; the
// tabs are found first, so a line of fewer than five fields is refused as such whatever its fields hold.
template <class T>
WG_HD int wg_bb_walk(const T& t, int64_t p, int64_t n, wg_bb_line& out)
{
    int64_t tab[4], i = p, end5 = -1;
    int k = 0;
    for (; i < n; i++) {
        const char ch = t.at(i);
        if (ch == '\n') break;
        if (ch != '\t') continue;
        if (k == 4) { end5 = i; break; }                           // the tab behind field 5
        tab[k++] = i;
    }
    if (k < 4) return WG_BB_FEW_FIELDS;
    if (end5 < 0) end5 = i;                                         // the line's newline (or n)
    out.cs = p; out.clen = tab[0] - p;
    if (!wg_bb_number(t, tab[0] + 1, tab[1], out.start) || !wg_bb_number(t, tab[2] + 1, tab[3], out.meth) || !wg_bb_number(t, tab[3] + 1, end5, out.total))
        return WG_BB_NOT_NUMBER;
    if (out.total > WG_BB_MAX_TOTAL) return WG_BB_TOTAL_RANGE;
    if (out.meth > out.total) return WG_BB_METH_GT_TOTAL;
    return 0;
}

// The genome's chromosomes in the byte order of their names, a prefix first: rank r's name is arena[off[r], off[r + 1]), its sites are
// [lo[r], hi[r]) of the loci (bed2beta_plan.h builds and checks the table).
struct wg_bb_chroms {
    const char* arena;
    const uint32_t* off;
    const int32_t* lo;
    const int32_t* hi;
    int32_t n;
};

// bytes [cs, cs + clen) of the text against a name, as strcmp orders them, a prefix first: < 0, 0, > 0
template <class T>
WG_HD int wg_bb_cmp_name(const T& t, int64_t cs, int64_t clen, const char* name, uint32_t nlen)
{
    const int64_t m = clen < (int64_t)nlen ? clen : (int64_t)nlen;
    for (int64_t i = 0; i < m; i++) {
        const int d = (int)(unsigned char)t.at(cs + i) - (int)(unsigned char)name[i];
        if (d) return d;
    }
    return clen < (int64_t)nlen ? -1 : clen > (int64_t)nlen ? 1 : 0;
}

// the rank of the chromosome whose name equals the field byte for byte, -1 when the genome has none (`chr1` is not `chr10`: the lengths
// are compared too).  hint: a rank tried first (neighbouring lines mostly name the same chromosome), -1: none.
template <class T>
WG_HD int32_t wg_bb_find_chrom(const T& t, int64_t cs, int64_t clen, const wg_bb_chroms& c, int32_t hint)
{
    if (hint >= 0 && hint < c.n && wg_bb_cmp_name(t, cs, clen, c.arena + c.off[hint], c.off[hint + 1] - c.off[hint]) == 0) return hint;
    int32_t a = 0, b = c.n;
    while (a < b) {
        const int32_t m = a + ((b - a) >> 1);
        const int d = wg_bb_cmp_name(t, cs, clen, c.arena + c.off[m], c.off[m + 1] - c.off[m]);
        if (d == 0) return m;
        if (d < 0) b = m; else a = m + 1;
    }
    return -1;
}

// the site whose locus is p among loci[lo, hi) (strictly ascending): the lower bound, a hit only on equality; -1: p is no CpG there
WG_HD int64_t wg_bb_find_locus(const uint32_t* loci, int64_t lo, int64_t hi, int64_t p)
{
    if (p < 0 || p > 0xffffffffLL) return -1;
    int64_t a = lo, b = hi;
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if ((int64_t)loci[m] < p) a = m + 1; else b = m;
    }
    return a < hi && (int64_t)loci[a] == p ? a : -1;
}

// The word of a matched line: (byte offset of the line in its file << 16) | m8 << 8 | c8 with (m8, c8) the line's pair as the .beta file
// stores it.  The minimum over the lines of a site is the first of them in the file, and its pair rides along.
WG_HD uint64_t wg_bb_word(uint64_t off, int64_t meth, int64_t total)
{
    uint32_t m8 = 0, c8 = 0;
    wg_merge_site((uint32_t)meth, (uint32_t)total, 255u, m8, c8);   // (0 <= meth <= total <= 2^31 - 1: the walk's refusals)
    return (off << 16) | (uint64_t)((m8 & 0xffu) << 8) | (uint64_t)(c8 & 0xffu);
}

// the two bytes of a site from its word: 0, 0 for the empty marker
WG_HD uint32_t wg_bb_pair(uint64_t word) { return word == WG_BB_EMPTY ? 0u : (uint32_t)((word >> 8) & 0xffu) | (uint32_t)(word & 0xffu) << 8; }

// what a line does: -reason when refused, else one of the three below; site / word are set for WG_BB_MATCHED
#define WG_BB_MATCHED 0
#define WG_BB_NO_CHROM 1
#define WG_BB_NO_CPG 2
template <class T>
WG_HD int wg_bb_line_to_site(const T& t, int64_t p, int64_t n, uint64_t file_off, const wg_bb_chroms& c, const uint32_t* loci, int add_one,
                             int32_t& hint, int64_t& site, uint64_t& word)
{
    wg_bb_line ln;
    const int why = wg_bb_walk(t, p, n, ln);
    if (why) return -why;
    const int32_t r = wg_bb_find_chrom(t, ln.cs, ln.clen, c, hint);
    if (r < 0) return WG_BB_NO_CHROM;
    hint = r;
    site = wg_bb_find_locus(loci, c.lo[r], c.hi[r], ln.start + (add_one ? 1 : 0));
    if (site < 0) return WG_BB_NO_CPG;
    word = wg_bb_word(file_off, ln.meth, ln.total);
    return WG_BB_MATCHED;
}
