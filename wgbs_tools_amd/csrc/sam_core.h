// sam_core.h — the rules of `wgbstools bam2pat` on SAM text, one set of functions for host and device (like view_core.h and
// bed2beta_core.h): what of a line is read, which lines `samtools view -q -F -f` and the strand filter let through, how one line
// becomes a single-read pat (patter.cpp:105-184 compareSeqToRef, patter_utils.cpp:209-251 clean_CIGAR, :270-280 strip_pat), which lines
// are mates (patter.cpp:381-416, patter_utils.cpp:170-176) and how two pats merge (patter_utils.cpp:292-342 merge_PE).  No HIP needed: g++
// compiles it alone (tests/native/sam_host.cpp and san_bam2pat.cpp hand it to the tests); the kernels of sam_kernels.h call the same
// functions on text in global memory.
//
// The text is read through any `T` with `char at(int64_t i) const`; a line begins at byte p of text[0, n) and ends at the first '\n' at
// or behind p (the feed guarantees one before n).  Only the first ten fields are read: QUAL and the tags are stepped over.
//
// The adjusted sequence of clean_CIGAR is never made: wg_sam_cursor walks the CIGAR forwards and answers "which base stands at index i"
// for ascending i, and the loci of the chromosome are walked beside it.
#pragma once
#include <cstdint>
#include "bed2beta_core.h"             // WG_HD, wg_bb_chroms, wg_bb_find_chrom

#if defined(__HIPCC__)
#define WG_HDM __host__ __device__ __forceinline__
#else
#define WG_HDM inline
#endif

#define WG_SAM_MAX_QNAME 254           // the SAM specification's limit; a longer QNAME makes the line invalid, and it pairs with nothing
#define WG_SAM_MAX_PE 300              // MAX_PE_PAT_LEN: a merged pair that spans more sites is dropped
#define WG_SAM_MAX_NUMBER 0x7fffffffLL // FLAG, MAPQ, a CIGAR length: what std::stoi holds

// what a line is.  The first four never reach the pairing; the last three keep their place in it.
#define WG_SAM_HEADER 1                // begins with '@'
#define WG_SAM_FILTERED 2              // FLAG / MAPQ / strand
#define WG_SAM_UNKNOWN 3               // its RNAME is not a chromosome of the dictionary
#define WG_SAM_INVALID 4               // fewer than 11 fields, a FLAG / POS / MAPQ that is not a number, a bad CIGAR, a QNAME above 254 bytes
#define WG_SAM_EMPTY 5                 // no called site
#define WG_SAM_PAT 6                   // a pat: sites [start, start + plen)

WG_HD bool wg_sam_participates(int state) { return state >= WG_SAM_INVALID; }

#define WG_SAM_BOTH 0                  // wg_sam_params.strand
#define WG_SAM_TOP 1
#define WG_SAM_BOTTOM 2

struct wg_sam_params {
    uint32_t exclude, include;         // samtools view -F, -f
    int32_t mapq;                      // -q
    int32_t paired;                    // the file is paired-end (FLAG & 1 of its first alignment)
    int32_t strand;
    int32_t clip, min_cpg;
};

struct wg_sam_text {
    const char* p;
    WG_HDM char at(int64_t i) const { return p[i]; }
};

// The tokens of the line at byte p as patter's line2tokens counts them (a last empty field is no token), at most 11: field k < 10 is
// bytes [p + fb[k], p + fe[k]).  Field 11 is only looked at: is it there.
template <class T>
WG_HD int wg_sam_split(const T& t, int64_t p, int64_t n, uint32_t* fb, uint32_t* fe)
{
    int k = 0;
    int64_t i = p, start = p;
    for (; i < n; i++) {
        const char ch = t.at(i);
        if (ch == '\n') break;
        if (ch != '\t') continue;
        fb[k] = (uint32_t)(start - p); fe[k] = (uint32_t)(i - p);
        k++;
        start = i + 1;
        if (k == 10) break;
    }
    if (k == 10) return i + 1 < n && t.at(i + 1) != '\n' ? 11 : 10;
    if (i > start) { fb[k] = (uint32_t)(start - p); fe[k] = (uint32_t)(i - p); k++; }
    return k;
}

// the field [b, e) as a number: 1 or more decimal digits and nothing else, at most `max`
template <class T>
WG_HD bool wg_sam_number(const T& t, int64_t b, int64_t e, int64_t max, int64_t& val)
{
    if (e <= b) return false;
    int64_t v = 0;
    for (; b < e; b++) {
        const char ch = t.at(b);
        if (ch < '0' || ch > '9') return false;
        if (v <= max) v = v * 10 + (ch - '0');
    }
    if (v > max) return false;
    val = v;
    return true;
}

// samtools view -q -F -f, and the awk of --top_strand / --bottom_strand (bam2pat.py:159-170)
WG_HD bool wg_sam_keep(uint32_t flag, int64_t mapq, const wg_sam_params& a)
{
    if ((flag & a.exclude) != 0 || (flag & a.include) != a.include || mapq < a.mapq) return false;
    if (a.strand == WG_SAM_TOP) return a.paired ? flag == 99 || flag == 147 : flag == 0;
    if (a.strand == WG_SAM_BOTTOM) return a.paired ? flag == 83 || flag == 163 : flag == 16;
    return true;
}

// patter_utils.cpp:163-168
WG_HD bool wg_sam_is_bottom(uint32_t flag, bool paired)
{
    return paired ? (flag & 0x53) == 83 || (flag & 0xA3) == 163 : (flag & 0x10) != 0;
}

// clean_CIGAR without its string: M = X copy, D N insert 'N', I S skip, H nothing; false for any other operation, '*', an operation
// without a number, a number above 2^31 - 1 and an M / = / X / I / S that runs past SEQ.  Digits behind the last operation are ignored,
// as there.  adj_len: the length of the adjusted sequence.
template <class T>
WG_HD bool wg_sam_cigar_check(const T& t, int64_t cb, int64_t ce, int64_t seq_len, int64_t& adj_len)
{
    int64_t num = 0, used = 0, adj = 0;
    bool digits = false;
    for (int64_t i = cb; i < ce; i++) {
        const char c = t.at(i);
        if (c >= '0' && c <= '9') {
            if (num <= WG_SAM_MAX_NUMBER) num = num * 10 + (c - '0');
            digits = true;
            continue;
        }
        if (!digits || num > WG_SAM_MAX_NUMBER) return false;
        if (c == 'M' || c == '=' || c == 'X') {
            if (num > seq_len - used) return false;
            used += num; adj += num;
        } else if (c == 'D' || c == 'N') adj += num;
        else if (c == 'I' || c == 'S') {
            if (num > seq_len - used) return false;
            used += num;
        } else if (c != 'H') return false;
        num = 0;
        digits = false;
    }
    adj_len = adj;
    return true;
}

// The adjusted sequence of a checked CIGAR, read forwards: at(i) for ascending i is its byte i, 0 behind its end.
template <class T>
struct wg_sam_cursor {
    const T* t;
    int64_t ci, ce;                    // the CIGAR bytes not yet read
    int64_t seq;                       // SEQ's first byte
    int64_t a0, a1, s0;                // the operation at hand covers [a0, a1) of the adjusted sequence from SEQ's byte s0 on (-1: inserted 'N')
    int64_t used;                      // bytes of SEQ the operations so far took
    WG_HDM char at(int64_t i)
    {
        while (i >= a1) {
            int64_t num = 0;
            char c = 0;
            while (ci < ce && (c = t->at(ci)) >= '0' && c <= '9') { num = num * 10 + (c - '0'); ci++; }
            if (ci >= ce) return 0;
            ci++;
            if (c == 'M' || c == '=' || c == 'X') { a0 = a1; a1 += num; s0 = used; used += num; }
            else if (c == 'D' || c == 'N') { a0 = a1; a1 += num; s0 = -1; }
            else if (c == 'I' || c == 'S') used += num;
        }
        return s0 < 0 ? 'N' : t->at(seq + s0 + (i - a0));
    }
};

// what of a line the calling needs: where its CIGAR and SEQ lie, POS, the adjusted length, the strand
struct wg_sam_geom {
    int64_t cb, ce, sb, pos, adj_len;
    bool bottom;
};

template <class T>
WG_HD wg_sam_cursor<T> wg_sam_begin(const T& t, const wg_sam_geom& g) { return {&t, g.cb, g.ce, g.sb, 0, 0, -1, 0}; }

// compareSeqToRef at the CpG whose locus is POS + i: C / T / '.'.  A top read shows the C itself (C or T before G), a bottom read the
// base opposite (G or A behind C); `clip` hides the call when the looked-at index j lies in the first or last `clip` bases.
template <class C>
WG_HD char wg_sam_call(C& cur, int64_t i, const wg_sam_geom& g, int64_t clip)
{
    const char x = cur.at(i), y = cur.at(i + 1);                    // (0 behind the end: no CpG there)
    const int64_t j = g.bottom ? i + 1 : i;
    char c = '.';
    if (!g.bottom) { if (y == 'G') c = x == 'C' ? 'C' : x == 'T' ? 'T' : '.'; }
    else if (x == 'C') c = y == 'G' ? 'C' : y == 'A' ? 'T' : '.';
    return j >= clip && j < g.adj_len - clip ? c : '.';
}

// the first locus at or behind p among loci[lo, hi)
WG_HD int64_t wg_sam_lower_bound(const uint32_t* loci, int64_t lo, int64_t hi, int64_t p)
{
    int64_t a = lo, b = hi;
    while (a < b) {
        const int64_t m = a + ((b - a) >> 1);
        if ((int64_t)loci[m] < p) a = m + 1; else b = m;
    }
    return a;
}

// The single-read pat of a line: the calls at the chromosome's CpGs inside the adjusted sequence, from the first called site to the
// last.  first: the index in loci of the first called site (its site number is first + 1), plen: the sites; false: no called site.
template <class T>
WG_HD bool wg_sam_line_pat(const T& t, const wg_sam_geom& g, const uint32_t* loci, int64_t lo, int64_t hi, int64_t clip, int64_t& first, int64_t& plen)
{
    wg_sam_cursor<T> cur = wg_sam_begin(t, g);
    int64_t f = -1, l = -1;
    for (int64_t li = wg_sam_lower_bound(loci, lo, hi, g.pos); li < hi; li++) {
        const int64_t i = (int64_t)loci[li] - g.pos;
        if (i >= g.adj_len) break;
        if (wg_sam_call(cur, i, g, clip) != '.') { if (f < 0) f = li; l = li; }
    }
    if (f < 0) return false;
    first = f; plen = l - f + 1;
    return true;
}

// byte k of a line's pat for ascending k: the call at the site of index first + k
template <class T>
struct wg_sam_pat_of_line {
    wg_sam_cursor<T> cur;
    wg_sam_geom g;
    const uint32_t* loci;
    int64_t first, clip;
    WG_HDM char operator()(int64_t k) { return wg_sam_call(cur, (int64_t)loci[first + k] - g.pos, g, clip); }
};

template <class T>
WG_HD wg_sam_pat_of_line<T> wg_sam_pat_begin(const T& t, const wg_sam_geom& g, const uint32_t* loci, int64_t first, int64_t clip)
{
    return {wg_sam_begin(t, g), g, loci, first, clip};
}

// byte k of a pat that lies in memory
struct wg_sam_pat_of_bytes {
    const char* p;
    WG_HDM char operator()(int64_t k) const { return p[k]; }
};

// What is known of a line once it has been read (k_sam_eval keeps one per line): its state, the rank of its chromosome (-1: none), its
// QNAME's length (255: longer than WG_SAM_MAX_QNAME) and, for a pat, its first site (1-based) and its length.
struct wg_sam_read {
    int64_t start;
    uint32_t line;                     // the line's first byte in its chunk
    uint32_t plen;
    int32_t rank;
    uint16_t qlen;
    uint8_t state, bottom;
};

// the geometry of the line at byte p, whose fields have been split: false when POS or the CIGAR makes the line invalid
template <class T>
WG_HD bool wg_sam_geom_of(const T& t, int64_t p, const uint32_t* fb, const uint32_t* fe, uint32_t flag, bool paired, wg_sam_geom& g)
{
    if (!wg_sam_number(t, p + fb[3], p + fe[3], 0xffffffffLL, g.pos)) return false;
    g.cb = p + fb[5]; g.ce = p + fe[5]; g.sb = p + fb[9];
    g.bottom = wg_sam_is_bottom(flag, paired);
    return wg_sam_cigar_check(t, g.cb, g.ce, (int64_t)fe[9] - (int64_t)fb[9], g.adj_len);
}

// The line at byte p -> its wg_sam_read.  Order: header; too few fields or a FLAG / MAPQ that is not a number (invalid: such a line
// cannot be filtered and keeps its place among the mates); the filter; an RNAME the dictionary does not have; a QNAME above 254 bytes, POS, the
// CIGAR (invalid); the calls.  An invalid line is looked up too: mates are lines of one chromosome, and an invalid line that names none
// of the dictionary's is in no chromosome's stream of the reference: it is dropped as an unknown chromosome is.
template <class T>
WG_HD wg_sam_read wg_sam_eval(const T& t, int64_t p, int64_t n, const wg_sam_params& a, const wg_bb_chroms& c, const uint32_t* loci)
{
    wg_sam_read r = {0, (uint32_t)p, 0u, -1, 0, WG_SAM_INVALID, 0};
    if (t.at(p) == '@') { r.state = WG_SAM_HEADER; return r; }
    uint32_t fb[10], fe[10];
    const int nf = wg_sam_split(t, p, n, fb, fe);
    const uint32_t ql = nf > 0 ? fe[0] - fb[0] : 0u;
    r.qlen = (uint16_t)(ql > WG_SAM_MAX_QNAME ? WG_SAM_MAX_QNAME + 1 : ql);
    if (nf >= 3) r.rank = wg_bb_find_chrom(t, p + fb[2], (int64_t)fe[2] - (int64_t)fb[2], c, -1);
    int64_t flag = 0, mapq = 0;
    if (nf < 11 || !wg_sam_number(t, p + fb[1], p + fe[1], WG_SAM_MAX_NUMBER, flag) || !wg_sam_number(t, p + fb[4], p + fe[4], WG_SAM_MAX_NUMBER, mapq)) {
        if (r.rank < 0) r.state = WG_SAM_UNKNOWN;                   // (no chromosome's stream holds it)
        return r;
    }
    if (!wg_sam_keep((uint32_t)flag, mapq, a)) { r.state = WG_SAM_FILTERED; return r; }
    if (r.rank < 0) { r.state = WG_SAM_UNKNOWN; return r; }
    wg_sam_geom g;
    if (ql > WG_SAM_MAX_QNAME || !wg_sam_geom_of(t, p, fb, fe, (uint32_t)flag, a.paired != 0, g)) return r;
    r.bottom = g.bottom ? 1 : 0;
    int64_t first = 0, plen = 0;
    if (!wg_sam_line_pat(t, g, loci, c.lo[r.rank], c.hi[r.rank], a.clip, first, plen)) { r.state = WG_SAM_EMPTY; return r; }
    r.state = WG_SAM_PAT;
    r.start = first + 1;
    r.plen = (uint32_t)plen;
    return r;
}

// the geometry of a line that wg_sam_eval found to be a pat, again (the kernels keep the summary, not the geometry)
template <class T>
WG_HD wg_sam_geom wg_sam_geom_again(const T& t, int64_t p, int64_t n, bool bottom)
{
    uint32_t fb[10], fe[10];
    (void)wg_sam_split(t, p, n, fb, fe);
    wg_sam_geom g = {p + fb[5], p + fe[5], p + fb[9], 0, 0, bottom};
    (void)wg_sam_number(t, p + fb[3], p + fe[3], 0xffffffffLL, g.pos);
    (void)wg_sam_cigar_check(t, g.cb, g.ce, (int64_t)fe[9] - (int64_t)fb[9], g.adj_len);
    return g;
}

// are_paired, per chromosome: the QNAMEs [qa, qa + la) of ta and [qb, qb + lb) of tb are equal byte for byte and the two lines name one
// chromosome.  (The reference streams every chromosome by itself, so only lines of one chromosome ever meet there.)
template <class TA, class TB>
WG_HD bool wg_sam_same_read(const TA& ta, int64_t qa, uint32_t la, int32_t rank_a, const TB& tb, int64_t qb, uint32_t lb, int32_t rank_b)
{
    if (la != lb || la > WG_SAM_MAX_QNAME || rank_a != rank_b) return false;
    for (uint32_t i = 0; i < la; i++)
        if (ta.at(qa + i) != tb.at(qb + i)) return false;
    return true;
}

// merge_PE of two pats (sites [sa, sa + la) and [sb, sb + lb), bytes pa(k) / pb(k) for ascending k): the earlier start first, a site
// both call differently becomes '.', trailing then leading dots go.  out(k, c): byte k of the span before the dots go (k ascending).
#define WG_SAM_MERGE_TOO_LONG 1        // the span exceeds WG_SAM_MAX_PE: the pair is dropped
#define WG_SAM_MERGE_EMPTY 2           // nothing but dots is left
struct wg_sam_merged {
    int why;                           // 0: a pat
    int64_t rs;                        // its first site
    int64_t first, len;                // bytes [first, first + len) of the span
};

template <class PA, class PB, class Out>
WG_HD wg_sam_merged wg_sam_merge(int64_t sa, int64_t la, PA&& pa, int64_t sb, int64_t lb, PB&& pb, Out&& out)
{
    const int64_t s = sa < sb ? sa : sb, last = sa + la > sb + lb ? sa + la : sb + lb;
    wg_sam_merged m = {WG_SAM_MERGE_TOO_LONG, 0, 0, 0};
    if (last - s > WG_SAM_MAX_PE) return m;
    int64_t first = -1, end = 0;
    for (int64_t k = 0; k < last - s; k++) {
        const int64_t site = s + k;
        const char a = site >= sa && site < sa + la ? pa(site - sa) : '.';
        const char b = site >= sb && site < sb + lb ? pb(site - sb) : '.';
        const char c = a == '.' ? b : b != '.' && b != a ? '.' : a;
        out(k, c);
        if (c != '.') { if (first < 0) first = k; end = k + 1; }
    }
    if (first < 0) { m.why = WG_SAM_MERGE_EMPTY; return m; }
    m.why = 0; m.rs = s + first; m.first = first; m.len = end - first;
    return m;
}

// the place of a line in its run of equal names: (0, 1), (2, 3), ... pair; an even place without a successor is single
WG_HD bool wg_sam_is_first(uint64_t place) { return (place & 1u) == 0; }

// What one chunk leaves for the next: the last line that keeps its place among the mates.  When that line is the first of a possible
// pair and a pat, it stands in the record table as a single read (count 1, or 0 when it is shorter than --min_cpg) and `rec` names the
// record: a mate at the head of the next chunk reads its bytes there, clears its count and adds the merged read.  So the bytes that
// come out do not depend on where the text is cut.
struct wg_sam_carry {
    int64_t rec;                       // the record of that single read; -1: none (the line is invalid, empty, or the second of its pair)
    int64_t start;                     // its pat: first site and length (state == WG_SAM_PAT)
    uint32_t plen;
    int32_t rank;
    uint32_t place;                    // its place in its run of equal names
    uint16_t qlen;
    uint8_t state, has;                // has: there is such a line
    char qname[WG_SAM_MAX_QNAME + 2];
};

// the counters of an engine, in the order wgbsseg_patview_sam_info reports them
#define WG_SAM_N_LINES 0
#define WG_SAM_N_HEADER 1
#define WG_SAM_N_FILTERED 2
#define WG_SAM_N_INVALID 3
#define WG_SAM_N_UNKNOWN 4
#define WG_SAM_N_EMPTY 5
#define WG_SAM_N_SHORT 6
#define WG_SAM_N_PAIRS 7
#define WG_SAM_N_LEFT_SINGLE 8
#define WG_SAM_N_TOO_LONG 9
#define WG_SAM_COUNTERS 10
