// fasta_core.h — the rule of `wgbstools init_genome`, one set of functions for host and device: what a byte of FASTA text is (a header,
// a byte of its name, a base, nothing), which bases are CpG sites, and what is refused.  No HIP needed: g++ compiles it alone.
//
//   header   a line that begins with '>' — as the first byte of the input or right after '\n' — up to the next '\n'
//   name     the bytes after '>' up to the first space, tab, '\r' or '\n'
//   base     every other byte that is not '\n' or '\r' (a '\r' is skipped wherever it stands); bases count from 1 in their sequence
//   site     a base C / c whose NEXT BASE in the same sequence is G / g, whatever line breaks lie between; its locus is the C's number
//
// This is the reference's ''.join(s.strip() for s in lines).upper() + finditer('CG') (init_genome.py:246-260) for every FASTA whose
// lines carry no blanks.  The state between two bytes is one of four (WG_FA_*), and '\n' leads to WG_FA_LS from every one of them: that
// is what lets a tile of text be summarised without knowing how it is entered (fasta_kernels.h).
//
// wg_fa_walk() is the one walk: the kernels run it over a thread's 16 bytes, wgbsseg_debug_fasta_walk over a whole text.  What it finds
// goes to a sink (header, name_byte, name_end, hit, pending, refuse); wg_fa_cur says where it stands.
#pragma once
#include <cstdint>
#include "bed_fmt.h"                   // WG_HD

#if defined(__HIPCC__)                 // (a member function: WG_HD's `static` on the host would say something else)
#define WG_HDM __host__ __device__ __forceinline__
#else
#define WG_HDM inline
#endif

#define WG_FA_MAX_NAME 255
#define WG_FA_MAX_BASES 0xfffffffeULL  // of one sequence: a locus is 32 bits and loci count from 1

#define WG_FA_LS 0                     // at the start of a line
#define WG_FA_SQ 1                     // inside a line of bases
#define WG_FA_NM 2                     // inside a header's name
#define WG_FA_HD 3                     // in the rest of a header

#define WG_FA_EV_NONE 0
#define WG_FA_EV_BASE 1
#define WG_FA_EV_HEADER 2              // the '>'
#define WG_FA_EV_NAME 3                // a byte of the name
#define WG_FA_EV_NAME_END 4            // the byte that ends the name

// the refusals; each comes with a byte offset of the uncompressed text, the smallest (offset << 8 | reason) wins
#define WG_FA_BAD_BEFORE 1             // a byte other than '\n' / '\r' before the first header         (the byte)
#define WG_FA_BAD_EMPTY_NAME 2         // a header with an empty name                                    (its '>')
#define WG_FA_BAD_LONG_NAME 3          // a name of more than WG_FA_MAX_NAME bytes                       (its '>')
#define WG_FA_BAD_BYTE 4               // a byte of a sequence outside 0x21 .. 0x7E                      (the byte)
#define WG_FA_BAD_LONG_SEQ 5           // a sequence of more than WG_FA_MAX_BASES bases                  (its '>')
#define WG_FA_BAD_REASONS 6

// a sequence as the engine records it: 280 bytes.  n_bases of sequence i is prev_bases of record i + 1 (the last one: the carry's)
struct wg_fa_seq {
    uint64_t hdr_off;                  // offset of the '>'
    uint64_t first_locus;              // sites of the sequences before it
    uint32_t prev_bases;               // the finished base count of the sequence before it
    uint32_t name_len;
    char name[WG_FA_MAX_NAME + 1];
};
static_assert(sizeof(wg_fa_seq) == 280, "the record table the host sizes");

// where a walk stands
struct wg_fa_cur {
    uint64_t seqs;                     // headers so far
    uint64_t bases;                    // bases of the current sequence so far
    uint64_t hits;                     // sites so far
    uint64_t hdr_off;                  // offset of the last header's '>'
    uint32_t state;
};

WG_HD int wg_fa_step(int s, uint8_t b, int* ev)
{
    *ev = WG_FA_EV_NONE;
    if (b == '\n') {
        if (s == WG_FA_NM) *ev = WG_FA_EV_NAME_END;
        return WG_FA_LS;
    }
    switch (s) {
    case WG_FA_LS:
        if (b == '>') { *ev = WG_FA_EV_HEADER; return WG_FA_NM; }
        /* fall through */
    case WG_FA_SQ:
        if (b != '\r') *ev = WG_FA_EV_BASE;
        return WG_FA_SQ;
    case WG_FA_NM:
        if (b == ' ' || b == '\t' || b == '\r') { *ev = WG_FA_EV_NAME_END; return WG_FA_HD; }
        *ev = WG_FA_EV_NAME;
        return WG_FA_NM;
    default:
        return WG_FA_HD;
    }
}

// the next base behind a C, from text[p] on (ls: text[p] begins a line): 1 it is G / g, 0 it is not (or a header, or a byte that is
// refused, comes first), -1 the text ends first
template <class Text>
WG_HD int wg_fa_next_is_g(const Text& T, int64_t n, int64_t p, bool ls)
{
    for (; p < n; p++) {
        const uint8_t b = (uint8_t)T.at(p);
        if (b == '\n') { ls = true; continue; }
        if (b == '\r') { ls = false; continue; }
        if (ls && b == '>') return 0;
        return (b | 0x20) == 'g' ? 1 : 0;
    }
    return -1;
}

// text[p0, p1) of a text of n bytes whose first byte has the offset abs0 in the input.  A C whose next base lies behind text[n) is
// left to the sink's pending().
template <class Text, class Sink>
WG_HD void wg_fa_walk(const Text& T, int64_t n, int64_t p0, int64_t p1, uint64_t abs0, wg_fa_cur& c, Sink& k)
{
    for (int64_t p = p0; p < p1; p++) {
        const uint8_t b = (uint8_t)T.at(p);
        const uint64_t at = abs0 + (uint64_t)p;
        int ev;
        const int next = wg_fa_step((int)c.state, b, &ev);
        if (ev == WG_FA_EV_BASE) {
            if (c.seqs == 0) k.refuse(at, WG_FA_BAD_BEFORE);
            else if (b < 0x21 || b > 0x7e) k.refuse(at, WG_FA_BAD_BYTE);
            c.bases++;
            if (c.bases == WG_FA_MAX_BASES + 1) k.refuse(c.hdr_off, WG_FA_BAD_LONG_SEQ);
            if ((b | 0x20) == 'c') {
                const int g = wg_fa_next_is_g(T, n, p + 1, false);
                if (g > 0) { k.hit(c.hits, c.bases); c.hits++; }
                else if (g < 0) k.pending(c.bases);
            }
        } else if (ev == WG_FA_EV_HEADER) {
            k.header(c, at);
            c.seqs++; c.bases = 0; c.hdr_off = at;
        } else if (ev == WG_FA_EV_NAME) {
            const uint64_t idx = at - c.hdr_off - 1;
            if (idx == WG_FA_MAX_NAME) k.refuse(c.hdr_off, WG_FA_BAD_LONG_NAME);
            if (idx < WG_FA_MAX_NAME) k.name_byte(c.seqs - 1, (uint32_t)idx, (char)b);
        } else if (ev == WG_FA_EV_NAME_END) {
            const uint64_t len = at - c.hdr_off - 1;
            if (len == 0) k.refuse(c.hdr_off, WG_FA_BAD_EMPTY_NAME);
            k.name_end(c.seqs - 1, len);
        }
        c.state = (uint32_t)next;
    }
}

// --- what a stretch of text does to a walk that enters it: it composes left to right (fasta_kernels.h) --------------------------------

// a map of the four states: two bits per entry state
#define WG_FA_MAP_ID 0xE4u             // 3 2 1 0
WG_HD uint32_t wg_fa_map_at(uint32_t m, uint32_t s) { return (m >> (2 * s)) & 3u; }
WG_HD uint32_t wg_fa_map_then(uint32_t first, uint32_t second)
{
    uint32_t r = 0;
    for (uint32_t s = 0; s < 4; s++) r |= wg_fa_map_at(second, wg_fa_map_at(first, s)) << (2 * s);
    return r;
}

// the counts of a stretch for ONE entry state.  T: uint32_t inside a tile, uint64_t over tiles
template <class T>
struct wg_fa_sum_t {
    T h;                               // headers
    T pre;                             // bases before the first header (all of them when h == 0)
    T post;                            // bases behind the last header (all of them when h == 0)
    T hits;
    T last;                            // where the last header begins (h > 0)
};
typedef wg_fa_sum_t<uint32_t> wg_fa_sum;
typedef wg_fa_sum_t<uint64_t> wg_fa_sum64;

template <class T>
WG_HD wg_fa_sum_t<T> wg_fa_sum_then(const wg_fa_sum_t<T>& a, const wg_fa_sum_t<T>& b)
{
    wg_fa_sum_t<T> r;
    r.h = a.h + b.h;
    r.pre = a.h ? a.pre : a.pre + b.pre;
    r.post = b.h ? b.post : a.post + b.post;
    r.hits = a.hits + b.hits;
    r.last = b.h ? b.last : a.last;
    return r;
}

// the walk that stands at `c`, behind a stretch with the counts s (s.last: an offset of the input)
WG_HD void wg_fa_cur_then(wg_fa_cur& c, const wg_fa_sum64& s)
{
    c.seqs += s.h;
    c.bases = s.h ? s.post : c.bases + s.post;
    c.hits += s.hits;
    if (s.h) c.hdr_off = s.last;
}

// the sink that counts one stretch: pre / post / last as wg_fa_sum has them, `last` relative to rel0
struct wg_fa_count_sink {
    wg_fa_sum s = {0, 0, 0, 0, 0};
    uint64_t rel0 = 0;
    WG_HDM void header(const wg_fa_cur& c, uint64_t at)
    {
        if (s.h == 0) s.pre = (uint32_t)c.bases;
        s.h++;
        s.last = (uint32_t)(at - rel0);
    }
    WG_HDM void name_byte(uint64_t, uint32_t, char) {}
    WG_HDM void name_end(uint64_t, uint64_t) {}
    WG_HDM void hit(uint64_t, uint64_t) { s.hits++; }
    WG_HDM void pending(uint64_t) {}
    WG_HDM void refuse(uint64_t, int) {}
    WG_HDM void close(const wg_fa_cur& c)
    {
        s.post = (uint32_t)c.bases;
        if (s.h == 0) s.pre = s.post;
    }
};

// text[p0, p1) entered in `state`: its counts (`last` relative to text[rel0]) and the state it leaves
template <class Text>
WG_HD wg_fa_sum wg_fa_count(const Text& T, int64_t n, int64_t p0, int64_t p1, int64_t rel0, uint32_t state, uint32_t* leaves)
{
    wg_fa_cur c = {1, 0, 0, 0, state};                             // (seqs 1: nothing is refused here, and name bytes have an index)
    wg_fa_count_sink k;
    k.rel0 = (uint64_t)rel0;
    c.hdr_off = (uint64_t)p0;                                      // (name indices stay small: they are not looked at)
    wg_fa_walk(T, n, p0, p1, 0, c, k);
    k.close(c);
    *leaves = c.state;
    return k.s;
}
