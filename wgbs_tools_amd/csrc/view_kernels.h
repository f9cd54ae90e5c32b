// view_kernels.h — `wgbstools view` / `cview` on gfx950: the reads of a pat file that an interval lets through, cut as --strict / --strip
// / --min_len / --no_gaps ask (view_core.h), kept on the device across chunks, then sorted, collapsed and written out as pat text.
// The pat text format comes from pat_kernels.h (PatTile, PatText, wg_pat_tile_lines, wg_pat_parse_line, wg_pat_site_before,
// wg_pat_is_last_read), the scan of per-workgroup totals from bed_kernels.h (k_bed_scan), the digits from bed_fmt.h.
//
// Selection is a test on the read alone.  The reference streams the reads past ONE block [s, e) (cview.cpp:87-128): it stops reading at
// the first read with rs >= e and skips a read that ends before s.  On reads that ascend by start every read behind the stopping one
// starts at or after e too, so "dropped iff rs >= e or rs + len - 1 < s" says the same read by read (the argument of frag_kernels.h
// with a single block) — provided the reads do ascend, which k_view_measure checks always, the whole genome included.
//
// Per fed chunk (one workgroup per 4 KB tile of text, one line per thread, as k_pat_count):
//   k_view_measure   parses the tile's lines, applies the cut rule, reports the lowest malformed (`bad`) and descending (`desc`) line and
//                    the lowest line whose count is below 1 (`low`: finish() looks at it only for a view over several files), and
//                    writes the tile's number of survivors and the bytes they put into the arena
//   (k_bed_scan)     twice: the tiles' first record and first arena byte in the chunk
//   k_view_pack      parses again and writes every survivor's record and bytes (chromosome, cut pattern) at tile offset + prefix inside
//                    the tile: input order, no atomics — the unsorted modes and the tie-break of the sort rest on it
// With a site mask (`wgbstools mask_pat`, wgbsseg_patview_set_mask):
//   k_view_mask_fill once: the bitmap of hidden sites (view_core.h wg_view_mask) from the disjoint intervals of mask_plan.h
//   k_view_measure_masked / k_view_pack_masked   the same two bodies (template <bool MASKED>) with view_core.h's masked cut: both see a
//                    hidden site as '.', so they agree on survivors and arena bytes, and the pack pass writes the '.'.  A read takes its
//                    hidden bits 64 sites at a time (wg_view_hidden64: at most three words of a bitmap that lives in L2).
// At finish, over the n records:
//   k_view_inorder   is the input order already the sorted one?  (then the sort is skipped)
//   k_view_sort_runs every workgroup sorts WG_VIEW_RUN indices in LDS (bitonic network; wg_view_less is a strict total order, so the
//                    network's result does not depend on how it gets there)
//   k_view_merge     one merge pass between two permutation buffers: every thread finds the start of its WG_VIEW_MERGE_ITEMS
//                    output elements by a merge-path binary search on its diagonal and merges them serially, ties from the left
//   k_view_heads     run heads over the (permuted) records, per-workgroup sums of counts and heads
//   k_view_tails     after the scans: the running int64 sum at every run's last line, stored by run number
//   k_view_runs      a run's sum = the difference of two neighbours; whether it prints, its line's length, the 10^15 flag
//   k_view_emit      after the scan: every printing run writes its line
// With sources and labels (`wgbstools mix_pat`, wgbsseg_patview_set_source / _set_labels):
//   k_view_measure_sampled / k_view_pack_sampled   the same two bodies (template <bool MASKED, bool SAMPLED>): a read the cut lets through is
//                    thinned by view_core.h's wg_view_sample — a function of the line's byte offset in its file, so both passes draw the
//                    same number — and kept with its new count when that is above 0; its record carries the rank of the file's label
//   the label kernels at the end of this file stand in for k_view_runs and k_view_emit
// Plain C++ only.
#pragma once
#include "pat_kernels.h"
#include "bed_kernels.h"
#include "view_core.h"
#include "view_plan.h"
#include "mask_plan.h"

static_assert(WG_BED_BLOCK == WG_BLOCK, "k_bed_scan's totals and the view kernels' workgroups are both 256 wide");
static_assert(WG_VIEW_RUN == 2 * WG_BLOCK, "one compare-exchange per thread and step of the network");

struct wg_view_args { int64_t s, e, min_len; int flags; };

// the source of the file being fed (wgbsseg_patview_set_source): the draw of view_core.h's wg_view_sample and the label of its reads.
// at: the offset inside the file of the chunk's first byte.  over / stats: the lowest line with count * reps above WG_VIEW_MAX_DRAWS |
// the reads that reached the sampler, those it dropped, the sum of the counts it kept (integer atomics: no order shows)
struct wg_view_source {
    uint64_t seed, at;
    uint32_t T, stream, reps, rank;
    unsigned long long *over, *stats;
};

// the labels in rank order: label k is bytes[off[k], off[k + 1])
struct wg_view_labels {
    const char* bytes;
    const uint32_t* off;
};

// what a thread knows of its line
struct wg_view_line {
    bool ok, keep, drawn, over;                                    // drawn: the read reached the sampler | over: count * reps is above the cap
    int64_t site, ps;
    uint32_t clen;
    int32_t count;
    wg_view_cut cut;
};

// the line that begins at byte p: malformed (fewer than four fields, a site / count that is not a number, an empty pattern, any byte
// between the count's digits and the newline), or parsed and cut
template <bool MASKED, bool SAMPLED = false>
__device__ __forceinline__ wg_view_line wg_view_eval(const PatText& T, int64_t p, int64_t n, const wg_view_args& a, const wg_view_mask& m, const wg_view_source* q = nullptr)
{
    wg_view_line L = {};
    int64_t plen = 0, count = 0;
    if (!wg_pat_parse_line(T, p, n, L.site, L.ps, plen, count) || plen <= 0) return L;
    int64_t i = L.ps + plen + 1, again = 0;
    (void)wg_parse_int(T, i, n, again);                             // (to the end of the count's digits)
    if (!(i < n && T.at(i) == '\n')) return L;
    L.ok = true;
    L.count = (int32_t)count;
    const int64_t ps = L.ps;
    if constexpr (MASKED) L.cut = wg_view_cut_read_masked(L.site, plen, [&](int64_t k) { return T.at(ps + k); }, m, a.s, a.e, a.flags, a.min_len);
    else L.cut = wg_view_cut_read(L.site, plen, [&](int64_t k) { return T.at(ps + k); }, a.s, a.e, a.flags, a.min_len);
    L.keep = L.cut.len > 0;
    if constexpr (SAMPLED) {                                        // a read the cut lets through is drawn: the same draw in both passes
        if (L.keep && count >= 1) {                                 // (a count below 1 is refused at finish(): `low`)
            L.drawn = true;
            L.over = count * (int64_t)q->reps > WG_VIEW_MAX_DRAWS;
            L.count = L.over ? 0 : (int32_t)wg_view_sample(count, q->reps, q->T, q->seed, q->stream, q->at + (uint64_t)p);
            L.keep = L.count > 0;
        }
    }
    if (L.keep) {
        int64_t c = p;
        while (T.at(c) != '\t') c++;
        L.clen = (uint32_t)(c - p);
    }
    return L;
}

// inclusive prefix sum of v over the workgroup and its total; sh: WG_BLOCK / 64 words of LDS, free again on return
__device__ __forceinline__ uint64_t wg_view_block_incl_u64(uint64_t v, uint64_t* sh, uint64_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t incl = wg_wave_incl_scan_u64(v, lane);
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WG_BLOCK / 64; w++) {
        const uint64_t t = sh[w];
        if (w < wave) before += t;
        all += t;
    }
    total = all;
    __syncthreads();
    return before + incl;
}

template <bool MASKED, bool SAMPLED = false>
__device__ __forceinline__ void wg_view_measure(const char* __restrict__ text, int64_t n, const wg_view_args& a, const wg_view_mask& m, uint64_t* __restrict__ tile_recs,
                                                uint64_t* __restrict__ tile_bytes, unsigned long long* bad, unsigned long long* desc,
                                                unsigned long long* low, const long long* prev_in, long long* prev_out, unsigned long long chunk_off,
                                                const wg_view_source* q = nullptr)
{
    __shared__ PatTile tile;
    __shared__ long long s_last[WG_BLOCK / 64];              // the start of every wavefront's last line in the round (WG_PAT_NO_SITE: no line / malformed)
    __shared__ long long s_prev;                             // the start of the read before the round's first line
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * WG_PAT_TILE;
    if (tid == 0) s_prev = wg_pat_site_before(text, n, base, prev_in);
    const uint32_t total = wg_pat_tile_lines(text, n, base, tile);   // (synchronises: s_prev visible)
    const PatText T = tile.text(text, base, n);
    uint64_t recs = 0, bytes = 0;
    for (uint32_t r0 = 0; r0 < total; r0 += WG_BLOCK) {
        const uint32_t l = r0 + (uint32_t)tid;
        wg_view_line L = {};
        if (l < total) {
            const int64_t p = base + tile.lstart[l];
            L = wg_view_eval<MASKED, SAMPLED>(T, p, n, a, m, q);
            if (!L.ok) atomicMin(bad, chunk_off + (unsigned long long)p);
            else if (L.count < 1 && !L.drawn) atomicMin(low, chunk_off + (unsigned long long)p);     // (a drawn read's count was at least 1)
            if (SAMPLED && L.over) atomicMin(q->over, chunk_off + (unsigned long long)p);
        }
        const long long mine = L.ok ? (long long)L.site : WG_PAT_NO_SITE;
        long long pv = __shfl_up(mine, 1);                       // the line before: the lane below, ...
        if (lane == 63) s_last[wv] = mine;
        __syncthreads();
        if (lane == 0) pv = wv ? s_last[wv - 1] : s_prev;        // ... the wavefront below, or the round / tile / chunk before
        if (L.ok) {
            if (pv != WG_PAT_NO_SITE && L.site < pv) atomicMin(desc, chunk_off + (unsigned long long)(base + tile.lstart[l]));
            if (l == total - 1 && wg_pat_is_last_read(T, L.ps, 1, n)) *prev_out = L.site;   // (from the pattern's first byte: the same walk to the line's end)
        }
        uint64_t rr, bb;
        (void)wg_view_block_incl_u64(L.keep ? 1u : 0u, sh, rr);  // (its barriers: s_last read before the next round rewrites it)
        (void)wg_view_block_incl_u64(L.keep ? (uint64_t)L.clen + (uint64_t)L.cut.len : 0u, sh, bb);
        recs += rr; bytes += bb;
        if constexpr (SAMPLED) {
            uint64_t reached, dropped, kept;
            (void)wg_view_block_incl_u64(L.drawn ? 1u : 0u, sh, reached);
            (void)wg_view_block_incl_u64(L.drawn && !L.keep ? 1u : 0u, sh, dropped);
            (void)wg_view_block_incl_u64(L.drawn && L.keep ? (uint64_t)L.count : 0u, sh, kept);
            if (tid == 0 && reached) {
                atomicAdd(q->stats, (unsigned long long)reached);
                atomicAdd(q->stats + 1, (unsigned long long)dropped);
                atomicAdd(q->stats + 2, (unsigned long long)kept);
            }
        }
        if (tid == 0) s_prev = s_last[WG_BLOCK / 64 - 1];        // the next round's first line follows this round's last
        __syncthreads();
    }
    if (tid == 0) { tile_recs[blockIdx.x] = recs; tile_bytes[blockIdx.x] = bytes; }
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_measure(const char* __restrict__ text, int64_t n, wg_view_args a, uint64_t* __restrict__ tile_recs,
                                                           uint64_t* __restrict__ tile_bytes, unsigned long long* bad, unsigned long long* desc,
                                                           unsigned long long* low, const long long* prev_in, long long* prev_out, unsigned long long chunk_off)
{
    wg_view_measure<false>(text, n, a, wg_view_mask{nullptr, 0, 0}, tile_recs, tile_bytes, bad, desc, low, prev_in, prev_out, chunk_off);
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_measure_masked(const char* __restrict__ text, int64_t n, wg_view_args a, wg_view_mask m, uint64_t* __restrict__ tile_recs,
                                                                  uint64_t* __restrict__ tile_bytes, unsigned long long* bad, unsigned long long* desc,
                                                                  unsigned long long* low, const long long* prev_in, long long* prev_out, unsigned long long chunk_off)
{
    wg_view_measure<true>(text, n, a, m, tile_recs, tile_bytes, bad, desc, low, prev_in, prev_out, chunk_off);
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_measure_sampled(const char* __restrict__ text, int64_t n, wg_view_args a, wg_view_source q, uint64_t* __restrict__ tile_recs,
                                                                   uint64_t* __restrict__ tile_bytes, unsigned long long* bad, unsigned long long* desc,
                                                                   unsigned long long* low, const long long* prev_in, long long* prev_out, unsigned long long chunk_off)
{
    wg_view_measure<false, true>(text, n, a, wg_view_mask{nullptr, 0, 0}, tile_recs, tile_bytes, bad, desc, low, prev_in, prev_out, chunk_off, &q);
}

// rec_base / arena_base: the scans of k_view_measure's totals; rec0 / arena0: what the chunks before left in the two buffers
template <bool MASKED, bool SAMPLED = false>
__device__ __forceinline__ void wg_view_pack(const char* __restrict__ text, int64_t n, const wg_view_args& a, const wg_view_mask& m, const uint64_t* __restrict__ rec_base,
                                             const uint64_t* __restrict__ arena_base, uint64_t rec0, uint64_t arena0,
                                             wg_view_rec* __restrict__ recs, char* __restrict__ arena, const wg_view_source* q = nullptr)
{
    __shared__ PatTile tile;
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * WG_PAT_TILE;
    const uint32_t total = wg_pat_tile_lines(text, n, base, tile);
    const PatText T = tile.text(text, base, n);
    uint64_t r_at = rec0 + rec_base[blockIdx.x], a_at = arena0 + arena_base[blockIdx.x];
    for (uint32_t r0 = 0; r0 < total; r0 += WG_BLOCK) {
        const uint32_t l = r0 + (uint32_t)tid;
        wg_view_line L = {};
        int64_t p = 0;
        if (l < total) {
            p = base + tile.lstart[l];
            L = wg_view_eval<MASKED, SAMPLED>(T, p, n, a, m, q);
        }
        const uint64_t mine = L.keep ? (uint64_t)L.clen + (uint64_t)L.cut.len : 0u;
        uint64_t rr, bb;
        const uint64_t ir = wg_view_block_incl_u64(L.keep ? 1u : 0u, sh, rr);
        const uint64_t ib = wg_view_block_incl_u64(mine, sh, bb);
        if (L.keep) {
            wg_view_rec r;
            r.off = a_at + ib - mine;
            r.rs = L.cut.rs;
            r.count = L.count;
            r.clen = L.clen;
            r.plen = (uint32_t)L.cut.len;
            if constexpr (SAMPLED) r.line = q->rank; else r.line = 0;
            recs[r_at + ir - 1] = r;
            char* dst = arena + r.off;
            for (uint32_t j = 0; j < L.clen; j++) dst[j] = T.at(p + j);
            dst += L.clen;
            const int64_t from = L.ps + L.cut.first;               // (a 1,500-CpG read: past the staged bytes T.at reads global memory)
            if constexpr (MASKED) {                                // byte cut.first + j of the read: '.' where its site is hidden
                wg_view_window w = {-1, 0};
                for (int64_t j = 0; j < L.cut.len; j++) dst[j] = wg_view_hidden_at(m, w, L.site, L.cut.first + j) ? '.' : T.at(from + j);
            } else {
                for (int64_t j = 0; j < L.cut.len; j++) dst[j] = T.at(from + j);
            }
        }
        r_at += rr; a_at += bb;
    }
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_pack(const char* __restrict__ text, int64_t n, wg_view_args a, const uint64_t* __restrict__ rec_base,
                                                        const uint64_t* __restrict__ arena_base, uint64_t rec0, uint64_t arena0,
                                                        wg_view_rec* __restrict__ recs, char* __restrict__ arena)
{
    wg_view_pack<false>(text, n, a, wg_view_mask{nullptr, 0, 0}, rec_base, arena_base, rec0, arena0, recs, arena);
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_pack_masked(const char* __restrict__ text, int64_t n, wg_view_args a, wg_view_mask m, const uint64_t* __restrict__ rec_base,
                                                               const uint64_t* __restrict__ arena_base, uint64_t rec0, uint64_t arena0,
                                                               wg_view_rec* __restrict__ recs, char* __restrict__ arena)
{
    wg_view_pack<true>(text, n, a, m, rec_base, arena_base, rec0, arena0, recs, arena);
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_pack_sampled(const char* __restrict__ text, int64_t n, wg_view_args a, wg_view_source q, const uint64_t* __restrict__ rec_base,
                                                                const uint64_t* __restrict__ arena_base, uint64_t rec0, uint64_t arena0,
                                                                wg_view_rec* __restrict__ recs, char* __restrict__ arena)
{
    wg_view_pack<false, true>(text, n, a, wg_view_mask{nullptr, 0, 0}, rec_base, arena_base, rec0, arena0, recs, arena, &q);
}

// One thread per word of the bitmap over [lo, lo + 32 n_words): the word is composed in registers from the disjoint ascending intervals
// (mask_plan.h wg_mask_word: a binary search, then the intervals that reach into the word) and written with one ordinary store.  No
// atomics: the bitmap does not depend on scheduling.
__global__ __launch_bounds__(WG_BLOCK) void k_view_mask_fill(const int64_t* __restrict__ starts, const int64_t* __restrict__ ends, int64_t n_intervals, int64_t lo,
                                                             int64_t n_words, uint32_t* __restrict__ words)
{
    const int64_t w = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (w < n_words) words[w] = wg_mask_word(starts, ends, n_intervals, lo, w);
}

// ------------------------------------------------------------------------------------------------------------
// the sort of the permutation
// ------------------------------------------------------------------------------------------------------------
#define WG_VIEW_NONE 0xffffffffu       // pads a short run: behind every record

template <bool LABELS = false>
__device__ __forceinline__ bool wg_view_less_pad(const wg_view_rec* recs, uint32_t x, uint32_t y, const char* arena)
{
    if (x == WG_VIEW_NONE) return false;
    if (y == WG_VIEW_NONE) return true;
    return wg_view_less<LABELS>(recs, x, y, arena);
}

// *unsorted = 1 when some record sorts before the record in front of it
template <bool LABELS>
__device__ __forceinline__ void wg_view_inorder(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, int64_t n, uint32_t* unsorted)
{
    const int64_t i = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (i + 1 < n && wg_view_cmp_as<LABELS>(recs[i + 1], recs[i], arena) < 0) *unsorted = 1u;
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_inorder(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, int64_t n, uint32_t* unsorted)
{
    wg_view_inorder<false>(recs, arena, n, unsorted);
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_inorder_labelled(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, int64_t n, uint32_t* unsorted)
{
    wg_view_inorder<true>(recs, arena, n, unsorted);
}

template <bool LABELS>
__device__ __forceinline__ void wg_view_sort_runs(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, int64_t n, uint32_t* __restrict__ perm)
{
    __shared__ uint32_t idx[WG_VIEW_RUN];
    const uint32_t t = threadIdx.x;
    const int64_t first = (int64_t)blockIdx.x * WG_VIEW_RUN;
    for (uint32_t i = t; i < WG_VIEW_RUN; i += WG_BLOCK) idx[i] = first + i < n ? (uint32_t)(first + i) : WG_VIEW_NONE;
    __syncthreads();
    for (uint32_t k = 2; k <= WG_VIEW_RUN; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;      // the pair (i, i + j) of this thread
            const uint32_t x = idx[i], y = idx[l];
            const bool up = (i & k) == 0;
            if (up ? wg_view_less_pad<LABELS>(recs, y, x, arena) : wg_view_less_pad<LABELS>(recs, x, y, arena)) { idx[i] = y; idx[l] = x; }
            __syncthreads();
        }
    for (uint32_t i = t; i < WG_VIEW_RUN; i += WG_BLOCK)
        if (first + i < n) perm[first + i] = idx[i];
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_sort_runs(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, int64_t n, uint32_t* __restrict__ perm)
{
    wg_view_sort_runs<false>(recs, arena, n, perm);
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_sort_runs_labelled(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, int64_t n, uint32_t* __restrict__ perm)
{
    wg_view_sort_runs<true>(recs, arena, n, perm);
}

// src holds sorted runs of `run` indices (the last one shorter); dst receives runs of 2 * run
template <bool LABELS>
__device__ __forceinline__ void wg_view_merge(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, int64_t n, int64_t run,
                                              const uint32_t* __restrict__ src, uint32_t* __restrict__ dst)
{
    const int64_t o0 = ((int64_t)blockIdx.x * WG_BLOCK + threadIdx.x) * WG_VIEW_MERGE_ITEMS;
    if (o0 >= n) return;
    const int64_t base = o0 / (2 * run) * (2 * run);                 // (2 * run is a multiple of the items: they lie in one pair of runs)
    const int64_t mid = base + run < n ? base + run : n, end = base + 2 * run < n ? base + 2 * run : n;
    const uint32_t *A = src + base, *B = src + mid;
    const int64_t la = mid - base, lb = end - mid, diag = o0 - base;
    int64_t lo = diag > lb ? diag - lb : 0, hi = diag < la ? diag : la;
    while (lo < hi) {                                                // how many of the `diag` elements in front come from A
        const int64_t m = (lo + hi) >> 1;
        if (!wg_view_less<LABELS>(recs, B[diag - 1 - m], A[m], arena)) lo = m + 1; else hi = m;
    }
    int64_t ai = lo, bi = diag - lo;
    const int64_t todo = la + lb - diag < WG_VIEW_MERGE_ITEMS ? la + lb - diag : WG_VIEW_MERGE_ITEMS;
    for (int64_t k = 0; k < todo; k++) {
        const bool take_a = bi >= lb || (ai < la && !wg_view_less<LABELS>(recs, B[bi], A[ai], arena));
        dst[o0 + k] = take_a ? A[ai++] : B[bi++];
    }
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_merge(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, int64_t n, int64_t run,
                                                         const uint32_t* __restrict__ src, uint32_t* __restrict__ dst)
{
    wg_view_merge<false>(recs, arena, n, run, src, dst);
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_merge_labelled(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, int64_t n, int64_t run,
                                                                  const uint32_t* __restrict__ src, uint32_t* __restrict__ dst)
{
    wg_view_merge<true>(recs, arena, n, run, src, dst);
}

// ------------------------------------------------------------------------------------------------------------
// collapse and emit.  perm == nullptr: the records in input order.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t wg_view_at(const uint32_t* perm, int64_t i) { return perm ? perm[i] : (uint32_t)i; }

template <bool LABELS>
__device__ __forceinline__ void wg_view_heads(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, const uint32_t* __restrict__ perm,
                                              int64_t n, uint8_t* __restrict__ head, uint64_t* __restrict__ wg_counts, uint64_t* __restrict__ wg_heads)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    uint64_t c = 0, h = 0;
    if (i < n) {
        const wg_view_rec& r = recs[wg_view_at(perm, i)];
        c = (uint64_t)(int64_t)r.count;                             // (a negative count subtracts: two's complement)
        h = i == 0 || wg_view_run_head<LABELS>(recs[wg_view_at(perm, i - 1)], r, arena) ? 1u : 0u;
        head[i] = (uint8_t)h;
    }
    uint64_t cs, hs;
    (void)wg_view_block_incl_u64(c, sh, cs);
    (void)wg_view_block_incl_u64(h, sh, hs);
    if (threadIdx.x == 0) { wg_counts[blockIdx.x] = cs; wg_heads[blockIdx.x] = hs; }
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_heads(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, const uint32_t* __restrict__ perm,
                                                         int64_t n, uint8_t* __restrict__ head, uint64_t* __restrict__ wg_counts, uint64_t* __restrict__ wg_heads)
{
    wg_view_heads<false>(recs, arena, perm, n, head, wg_counts, wg_heads);
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_heads_labelled(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, const uint32_t* __restrict__ perm,
                                                                  int64_t n, uint8_t* __restrict__ head, uint64_t* __restrict__ wg_counts, uint64_t* __restrict__ wg_heads)
{
    wg_view_heads<true>(recs, arena, perm, n, head, wg_counts, wg_heads);
}

// run_end[r] = the sum of the counts up to and including run r's last line, run_tail[r] = that line's position
__global__ __launch_bounds__(WG_BLOCK) void k_view_tails(const wg_view_rec* __restrict__ recs, const uint32_t* __restrict__ perm, int64_t n,
                                                         const uint8_t* __restrict__ head, const uint64_t* __restrict__ count_base, const uint64_t* __restrict__ head_base,
                                                         int64_t* __restrict__ run_end, uint32_t* __restrict__ run_tail)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t i = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    uint64_t c = 0, h = 0;
    if (i < n) { c = (uint64_t)(int64_t)recs[wg_view_at(perm, i)].count; h = head[i]; }
    uint64_t all;
    const uint64_t cs = count_base[blockIdx.x] + wg_view_block_incl_u64(c, sh, all);
    const uint64_t hs = head_base[blockIdx.x] + wg_view_block_incl_u64(h, sh, all);
    if (i < n && (i == n - 1 || head[i + 1])) { run_end[hs - 1] = (int64_t)cs; run_tail[hs - 1] = (uint32_t)i; }
}

// n_runs: the total of the heads (k_bed_scan's totals[0]).  The grid covers n lines, which is no fewer.
__global__ __launch_bounds__(WG_BLOCK) void k_view_runs(const wg_view_rec* __restrict__ recs, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ n_runs,
                                                        const int64_t* __restrict__ run_end, const uint32_t* __restrict__ run_tail, int64_t* __restrict__ run_sum,
                                                        uint64_t* __restrict__ wg_bytes, uint64_t* __restrict__ wg_lines, uint32_t* too_big)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t r = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    uint64_t len = 0;
    if (r < (int64_t)*n_runs) {
        const int64_t sum = run_end[r] - (r ? run_end[r - 1] : 0);
        run_sum[r] = sum;
        if (sum >= WG_VIEW_MAX_SUM) *too_big = 1u;
        len = wg_view_line_len(recs[wg_view_at(perm, run_tail[r])], sum);
    }
    uint64_t bs, ls;
    (void)wg_view_block_incl_u64(len, sh, bs);
    (void)wg_view_block_incl_u64(len ? 1u : 0u, sh, ls);
    if (threadIdx.x == 0) { wg_bytes[blockIdx.x] = bs; wg_lines[blockIdx.x] = ls; }
}

// the line of a run without its end: "chrom \t rs' \t pattern \t sum" at dst -> the byte behind it
__device__ __forceinline__ char* wg_view_put_line(const wg_view_rec& rec, const char* __restrict__ arena, int64_t sum, char* dst)
{
    const char* src = arena + rec.off;
    for (uint32_t j = 0; j < rec.clen; j++) dst[j] = src[j];
    dst += rec.clen;
    *dst++ = '\t';
    dst += wg_view_int_put(dst, rec.rs);
    *dst++ = '\t';
    src += rec.clen;
    for (uint32_t j = 0; j < rec.plen; j++) dst[j] = src[j];
    dst += rec.plen;
    *dst++ = '\t';
    return dst + wg_dec_put(dst, (uint64_t)sum);
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_emit(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, const uint32_t* __restrict__ perm,
                                                        const uint64_t* __restrict__ n_runs, const int64_t* __restrict__ run_sum, const uint32_t* __restrict__ run_tail,
                                                        const uint64_t* __restrict__ wg_base, char* __restrict__ out)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t r = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    uint64_t len = 0;
    int64_t sum = 0;
    uint32_t at = 0;
    if (r < (int64_t)*n_runs) {
        sum = run_sum[r];
        at = wg_view_at(perm, run_tail[r]);
        len = wg_view_line_len(recs[at], sum);
    }
    uint64_t all;
    const uint64_t incl = wg_view_block_incl_u64(len, sh, all);
    if (!len) return;
    const wg_view_rec rec = recs[at];
    const char* src = arena + rec.off;
    char* dst = out + wg_base[blockIdx.x] + incl - len;
    for (uint32_t j = 0; j < rec.clen; j++) dst[j] = src[j];
    dst += rec.clen;
    *dst++ = '\t';
    dst += wg_view_int_put(dst, rec.rs);
    *dst++ = '\t';
    src += rec.clen;
    for (uint32_t j = 0; j < rec.plen; j++) dst[j] = src[j];
    dst += rec.plen;
    *dst++ = '\t';
    dst += wg_dec_put(dst, (uint64_t)sum);
    *dst = '\n';
}

// ------------------------------------------------------------------------------------------------------------
// With labels (`wgbstools mix_pat`, wgbsseg_patview_set_labels): k_view_inorder_labelled, k_view_sort_runs_labelled, k_view_merge_labelled and
// k_view_heads_labelled — the bodies above with the label rank as the last key (template <bool LABELS>; the kernels without labels are the
// instantiations they were) — have made a run the lines of ONE label; k_view_tails has left run_end / run_tail.  Then, in place of
// k_view_runs and k_view_emit:
//   k_view_run_sums      a run's sum, the 10^15 flag
//   k_view_tie_order     the runs equal in (start, pattern, chromosome) — neighbours, at most one per label — into the order of the
//                        reference's `sort -m`: the decimal text of the sum, then the label (view_core.h wg_view_tie_less).  Every run finds
//                        its group by walking over its neighbours and its place by counting the runs of the group before it, and writes
//                        its sum and tail there: no atomics, and before the byte scan, so the emit pass writes the runs in that order
//   k_view_runs_labelled the length of every run's line with its label, per-workgroup sums
//   k_view_emit_labelled after the scan: "chrom \t rs' \t pattern \t sum \t label \n"
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG_BLOCK) void k_view_run_sums(const uint64_t* __restrict__ n_runs, const int64_t* __restrict__ run_end, int64_t* __restrict__ run_sum,
                                                            uint32_t* too_big)
{
    const int64_t r = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (r >= (int64_t)*n_runs) return;
    const int64_t sum = run_end[r] - (r ? run_end[r - 1] : 0);
    run_sum[r] = sum;
    if (sum >= WG_VIEW_MAX_SUM) *too_big = 1u;
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_tie_order(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, const uint32_t* __restrict__ perm,
                                                             const uint64_t* __restrict__ n_runs, const int64_t* __restrict__ run_sum, const uint32_t* __restrict__ run_tail,
                                                             int64_t* __restrict__ tie_sum, uint32_t* __restrict__ tie_tail)
{
    const int64_t r = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x, nr = (int64_t)*n_runs;
    if (r >= nr) return;
    const wg_view_rec& mine = recs[wg_view_at(perm, run_tail[r])];
    const int64_t sum = run_sum[r];
    int64_t g0 = r, g1 = r + 1, before = 0;                          // the group [g0, g1) of r; the label ranks of a group ascend and differ
    while (g0 > 0 && wg_view_cmp(recs[wg_view_at(perm, run_tail[g0 - 1])], mine, arena) == 0) g0--;
    while (g1 < nr && wg_view_cmp(recs[wg_view_at(perm, run_tail[g1])], mine, arena) == 0) g1++;
    for (int64_t j = g0; j < g1; j++)
        if (j != r && wg_view_tie_less(run_sum[j], recs[wg_view_at(perm, run_tail[j])].line, sum, mine.line)) before++;
    tie_sum[g0 + before] = sum;
    tie_tail[g0 + before] = run_tail[r];
}

__device__ __forceinline__ uint32_t wg_view_label_len(const wg_view_labels& lab, uint32_t rank) { return lab.off[rank + 1] - lab.off[rank]; }

__global__ __launch_bounds__(WG_BLOCK) void k_view_runs_labelled(const wg_view_rec* __restrict__ recs, const uint32_t* __restrict__ perm, const uint64_t* __restrict__ n_runs,
                                                                 const int64_t* __restrict__ tie_sum, const uint32_t* __restrict__ tie_tail, wg_view_labels lab,
                                                                 uint64_t* __restrict__ wg_bytes, uint64_t* __restrict__ wg_lines)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t r = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    uint64_t len = 0;
    if (r < (int64_t)*n_runs) {
        const wg_view_rec& rec = recs[wg_view_at(perm, tie_tail[r])];
        len = wg_view_line_len_labelled(rec, tie_sum[r], wg_view_label_len(lab, rec.line));
    }
    uint64_t bs, ls;
    (void)wg_view_block_incl_u64(len, sh, bs);
    (void)wg_view_block_incl_u64(len ? 1u : 0u, sh, ls);
    if (threadIdx.x == 0) { wg_bytes[blockIdx.x] = bs; wg_lines[blockIdx.x] = ls; }
}

__global__ __launch_bounds__(WG_BLOCK) void k_view_emit_labelled(const wg_view_rec* __restrict__ recs, const char* __restrict__ arena, const uint32_t* __restrict__ perm,
                                                                 const uint64_t* __restrict__ n_runs, const int64_t* __restrict__ tie_sum, const uint32_t* __restrict__ tie_tail,
                                                                 wg_view_labels lab, const uint64_t* __restrict__ wg_base, char* __restrict__ out)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t r = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    uint64_t len = 0;
    int64_t sum = 0;
    uint32_t at = 0, rank = 0;
    if (r < (int64_t)*n_runs) {
        sum = tie_sum[r];
        at = wg_view_at(perm, tie_tail[r]);
        rank = recs[at].line;
        len = wg_view_line_len_labelled(recs[at], sum, wg_view_label_len(lab, rank));
    }
    uint64_t all;
    const uint64_t incl = wg_view_block_incl_u64(len, sh, all);
    if (!len) return;
    char* dst = wg_view_put_line(recs[at], arena, sum, out + wg_base[blockIdx.x] + incl - len);
    *dst++ = '\t';
    const char* name = lab.bytes + lab.off[rank];
    const uint32_t nl = wg_view_label_len(lab, rank);
    for (uint32_t j = 0; j < nl; j++) dst[j] = name[j];
    dst[nl] = '\n';
}
