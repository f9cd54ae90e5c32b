// homog_kernels.h — `wgbstools homog` on gfx950: per block, the reads that are mostly unmethylated (U), mixed (X) or mostly
// methylated (M).  The pat text format comes from pat_kernels.h (WG_PAT_TILE, PatTile, PatText, wg_pat_tile_lines, wg_pat_parse_line;
// WG_BLOCK through its seg_kernels.h).
//
// The reference (src/homog/homog.cpp:154-260) streams the sorted blocks beside the sorted reads and keeps a deque of the
// blocks a read may still reach.  On reads sorted by start and blocks sorted by (startCpG, endCpG) every one of its stop
// conditions is a test on the read alone, which is why the reads can be counted in parallel:
//   - "the read starts at or after the endCpG of the last loaded block once the blocks file is exhausted: stop" — when
//     s >= last.endCpG the last block has start < s <= read_end, so loading up to read_end has exhausted the file by then:
//     the condition is s >= endCpG of the LAST block in sorted order (blocks nested in a longer earlier block included), and
//     every later read starts there too.  So: a read counts only when s < last.endCpG.
//   - "advance the current block while s >= its endCpG": the blocks skipped end at or before an earlier (hence this) read's
//     start and cannot overlap it; "no current block left, file exhausted: stop" implies s >= every endCpG, the rule above;
//     "read_end < startCpG of the current block: skip" — later blocks start later still.  Every block with
//     startCpG <= read_end has been loaded (load_blocks_until(read_end)).
// So a read [s, s + len) counts into every block [startCpG, endCpG) it overlaps, and into nothing else, as long as
// s < last.endCpG.  Per (read, block) (update_block / update_m2): the pattern clipped to the overlap (--inclusive: the whole
// pattern) must be at least min_cpgs long, hold at least min_cpgs C / H / T, and meth = (float)nrC / (float)(nrC + nrT) —
// IEEE float32 division (no reciprocal, no fast math) — picks bin b with range[b] <= meth < range[b + 1] (meth == 1: the last
// bin), which gains `count` (int32, wrapping like the reference's counters).
//
// Layout: the pat text is staged and split into lines like k_pat_count (a 4 KB tile + 1 KB spill in LDS, one line per thread,
// long lines read on from global memory).  The lines of a tile are taken in rounds of WG_BLOCK; per round the blocks any of
// its lines can reach form one window [lo, hi): lo = the first block whose prefix maximum of endCpG exceeds the round's lowest
// start (a monotone bound even when blocks nest), hi = the first block starting at or after the round's highest read end.
// When the window fits (WG_HOMOG_WIN blocks, WG_HOMOG_CELLS counters) its blocks are staged in LDS, every line searches only
// the window and adds into LDS counters, and the round flushes one global atomic per touched (block, bin) cell; reads are
// sorted, so neighbouring lanes mostly hit the same block.  Otherwise (a block that spans most of a chromosome keeps lo
// low) lines search the whole block list and add with global atomics; such a table is slow (a line then walks every block
// from the long one on up to its own end) but counted correctly.
//
// Refusals (the reference silently produces partial or order-dependent output): a malformed line -> `bad` (lowest byte
// offset); a read starting before the read before it -> `desc` (lowest byte offset).  The read before a tile's first line
// is found by scanning back from the tile; before a chunk's first line it is the last read of the previous chunk, kept in
// device memory (prev_in / prev_out: two slots alternating per chunk).
#pragma once
#include "pat_kernels.h"
#include "homog_plan.h"      // WG_HOMOG_MAX_BINS, WG_HOMOG_NO_SITE

#define WG_HOMOG_WIN 512
#define WG_HOMOG_CELLS 2048

// the bin of (nrC, nrT) (update_m2, homog.cpp:154-183); -1 when meth < range[0]
__device__ __forceinline__ int wg_homog_bin(int nrc, int nrt, const float* range, int nb)
{
    const float meth = (float)nrc / (float)(nrc + nrt);
    if (meth < range[0]) return -1;
    int b = 0;
    for (; b < nb; b++)
        if (meth >= range[b] && meth < range[b + 1]) break;
    return b == nb ? nb - 1 : b;
}

// first index j in [lo, hi) with a[j] > v (a ascending); hi when none
__device__ __forceinline__ int64_t wg_homog_upper(const int32_t* a, int64_t lo, int64_t hi, int64_t v)
{
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if ((int64_t)a[m] > v) hi = m; else lo = m + 1;
    }
    return lo;
}

// (waves_per_eu(6): the kernel's occupancy.  With the tile in one PatTile object the LDS layout puts s_lo / s_hi side by side, the
// compiler merges their accesses, and the allocation lands 2 VGPRs above the 80 that 6 waves per SIMD allow.)
__global__ __launch_bounds__(WG_BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void k_homog_count(const char* __restrict__ text, int64_t n,
                                                          const int32_t* __restrict__ bstart, const int32_t* __restrict__ bend,
                                                          const int32_t* __restrict__ bpmax, int64_t nblk, int64_t last_end,
                                                          const float* __restrict__ range, int nb, int min_cpgs, int inclusive,
                                                          int32_t* __restrict__ counts, unsigned long long* bad, unsigned long long* desc,
                                                          const long long* prev_in, long long* prev_out, unsigned long long chunk_off)
{
    __shared__ PatTile tile;
    __shared__ long long s_site[WG_BLOCK];                   // the round's starts (WG_HOMOG_NO_SITE: no line / malformed)
    __shared__ int32_t w_start[WG_HOMOG_WIN], w_end[WG_HOMOG_WIN], w_pmax[WG_HOMOG_WIN];
    __shared__ int32_t w_cnt[WG_HOMOG_CELLS];
    __shared__ float s_range[WG_HOMOG_MAX_BINS + 1];
    __shared__ long long s_prev, s_lo_site, s_hi_end;
    __shared__ int64_t s_lo, s_hi;
    __shared__ int s_win;
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * WG_PAT_TILE;
    if (tid <= nb) s_range[tid] = range[tid];
    if (tid == 0) {
        // the read before the tile's first line: scan back over empty lines to the line that holds byte base - 1
        long long pv = WG_HOMOG_NO_SITE;
        int64_t i = base - 1;
        while (i >= 0 && text[i] == '\n') i--;
        if (i < 0) pv = *prev_in;
        else {
            while (i > 0 && text[i - 1] != '\n') i--;
            const PatText G = {tile.tx, text, INT64_MIN / 4, n};       // (base far below: every byte from global memory)
            int64_t site = 0, ps = 0, plen = 0, count = 0;
            if (wg_pat_parse_line(G, i, n, site, ps, plen, count)) pv = site;
        }
        s_prev = pv;
    }
    const uint32_t total = wg_pat_tile_lines(text, n, base, tile);   // (synchronises: s_prev, s_range visible)
    const PatText T = tile.text(text, base, n);
    for (uint32_t r0 = 0; r0 < total; r0 += WG_BLOCK) {
        const uint32_t l = r0 + (uint32_t)tid;
        int64_t p = 0, site = 0, ps = 0, plen = 0, count = 0;
        bool ok = false;
        if (l < total) {
            p = base + tile.lstart[l];
            ok = wg_pat_parse_line(T, p, n, site, ps, plen, count);
            if (!ok) atomicMin(bad, chunk_off + (unsigned long long)p);
        }
        s_site[tid] = ok ? (long long)site : WG_HOMOG_NO_SITE;
        if (tid == 0) { s_lo_site = INT64_MAX; s_hi_end = INT64_MIN; }
        __syncthreads();
        if (ok) {
            const long long pv = tid ? s_site[tid - 1] : s_prev;
            if (pv != WG_HOMOG_NO_SITE && site < pv) atomicMin(desc, chunk_off + (unsigned long long)p);
            if (l == total - 1) {                                // the chunk's last read?  (what the next chunk's first read is checked against)
                int64_t i = ps + plen;
                while (i < n && T.at(i) != '\n') i++;
                while (i < n && T.at(i) == '\n') i++;
                if (i == n) *prev_out = site;
            }
        }
        const bool act = ok && site < last_end && plen >= min_cpgs && plen > 0;
        if (act) { atomicMin(&s_lo_site, (long long)site); atomicMax(&s_hi_end, (long long)(site + plen)); }
        __syncthreads();
        if (tid == 0) {
            s_prev = s_site[WG_BLOCK - 1];                       // the next round's first line follows this round's last
            int64_t lo = 0, hi = 0;
            if (s_lo_site != INT64_MAX) {
                lo = wg_homog_upper(bpmax, 0, nblk, s_lo_site);              // blocks before lo end at or before every start of the round
                hi = wg_homog_upper(bstart, 0, nblk, s_hi_end - 1);          // blocks from hi start after every read end of the round
                if (hi < lo) hi = lo;
            }
            s_lo = lo; s_hi = hi;
            s_win = (hi - lo) <= WG_HOMOG_WIN && (hi - lo) * nb <= WG_HOMOG_CELLS;
        }
        __syncthreads();
        const int64_t lo = s_lo, hi = s_hi;
        const bool win = s_win != 0;
        if (win) {
            for (int64_t j = tid; j < hi - lo; j += WG_BLOCK) { w_start[j] = bstart[lo + j]; w_end[j] = bend[lo + j]; w_pmax[j] = bpmax[lo + j]; }
            for (int64_t c = tid; c < (hi - lo) * nb; c += WG_BLOCK) w_cnt[c] = 0;
            __syncthreads();
        }
        if (act && hi > lo) {
            const int32_t* qs = win ? w_start : bstart;
            const int32_t* qe = win ? w_end : bend;
            const int32_t* qp = win ? w_pmax : bpmax;
            const int64_t off = win ? lo : 0;                    // index in qs / qe / qp = block index - off
            const int64_t j0 = wg_homog_upper(qp, lo - off, hi - off, site);
            const int64_t j1 = wg_homog_upper(qs, j0, hi - off, site + plen - 1);
            int all_c = 0, all_t = 0;
            if (inclusive) {
                for (int64_t k = 0; k < plen; k++) { const char c = T.at(ps + k); all_c += (c == 'C' || c == 'H'); all_t += (c == 'T'); }
            }
            for (int64_t j = j0; j < j1; j++) {
                const int64_t bs = qs[j], be = qe[j];
                const int64_t os = site > bs ? site : bs, oe = (site + plen) < be ? (site + plen) : be;
                if (os >= oe) continue;                          // (nested blocks that end before the read)
                int nc = all_c, nt = all_t;
                if (!inclusive) {
                    if (oe - os < min_cpgs) continue;
                    nc = 0; nt = 0;
                    for (int64_t k = os - site; k < oe - site; k++) { const char c = T.at(ps + k); nc += (c == 'C' || c == 'H'); nt += (c == 'T'); }
                }
                if (nc + nt < min_cpgs) continue;
                const int b = wg_homog_bin(nc, nt, s_range, nb);
                if (b < 0) continue;
                if (win) atomicAdd(&w_cnt[j * nb + b], (int32_t)count);
                else atomicAdd(&counts[j * nb + b], (int32_t)count);
            }
        }
        if (win) {
            __syncthreads();
            for (int64_t c = tid; c < (hi - lo) * nb; c += WG_BLOCK)
                if (w_cnt[c] != 0) atomicAdd(&counts[lo * nb + c], w_cnt[c]);
        }
        __syncthreads();                                         // (s_site, the window: reused by the next round)
    }
}

// test hook: the bin of every (nrC, nrT) with nrC + nrT <= max_total, at index t (t + 1) / 2 + nrC for t = nrC + nrT
__global__ __launch_bounds__(WG_BLOCK) void k_homog_bins(const float* __restrict__ range, int nb, int max_total, int8_t* __restrict__ out)
{
    const int64_t idx = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    const int64_t n = (int64_t)(max_total + 1) * (max_total + 2) / 2;
    if (idx >= n) return;
    int64_t t = (int64_t)((sqrt(8.0 * (double)idx + 1.0) - 1.0) * 0.5);
    while (t * (t + 1) / 2 > idx) t--;
    while ((t + 1) * (t + 2) / 2 <= idx) t++;
    const int nrc = (int)(idx - t * (t + 1) / 2);
    out[idx] = (int8_t)wg_homog_bin(nrc, (int)t - nrc, range, nb);
}
