// frag_kernels.h — `wgbstools frag_len` on gfx950: the histogram of the reads' lengths in CpGs, weighted by the reads' counts, over
// every read of a pat file or over the reads a region / a block list lets through.  The pat text format comes from pat_kernels.h
// (PatTile, PatText, wg_pat_tile_lines, wg_pat_parse_line, wg_pat_site_before, wg_pat_is_last_read), the search from homog_kernels.h
// (wg_homog_upper), the constants from frag_plan.h.
//
// A selected line `chr, s, pattern, count` adds count to bin min(len(pattern), max_frag) (frag_len.py:27: the awk program at the
// end of the reference's pipe).  Which lines are selected is the rule of the reference's cview without --strict
// (src/cview/cview.cpp:87-128), which streams the reads past the blocks, the blocks ordered by `sort -k1,1n` of the text
// "startCpG\tendCpG" (startCpG ascending; endCpG need NOT ascend among equal starts, nor from one start to the next), with a cursor
// `cur` that only moves forward.  On reads sorted by start every one of its steps is a test on the read alone, which is why the reads
// can be taken in parallel (the argument of homog_kernels.h, for this walk):
//   - "the read starts at or after the endCpG of the block that sorts LAST: stop reading" — every later read starts there too, so
//     a read [s, s + len) is dropped exactly when s >= end_last, also where an earlier, longer block still holds it.
//   - "advance cur while s >= endCpG[cur]": the blocks passed end at or before this read's start or an earlier read's, which is no
//     larger, so every block before cur has endCpG <= s, and cur's own has endCpG > s: cur is the FIRST block whose endCpG exceeds
//     s, wherever the reads before left the cursor.  endCpG is not ascending, its running maximum pmax is, and the first block with
//     endCpG > s is the first with pmax > s: one binary search.  It exists, because s < end_last <= pmax of the last block.
//   - "the read ends before startCpG[cur]: skip it; else pass it on whole": selected iff s + len - 1 >= startCpG[cur].  (A later
//     block that starts inside the read does not bring it back: the reference looks at cur only.)
// With one block — a region or a site range — cur is that block and the two comparisons are made directly.  Without blocks every
// line is selected and the order of the reads does not matter: nothing below looks at it.
//
// Layout: a workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... of the chunk (staged and split into lines like
// k_pat_count: a 4 KB tile + 1 KB spill in LDS, one line per thread, long lines read on from global memory) and keeps ITS histogram in
// LDS across all of them, as 64-bit counters (three lines of count 2^31 - 1 overflow 32 bits); at the end it adds every non-zero bin
// to the global histogram with one 64-bit integer atomic.  The grid is capped (WG_FRAG_GROUPS), so the few hot global bins — reads
// are mostly a handful of CpGs long — see a few thousand atomics per launch, not one per tile.  Integer sums do not depend on the
// order of the additions: the result is bit-reproducible.  Bins from WG_FRAG_LDS_BINS on (max_frag above it) are added to in
// global memory directly: reads that long are rare.
//
// Refusals, as in the other pat engines: a malformed line -> `bad` (lowest byte offset; an EMPTY pattern is malformed here: the
// reference's awk would take the count for the pattern); with blocks, a read starting before the read before it -> `desc` (lowest
// byte offset).  The read before a tile's first line and the chunk's last read: wg_pat_site_before / wg_pat_is_last_read.
#pragma once
#include "pat_kernels.h"
#include "homog_kernels.h"   // wg_homog_upper
#include "frag_plan.h"       // WG_FRAG_LDS_BINS

// (waves_per_eu(6): what the LDS admits — six workgroups of ~26 KB per CU, one wavefront of each per SIMD; left alone the allocation lands
// 1 VGPR above the 80 that six waves per SIMD allow.  The price: one 8-byte spill, reloaded once per tile by the lane that scans back.)
__global__ __launch_bounds__(WG_BLOCK) __attribute__((amdgpu_waves_per_eu(6))) void k_frag_hist(const char* __restrict__ text, int64_t n, int64_t tiles,
                                                        const int32_t* __restrict__ bstart, const int32_t* __restrict__ bpmax, int64_t nblk, int64_t end_last,
                                                        int max_frag, unsigned long long* __restrict__ hist, unsigned long long* bad, unsigned long long* desc,
                                                        const long long* prev_in, long long* prev_out, unsigned long long chunk_off)
{
    __shared__ PatTile tile;
    __shared__ unsigned long long s_hist[WG_FRAG_LDS_BINS];
    __shared__ long long s_last[WG_BLOCK / 64];              // the start of every wavefront's last line in the round (WG_PAT_NO_SITE: no line / malformed)
    __shared__ long long s_prev;                             // the start of the read before the round's first line; both with blocks only
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lds_bins = max_frag < WG_FRAG_LDS_BINS ? max_frag : WG_FRAG_LDS_BINS;
    const bool select = nblk > 0;                            // (uniform: a kernel argument)
    int32_t one_start = 0;
    if (nblk == 1) one_start = bstart[0];
    for (int b = tid; b < lds_bins; b += WG_BLOCK) s_hist[b] = 0;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t base = t * WG_PAT_TILE;
        if (select && tid == 0) s_prev = wg_pat_site_before(text, n, base, prev_in);
        const uint32_t total = wg_pat_tile_lines(text, n, base, tile);   // (synchronises: s_prev, the cleared s_hist visible)
        const PatText T = tile.text(text, base, n);
        for (uint32_t r0 = 0; r0 < total; r0 += WG_BLOCK) {
            const uint32_t l = r0 + (uint32_t)tid;
            int64_t site = 0, ps = 0, plen = 0, count = 0;
            bool ok = false;
            if (l < total) {
                const int64_t p = base + tile.lstart[l];
                ok = wg_pat_parse_line(T, p, n, site, ps, plen, count) && plen > 0;
                if (!ok) atomicMin(bad, chunk_off + (unsigned long long)p);
            }
            bool sel = ok;
            if (select) {
                const long long mine = ok ? (long long)site : WG_PAT_NO_SITE;
                long long pv = __shfl_up(mine, 1);                   // the line before: the lane below, ...
                if (lane == 63) s_last[wv] = mine;
                __syncthreads();
                if (lane == 0) pv = wv ? s_last[wv - 1] : s_prev;    // ... the wavefront below, or the round / tile / chunk before
                if (ok) {
                    if (pv != WG_PAT_NO_SITE && site < pv) atomicMin(desc, chunk_off + (unsigned long long)(base + tile.lstart[l]));   // (read again: not kept in registers)
                    if (l == total - 1 && wg_pat_is_last_read(T, ps, plen, n)) *prev_out = site;
                    sel = site < end_last;
                    if (sel) {
                        const int32_t cs = nblk == 1 ? one_start : bstart[wg_homog_upper(bpmax, 0, nblk, site)];
                        sel = site + plen - 1 >= (int64_t)cs;
                    }
                }
            }
            if (sel) {
                const int64_t b = (plen < max_frag ? plen : (int64_t)max_frag) - 1;
                const unsigned long long c = (unsigned long long)(long long)count;     // (a negative count subtracts: two's complement)
                if (b < WG_FRAG_LDS_BINS) atomicAdd(&s_hist[b], c);
                else atomicAdd(&hist[b], c);
            }
            if (select) {
                __syncthreads();
                if (tid == 0) s_prev = s_last[WG_BLOCK / 64 - 1];    // the next round's first line follows this round's last
                __syncthreads();                                     // (s_last: rewritten by the next round)
            }
        }
        __syncthreads();                                             // (the tile: restaged by the next one)
    }
    __syncthreads();
    for (int b = tid; b < lds_bins; b += WG_BLOCK)
        if (s_hist[b] != 0) atomicAdd(&hist[b], s_hist[b]);
}
