// bed2beta_kernels.h — `wgbstools bed2beta` on gfx950: BED methylation calls `chr \t start \t end \t #meth \t #total` joined to the
// genome's CpG dictionary, the first of duplicated lines kept, in one pass over the text (the reference: bed2beta.py:11-51, a pandas
// drop_duplicates and a left merge of the whole dictionary frame).  The rules of a line are bed2beta_core.h's, shared with the host; the
// staging of a tile of text and its line finding are pat_kernels.h's (PatTile, PatText, wg_pat_tile_lines).
//
// k_bedbeta_scan, per fed chunk.  Layout as k_pat_count: one workgroup per 4 KB tile (+ 1 KB spill) in LDS, one line per thread, rounds of
// WG_BLOCK for a tile of more lines, a line that runs past the staged bytes read on from global memory.  A line is walked
// (wg_bb_walk), its chromosome found among the names in byte order (wg_bb_find_chrom: the rank the thread found last is tried first),
// its position searched among that chromosome's loci (wg_bb_find_locus: a lower bound, a hit on equality), its pair trimmed as the
// .beta file stores it, and ONE 64-bit atomicMin puts (byte offset of the line in its file << 16 | m8 << 8 | c8) into the table's word
// of the site.  The table starts as all ones; the minimum over a site's lines is the first of them in the file and carries that line's
// pair, so nothing is parsed twice and the result does not depend on the order of the work, of the tiles or of the chunks.
// Reports: the lowest refused line as (offset << 8 | reason) by atomicMin; the four counters — lines read, matched, on an unknown
// chromosome, at no CpG — summed per workgroup, then one atomicAdd each.  Plain C++ only.
//
// k_bedbeta_unpack, at finish.  One thread per 8 sites: eight words in (four 16-byte loads), one 16-byte store out, 0, 0 for the empty
// marker; the sites set are counted per workgroup, then one atomicAdd (duplicates = matched - sites set).  The table and the result are
// padded to whole threads (BedBetaPlan::n_words): the words behind n_sites stay empty.
#pragma once
#include "pat_kernels.h"
#include "bed2beta_core.h"

// the scan's report on the device: 8-byte words
#define WG_BB_REP_BAD 0                // (offset << 8 | reason) of the lowest refused line; ~0: none
#define WG_BB_REP_LINES 1              // lines read (the header and empty lines are none)
#define WG_BB_REP_MATCHED 2
#define WG_BB_REP_NO_CHROM 3
#define WG_BB_REP_NO_CPG 4
#define WG_BB_REP_SET 5                // k_bedbeta_unpack: sites with a line
#define WG_BB_REP_WORDS 6

// the workgroup's sum of v[0 .. 3] -> one atomicAdd each into dst[0 .. 3] (every thread calls it)
__device__ __forceinline__ void wg_bb_block_add4(const uint32_t (&v)[4], uint32_t (&s_part)[WG_BLOCK / 64][4], unsigned long long* dst)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t w = wg_wave_sum_u32(v[k]);
        if (lane == 0) s_part[wv][k] = w;
    }
    __syncthreads();
    if (tid < 4) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < WG_BLOCK / 64; w++) sum += s_part[w][tid];
        if (sum) atomicAdd(&dst[tid], (unsigned long long)sum);
    }
}

__global__ __launch_bounds__(WG_BLOCK) void k_bedbeta_scan(const char* __restrict__ text, int64_t n, wg_bb_chroms chroms, const uint32_t* __restrict__ loci,
                                                           int add_one, int drop_header, unsigned long long* __restrict__ table,
                                                           unsigned long long* report, unsigned long long chunk_off)
{
    __shared__ PatTile tile;
    __shared__ uint32_t s_part[WG_BLOCK / 64][4];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * WG_PAT_TILE;
    const uint32_t total = wg_pat_tile_lines(text, n, base, tile);
    const PatText T = tile.text(text, base, n);
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};                             // lines, matched, unknown chromosome, no CpG
    int32_t hint = -1;
    for (uint32_t l = (uint32_t)tid; l < total; l += WG_BLOCK) {
        const int64_t p = base + tile.lstart[l];
        const unsigned long long off = chunk_off + (unsigned long long)p;
        if (drop_header && off == 0) continue;                      // the file's first line, which Python found to be a header
        cnt[0]++;
        int64_t site = -1;
        uint64_t word = 0;
        const int what = wg_bb_line_to_site(T, p, n, off, chroms, loci, add_one, hint, site, word);
        if (what < 0) { atomicMin(&report[WG_BB_REP_BAD], (off << 8) | (unsigned long long)(-what)); continue; }
        if (what == WG_BB_MATCHED) atomicMin(&table[site], (unsigned long long)word);
        cnt[1 + what]++;
    }
    wg_bb_block_add4(cnt, s_part, report + WG_BB_REP_LINES);
}

__global__ __launch_bounds__(WG_BLOCK) void k_bedbeta_unpack(const unsigned long long* __restrict__ table, int64_t n_threads, uint8_t* __restrict__ out,
                                                             unsigned long long* report)
{
    __shared__ uint32_t s_part[WG_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t u = (int64_t)blockIdx.x * WG_BLOCK + tid;
    uint32_t set = 0;
    if (u < n_threads) {
        const ulonglong2* src = reinterpret_cast<const ulonglong2*>(table + u * 8);
        ulonglong2 v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = src[k];
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            w[k] = wg_bb_pair(v[k].x) | wg_bb_pair(v[k].y) << 16;
            set += (v[k].x != WG_BB_EMPTY ? 1u : 0u) + (v[k].y != WG_BB_EMPTY ? 1u : 0u);
        }
        *reinterpret_cast<uint4*>(out + u * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    const uint32_t ws = wg_wave_sum_u32(set);
    if (lane == 0) s_part[wv] = ws;
    __syncthreads();
    if (tid == 0) {
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < WG_BLOCK / 64; w++) sum += s_part[w];
        if (sum) atomicAdd(&report[WG_BB_REP_SET], (unsigned long long)sum);
    }
}
