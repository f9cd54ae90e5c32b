// block_plan.h — the host plan of the block reduction (wgbsseg_block_sums) and what host and device must agree on: the tile
// constants and the two rules of the streaming kernel's tile table.  No HIP here (like env.h and stitch.h): g++ compiles it
// alone, tests/native/blockplan_host.cpp hands it to the tests.
//
// A call's tables go up in ONE buffer of int32 — BlockSumPlan::upload — laid out as
//     x0 [n_blocks] | x1 [n_blocks] | perm [n_blocks, unsorted tables only] | tile_first [n_tiles + 1] | direct [n_direct]
// BlockSumPlan::view() is the only statement of that layout: the host fills the tables through it, the launches find them
// on the device through it.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/wgbsseg.h"
#include "exact_log2.h"      // WG_HD: __host__ __device__ under hipcc, plain inline for g++

#define WG_BS_TILE 896         // general kernel (k_block_sums): tile stride; WG_BS_EXT = 1024 sites are staged per tile (one wavefront pass of 16 sites per lane for uint8 rows)
#define WG_BS_RUN 8            // ... consecutive tiles streamed by one workgroup
#define WG_BSR_SPL 16                          // streaming kernel (k_block_sums_run): sites per lane of a tile: two 16-byte vectors.  (8 = 512-site tiles, runs of 16: 68 VGPRs and 20 KB of
                                               // LDS per workgroup, i.e. 28 instead of 16 resident wavefronts per CU — measured 0.467 vs 0.434-0.455 ms: the
                                               // pass is instruction-bound, and the per-tile work is spread over half the sites)
#define WG_BSR_TILE (64 * WG_BSR_SPL)
#define WG_BSR_RUN 8

// Rule 1: the streaming tile a block [x0, x1) is resolved in: the one holding its last site (an empty block: its position).
WG_HD int64_t wg_bsr_tile_of(int32_t x0, int32_t x1) { return (int64_t)(x1 - 1 > x0 ? x1 - 1 : x0) / WG_BSR_TILE; }

// Rule 2: can the two-tile prefix ring of tile t serve the block?  Not when it begins before t's run, or more than a tile before
// t: k_block_sums_direct takes those.  An empty block reads one ring entry twice: always served.
WG_HD bool wg_bsr_ring_reaches(int32_t x0, int32_t x1, int64_t t)
{
    const int64_t lo = t * WG_BSR_TILE;
    return x1 <= x0 || (t % WG_BSR_RUN == 0 ? x0 >= lo : x0 >= lo - (WG_BSR_TILE - 1));
}

struct BlockSumPlan {
    int64_t n_blocks = 0;
    bool sorted = true;        // the table came ordered by first site: no permutation
    bool monotone = false;     // ordered by last site too, uint8 rows: the streaming kernel (prep, run, direct); else the general one
    int64_t n_tiles = 0;       // tiles of the kernel that runs: of WG_BSR_TILE sites when monotone, else of WG_BS_TILE
    int64_t n_direct = 0;      // blocks the ring cannot serve (monotone only)
    std::vector<int32_t> upload;

    template <class T> struct View {
        T* x0; T* x1;          // the blocks in order of their first site
        T* perm;               // the caller's row of sorted block i; nullptr when the table came sorted
        T* tile_first;         // general: first block that starts at or behind each tile's first site; streaming: first block resolved in the tile or behind
        T* direct;             // sorted indices of the blocks for k_block_sums_direct
    };
    template <class T> View<T> view(T* base) const
    {
        T* const tf = base + row_words();
        return {base, base + n_blocks, sorted ? nullptr : base + 2 * n_blocks, tf, tf + n_tiles + 1};
    }
    size_t row_words() const { return (size_t)((sorted ? 2 : 3) * n_blocks); }
    size_t upload_words() const { return row_words() + (size_t)(n_tiles + 1 + n_direct); }
};

inline int wg_plan_refuse(std::string& msg, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return WGBSSEG_E_ARG;
}

// Checks the table against rows of n_total sites (`elem` bytes per count) and plans its reduction.  n_blocks == 0: an empty plan.
inline int plan_block_sums(const int64_t* start0, const int64_t* end0, int64_t n_blocks, int64_t n_total, int elem, int mode, bool force_general,
                           BlockSumPlan& p, std::string& msg)
{
    p = BlockSumPlan();
    if (n_blocks < 0 || mode < 0 || mode > 3 || (n_blocks && (!start0 || !end0))) return wg_plan_refuse(msg, "bad arguments to block_sums");
    if (n_blocks == 0) return WGBSSEG_OK;
    if (n_blocks > 0x7fffffff || n_total > 0x7fffffff) return wg_plan_refuse(msg, "too many blocks / sites for one block_sums call");
    for (int64_t i = 0; i < n_blocks; i++) {
        if (start0[i] < 0 || end0[i] < start0[i] || end0[i] > n_total)
            return wg_plan_refuse(msg, "block %lld = sites [%lld, %lld) is outside the %lld sites of the beta files or reversed",
                                  (long long)i, (long long)start0[i], (long long)end0[i], (long long)n_total);
        if (mode == 0 && elem == 2 && end0[i] - start0[i] > 65536)
            return wg_plan_refuse(msg, "block %lld: uint32 sums of uint16 counts are only exact up to 65536 sites per block", (long long)i);
        if (i && start0[i] < start0[i - 1]) p.sorted = false;
    }
    p.n_blocks = n_blocks;
    const int64_t n_gtiles = (n_total + WG_BS_TILE - 1) / WG_BS_TILE, n_rtiles = (n_total + WG_BSR_TILE - 1) / WG_BSR_TILE;
    p.upload.reserve(p.row_words() + (size_t)n_gtiles + 1);       // (room for the larger tile table: the second resize below copies nothing)
    p.upload.resize(p.row_words());
    // the kernels want the blocks in order of their first site (a table a segmentation wrote already is): sort a copy
    BlockSumPlan::View<int32_t> v = p.view(p.upload.data());
    if (p.sorted) {
        for (int64_t i = 0; i < n_blocks; i++) { v.x0[i] = (int32_t)start0[i]; v.x1[i] = (int32_t)end0[i]; }
    } else {
        // first site, then row in the file (both below 2^31) as one number: sorting those is the stable sort by first site, without its indirect compares
        std::vector<int64_t> key((size_t)n_blocks);
        for (int64_t i = 0; i < n_blocks; i++) key[(size_t)i] = (start0[i] << 32) | i;
        std::sort(key.begin(), key.end());
        for (int64_t i = 0; i < n_blocks; i++) {
            v.perm[i] = (int32_t)(key[(size_t)i] & 0x7fffffff); v.x0[i] = (int32_t)(key[(size_t)i] >> 32); v.x1[i] = (int32_t)end0[v.perm[i]];
        }
    }
    // uint8 rows and a table ordered by first AND last site (what a segmentation writes; beta_to_blocks' "nice" tables): the streaming kernel
    p.monotone = !force_general && elem == 1 && (uint64_t)n_blocks * 8 < (1ull << 32);      // (32-bit output offsets in the streaming kernel)
    for (int64_t i = 1; i < n_blocks && p.monotone; i++) p.monotone = v.x1[i] >= v.x1[i - 1];
    p.n_tiles = p.monotone ? n_rtiles : n_gtiles;
    p.upload.resize(p.upload_words());
    v = p.view(p.upload.data());
    int64_t b = 0;
    for (int64_t t = 0; t < p.n_tiles; t++) {
        // general: the first block that starts at or after the tile's first site (empty blocks ride along with their start site);
        // streaming: the first block resolved in the tile or behind it
        if (p.monotone) while (b < n_blocks && wg_bsr_tile_of(v.x0[b], v.x1[b]) < t) b++;
        else while (b < n_blocks && v.x0[b] < t * WG_BS_TILE) b++;
        v.tile_first[t] = (int32_t)b;
    }
    // Empty blocks at n_total belong to the last tile, whatever tile their position names (one behind the last when n_total is a multiple
    // of the tile): the table ends with n_blocks.  That is why no clamp stands here; k_block_sums_prep, which works per block, has one.
    v.tile_first[p.n_tiles] = (int32_t)n_blocks;
    if (p.monotone) {
        std::vector<int32_t> direct;
        for (int64_t i = 0; i < n_blocks; i++)
            if (!wg_bsr_ring_reaches(v.x0[i], v.x1[i], wg_bsr_tile_of(v.x0[i], v.x1[i]))) direct.push_back((int32_t)i);
        p.n_direct = (int64_t)direct.size();
        p.upload.insert(p.upload.end(), direct.begin(), direct.end());      // (v ends here: the buffer may move)
    }
    return WGBSSEG_OK;
}
