// stats_kernels.h — per-sample whole-file statistics of the resident rows (`wgbstools beta_cov` / `beta_stats`): one pass over
// the union of a list of site ranges, every result an integer ("Per-sample statistics").
//
// Work is cut in 16-byte vectors of a row, not in sites: range i = sites [x0, x1) touches the aligned vectors
// floor(x0 / S) .. ceil(x1 / S) - 1 (S = 8 sites of uint8 pairs, 4 of uint16 pairs), cumv[i] counts the vectors of the ranges
// before it, and unit u of the concatenation belongs to the last range with cumv[i] <= u.  Every load is an aligned 16-byte
// load inside the row's pitch; the sites of a vector that lie outside the range (a range may begin and end at any site, and
// two ranges may share a vector) are masked, which is what a scalar head and tail would do, without a second code path.
//
// The mean-methylation sum is exact: a term fl(fl(meth / cov) * 100.0) is an IEEE double computed with the plain `/` and `*`
// (no fast-math; -ffp-contract=off keeps them apart), then turned into a 128-bit integer in units of 2^-62 from its mantissa
// and exponent.  uint8 rows: a nonzero term lies in [100/255, 25500], uint16 rows: in [100/65535, 6553500] — its last
// mantissa bit is worth at least 2^-62 and the term is below 2^23, so the integer has at most 85 bits and 2^25 sites stay
// below 2^110.  Sums run in integers only (thread, wavefront, workgroup, then k_sample_stats_fold over the tiles' partial
// results): any launch geometry and any split of the ranges gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stats_plan.h"      // WG_ST_BLOCK, WG_ST_VPT, WG_ST_TILE
#include "wave_prims.h"

// what one workgroup leaves for the fold (and the fold's running sums)
struct wg_stat_part {
    uint64_t meth, cov, covered, covered_at, orphans, max_cov, ratio_lo, ratio_hi;
};

// the layout of wgbsseg_sample_stat (include/wgbsseg.h)
struct wg_sample_stat {
    uint64_t n_sites, meth_sum, cov_sum, covered, covered_at, orphans, ratio_lo, ratio_hi;
    uint32_t max_cov, reserved;
};

__device__ __forceinline__ void wg_st_add128(uint64_t& lo, uint64_t& hi, uint64_t alo, uint64_t ahi)
{
    lo += alo;
    hi += ahi + (lo < alo ? 1u : 0u);
}

// Sum of every thread's `p` over the workgroup, valid in thread 0.  The 128-bit sum travels as three 64-bit sums of its limbs
// (low and high half of ratio_lo, ratio_hi): no carries between lanes, 256 addends of 32 bits cannot overflow.
__device__ __forceinline__ wg_stat_part wg_st_block_sum(const wg_stat_part& p, uint64_t (*sh)[9])
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t v[9] = {p.meth, p.cov, p.covered, p.covered_at, p.orphans, 0, p.ratio_lo & 0xffffffffull, p.ratio_lo >> 32, p.ratio_hi};
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = wg_wave_sum_u64(v[k]);
    v[5] = wg_wave_max_u32((uint32_t)p.max_cov);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 9; k++) sh[wave][k] = v[k];
    }
    __syncthreads();
    wg_stat_part r = {};
    if (threadIdx.x == 0) {
        uint64_t s[9];
        for (int k = 0; k < 9; k++) {
            s[k] = sh[0][k];
            for (int w = 1; w < WG_ST_BLOCK / 64; w++) s[k] = k == 5 ? (sh[w][k] > s[k] ? sh[w][k] : s[k]) : s[k] + sh[w][k];
        }
        r.meth = s[0]; r.cov = s[1]; r.covered = s[2]; r.covered_at = s[3]; r.orphans = s[4]; r.max_cov = s[5];
        r.ratio_lo = s[6];
        r.ratio_hi = s[8] + (s[7] >> 32);
        wg_st_add128(r.ratio_lo, r.ratio_hi, s[7] << 32, 0);
    }
    return r;
}

// one site into a thread's sums; `in` = 0 for a site of the vector that lies outside the range
__device__ __forceinline__ void wg_st_site(uint32_t m, uint32_t c, bool in, int32_t depth_at, uint32_t& meth, uint32_t& cov, uint32_t& covered,
                                           uint32_t& covered_at, uint32_t& orphans, uint32_t& max_cov, uint64_t& rlo, uint64_t& rhi)
{
    m = in ? m : 0u;
    c = in ? c : 0u;
    meth += m;
    cov += c;
    covered += c > 0u ? 1u : 0u;
    covered_at += (in && (int32_t)c >= depth_at) ? 1u : 0u;
    orphans += (c == 0u && m > 0u) ? 1u : 0u;
    max_cov = c > max_cov ? c : max_cov;
    // fl(fl(m / c) * 100): two IEEE operations; a site without coverage adds the term 0 / 1 * 100 = 0
    const double q = (double)(c > 0u ? m : 0u) / (double)(c > 0u ? c : 1u);
    const double t = q * 100.0;
    const uint64_t bits = (uint64_t)__double_as_longlong(t);
    const bool some = bits != 0ull;
    const uint64_t mant = some ? ((bits & 0x000fffffffffffffull) | 0x0010000000000000ull) : 0ull;
    // t = mant * 2^(e - 1075), in units of 2^-62: mant << (e - 1013); 0 <= e - 1013 <= 32 for every term of uint8 / uint16 counts
    const uint32_t sh = some ? (uint32_t)(bits >> 52) - 1013u : 0u;
    wg_st_add128(rlo, rhi, mant << sh, (mant >> 1) >> (63u - sh));
}

template <int ELEM>
__global__ __launch_bounds__(WG_ST_BLOCK) void k_sample_stats(const uint8_t* __restrict__ rows, int64_t pitch, const int64_t* __restrict__ x0,
                                                              const int64_t* __restrict__ x1, const int64_t* __restrict__ cumv, int64_t n_ranges,
                                                              int64_t n_vec, int32_t depth_at, wg_stat_part* __restrict__ parts, int64_t n_tiles)
{
    constexpr int S = 8 / ELEM;                      // sites per 16-byte vector
    __shared__ uint64_t sh[WG_ST_BLOCK / 64][9];
    const int64_t tile = blockIdx.x;
    const int sample = blockIdx.y;
    const int64_t u0 = tile * WG_ST_TILE;
    const int64_t u1 = u0 + WG_ST_TILE < n_vec ? u0 + WG_ST_TILE : n_vec;          // u0 < n_vec: the grid has ceil(n_vec / TILE) tiles
    // the ranges this tile's units lie in: [lo, hi], lo / hi = last range with cumv[i] <= u0 / u1 - 1 (wave-uniform searches)
    int64_t lo = 0, hi = n_ranges - 1;
    {
        int64_t a = 0, b = n_ranges - 1;
        while (a < b) { const int64_t mid = (a + b + 1) >> 1; if (cumv[mid] <= u0) a = mid; else b = mid - 1; }
        lo = a;
        b = n_ranges - 1;
        while (a < b) { const int64_t mid = (a + b + 1) >> 1; if (cumv[mid] <= u1 - 1) a = mid; else b = mid - 1; }
        hi = a;
    }
    const uint8_t* row = rows + (size_t)sample * (size_t)pitch;
    uint4 vec[WG_ST_VPT];
    int ja[WG_ST_VPT], jb[WG_ST_VPT];                // sites [ja, jb) of vector k belong to its range
#pragma unroll
    for (int k = 0; k < WG_ST_VPT; k++) {
        int64_t u = u0 + (int64_t)k * WG_ST_BLOCK + threadIdx.x;
        const bool live = u < u1;
        u = live ? u : u1 - 1;                       // a thread past the end loads the tile's last vector and masks all of it
        int64_t a = lo, b = hi;
        while (a < b) { const int64_t mid = (a + b + 1) >> 1; if (cumv[mid] <= u) a = mid; else b = mid - 1; }
        const int64_t r0 = x0[a], r1 = x1[a];
        const int64_t v = r0 / S + (u - cumv[a]);    // vector index in the row; r0 >= 0
        vec[k] = *reinterpret_cast<const uint4*>(row + (size_t)v * 16);
        const int64_t s0 = v * S;
        const int64_t f = r0 > s0 ? r0 - s0 : 0, g = r1 < s0 + S ? r1 - s0 : S;
        ja[k] = live ? (int)f : 0;
        jb[k] = live ? (int)g : 0;
    }
    uint32_t meth = 0, cov = 0, covered = 0, covered_at = 0, orphans = 0, max_cov = 0;
    uint64_t rlo = 0, rhi = 0;
#pragma unroll
    for (int k = 0; k < WG_ST_VPT; k++) {
        const uint32_t w[4] = {vec[k].x, vec[k].y, vec[k].z, vec[k].w};
#pragma unroll
        for (int j = 0; j < S; j++) {
            uint32_t m, c;
            if (ELEM == 1) { const uint32_t p = w[j >> 1] >> ((j & 1) * 16); m = p & 0xffu; c = (p >> 8) & 0xffu; }
            else { m = w[j] & 0xffffu; c = w[j] >> 16; }
            wg_st_site(m, c, j >= ja[k] && j < jb[k], depth_at, meth, cov, covered, covered_at, orphans, max_cov, rlo, rhi);
        }
    }
    wg_stat_part p = {meth, cov, covered, covered_at, orphans, max_cov, rlo, rhi};
    const wg_stat_part r = wg_st_block_sum(p, sh);
    if (threadIdx.x == 0) parts[(size_t)sample * (size_t)n_tiles + (size_t)tile] = r;
}

// The tiles' partial results of one sample -> its wgbsseg_sample_stat.  One workgroup per sample.
__global__ __launch_bounds__(WG_ST_BLOCK) void k_sample_stats_fold(const wg_stat_part* __restrict__ parts, int64_t n_tiles, uint64_t n_sites,
                                                                   wg_sample_stat* __restrict__ out)
{
    __shared__ uint64_t sh[WG_ST_BLOCK / 64][9];
    const int sample = blockIdx.x;
    const wg_stat_part* mine = parts + (size_t)sample * (size_t)n_tiles;
    wg_stat_part p = {};
    for (int64_t t = threadIdx.x; t < n_tiles; t += WG_ST_BLOCK) {
        const wg_stat_part q = mine[t];
        p.meth += q.meth; p.cov += q.cov; p.covered += q.covered; p.covered_at += q.covered_at; p.orphans += q.orphans;
        p.max_cov = q.max_cov > p.max_cov ? q.max_cov : p.max_cov;
        wg_st_add128(p.ratio_lo, p.ratio_hi, q.ratio_lo, q.ratio_hi);
    }
    const wg_stat_part r = wg_st_block_sum(p, sh);
    if (threadIdx.x == 0) {
        wg_sample_stat s;
        s.n_sites = n_sites; s.meth_sum = r.meth; s.cov_sum = r.cov; s.covered = r.covered; s.covered_at = r.covered_at;
        s.orphans = r.orphans; s.ratio_lo = r.ratio_lo; s.ratio_hi = r.ratio_hi; s.max_cov = (uint32_t)r.max_cov; s.reserved = 0;
        out[sample] = s;
    }
}
