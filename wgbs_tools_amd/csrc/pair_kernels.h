// pair_kernels.h — all-pairs 2-D histograms of the resident rows (`wgbstools compare_betas`): for a list of sample pairs (a, b),
// the sites where both have coverage >= min_cov, histogrammed by (fl(meth_b / cov_b), fl(meth_a / cov_a)) into bins x bins
// cells ("Pairwise histograms").  Two passes, because the cell edges of a pair come from the pair's own masked
// values: k_pair_ranges gives each pair's site count and the min / max of either ratio, the host turns them into edges
// (np.linspace's own doubles), k_pair_hist counts against those edges.
//
// Exactness.  A ratio is ONE IEEE division of two integers converted to double (plain `/`, no fast-math): numpy's uint8 /
// uint8 in float64.  The ratios are non-negative, so their bit patterns order like unsigned integers: min and max run on the
// bits (thread, wavefront, workgroup, then 64-bit atomics on the device) and cannot depend on the order.  The cell of a value is
// searchsorted(edges, v, 'right') - 1 with v == the last edge in the last cell and anything outside the edges dropped: a guess
// from (v - lo) * bins / (hi - lo) is only where the search over the edges THEMSELVES starts.  Counts are integers all the way
// (uint32 in LDS, uint64 in HBM): any launch geometry gives the same bytes.
//
// One workgroup takes one pair and one run of WG_PH_RUN sites.  The rows are read with aligned 16-byte loads (the run begins at a
// multiple of the vector; the sites of the last vector behind n_sites are masked; a row's pitch covers its last vector).
// Workgroups are numbered run-major, pair fastest: the pairs of one run read the same 2 * n_samples pieces of rows from L2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pair_plan.h"
#include "wave_prims.h"

#define WG_PH_BLOCK 256

// what k_pair_ranges leaves per pair: the ratios' bit patterns (a_min = b_min = ~0 and the maxima 0 before the first site)
struct wg_pair_range {
    uint64_t n, a_min, a_max, b_min, b_max;
};

__device__ __forceinline__ uint64_t wg_ph_shfl_xor_u64(uint64_t v, int d)
{
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wg_ph_wave_min_u64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint64_t o = wg_ph_shfl_xor_u64(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ uint64_t wg_ph_wave_max_u64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const uint64_t o = wg_ph_shfl_xor_u64(v, d); v = o > v ? o : v; }
    return v;
}

// site j of a 16-byte vector of (meth, cov) pairs
template <int ELEM>
__device__ __forceinline__ void wg_ph_site(const uint4& q, int j, uint32_t& m, uint32_t& c)
{
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
    if (ELEM == 1) { const uint32_t p = w[j >> 1] >> ((j & 1) * 16); m = p & 0xffu; c = (p >> 8) & 0xffu; }
    else { m = w[j] & 0xffffu; c = w[j] >> 16; }
}

// Pass 1.  grid = n_runs * n_pairs workgroups.  out[pair] must hold {0, ~0, 0, ~0, 0} before the launch; the bit patterns it holds
// afterwards ARE wgbsseg_pair_range's doubles (the host zeroes those of a pair without sites).
template <int ELEM>
__global__ __launch_bounds__(WG_PH_BLOCK) void k_pair_ranges(const uint8_t* __restrict__ rows, int64_t pitch, int64_t n_sites, const int32_t* __restrict__ pa,
                                                             const int32_t* __restrict__ pb, int32_t n_pairs, int32_t min_cov, wg_pair_range* __restrict__ out)
{
    constexpr int S = 8 / ELEM;                      // sites per 16-byte vector
    __shared__ uint64_t sh[WG_PH_BLOCK / 64][5];
    const int pair = (int)(blockIdx.x % (unsigned)n_pairs);
    const int64_t run = blockIdx.x / (unsigned)n_pairs;
    const int64_t s0 = run * WG_PH_RUN;
    const int64_t s1 = s0 + WG_PH_RUN < n_sites ? s0 + WG_PH_RUN : n_sites;
    const uint8_t* rowa = rows + (size_t)pa[pair] * (size_t)pitch;
    const uint8_t* rowb = rows + (size_t)pb[pair] * (size_t)pitch;
    uint32_t n = 0;
    uint64_t amin = ~0ull, amax = 0, bmin = ~0ull, bmax = 0;
    for (int64_t v = s0 / S + threadIdx.x; v * S < s1; v += WG_PH_BLOCK) {
        const uint4 qa = *reinterpret_cast<const uint4*>(rowa + (size_t)v * 16);
        const uint4 qb = *reinterpret_cast<const uint4*>(rowb + (size_t)v * 16);
#pragma unroll
        for (int j = 0; j < S; j++) {
            uint32_t ma, ca, mb, cb;
            wg_ph_site<ELEM>(qa, j, ma, ca);
            wg_ph_site<ELEM>(qb, j, mb, cb);
            const bool in = v * S + j < s1 && (int32_t)(ca < cb ? ca : cb) >= min_cov;       // min_cov >= 1: a site that is in has coverage
            const uint64_t ba = (uint64_t)__double_as_longlong((double)ma / (double)(in ? ca : 1u));
            const uint64_t bb = (uint64_t)__double_as_longlong((double)mb / (double)(in ? cb : 1u));
            n += in ? 1u : 0u;
            amin = in && ba < amin ? ba : amin;
            amax = in && ba > amax ? ba : amax;
            bmin = in && bb < bmin ? bb : bmin;
            bmax = in && bb > bmax ? bb : bmax;
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t wn = wg_wave_sum_u64(n);
    amin = wg_ph_wave_min_u64(amin); amax = wg_ph_wave_max_u64(amax);
    bmin = wg_ph_wave_min_u64(bmin); bmax = wg_ph_wave_max_u64(bmax);
    if (lane == 0) { sh[wave][0] = wn; sh[wave][1] = amin; sh[wave][2] = amax; sh[wave][3] = bmin; sh[wave][4] = bmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t r[5] = {sh[0][0], sh[0][1], sh[0][2], sh[0][3], sh[0][4]};
        for (int w = 1; w < WG_PH_BLOCK / 64; w++) {
            r[0] += sh[w][0];
            r[1] = sh[w][1] < r[1] ? sh[w][1] : r[1]; r[2] = sh[w][2] > r[2] ? sh[w][2] : r[2];
            r[3] = sh[w][3] < r[3] ? sh[w][3] : r[3]; r[4] = sh[w][4] > r[4] ? sh[w][4] : r[4];
        }
        if (r[0]) {                                  // device-scope atomics: the runs of a pair are spread over the chip
            wg_pair_range* o = out + pair;
            atomicAdd(reinterpret_cast<unsigned long long*>(&o->n), (unsigned long long)r[0]);
            atomicMin(reinterpret_cast<unsigned long long*>(&o->a_min), (unsigned long long)r[1]);
            atomicMax(reinterpret_cast<unsigned long long*>(&o->a_max), (unsigned long long)r[2]);
            atomicMin(reinterpret_cast<unsigned long long*>(&o->b_min), (unsigned long long)r[3]);
            atomicMax(reinterpret_cast<unsigned long long*>(&o->b_max), (unsigned long long)r[4]);
        }
    }
}

// searchsorted(e, v, 'right') - 1 over bins + 1 ascending edges in LDS, v == e[bins] in the last cell, -1 for a value outside.
// `lo` = e[0], `scale` = bins / (e[bins] - e[0]) only place the start of the search (a NaN or an overflow there starts it at an end).
__device__ __forceinline__ int wg_ph_cell(const double* e, int bins, double lo, double scale, double v)
{
    const double t = (v - lo) * scale;
    int g = t >= 0.0 ? (t < (double)(bins - 1) ? (int)t : bins - 1) : 0;
    while (g > 0 && v < e[g]) g--;
    while (g < bins - 1 && v >= e[g + 1]) g++;
    return (v < e[g] || v > e[bins]) ? -1 : g;
}

// Pass 2.  grid = n_runs * n_pairs workgroups, wg_ph_lds_bytes(bins) of dynamic LDS: x edges | y edges | the histogram.
// x = sample b, y = sample a; counts[pair][x_cell][y_cell] must be zero before the launch.
// CORNERS: the cells (first, first) and (last, last) — where most sites of a concordant pair of bimodal samples fall — are
// counted in registers and added to the LDS histogram once per wavefront; the rest goes through LDS atomics either way.
// Measured on the benchmark rows (10 % of the counted sites in the corners): 5 % slower than without, so the library launches
// CORNERS = false unless WGBSSEG_PAIR_CORNERS=1.
template <int ELEM, bool CORNERS>
__global__ __launch_bounds__(WG_PH_BLOCK) void k_pair_hist(const uint8_t* __restrict__ rows, int64_t pitch, int64_t n_sites, const int32_t* __restrict__ pa,
                                                           const int32_t* __restrict__ pb, int32_t n_pairs, int32_t min_cov, int32_t bins,
                                                           const double* __restrict__ edges, unsigned long long* __restrict__ counts)
{
    constexpr int S = 8 / ELEM;
    extern __shared__ double wg_ph_lds[];
    double* ex = wg_ph_lds;
    double* ey = ex + (bins + 1);
    uint32_t* hist = reinterpret_cast<uint32_t*>(ey + (bins + 1));
    const int pair = (int)(blockIdx.x % (unsigned)n_pairs);
    const int64_t run = blockIdx.x / (unsigned)n_pairs;
    const int cells = bins * bins;
    const double* ge = edges + (size_t)pair * 2 * (size_t)(bins + 1);
    for (int i = threadIdx.x; i < 2 * (bins + 1); i += WG_PH_BLOCK) ex[i] = ge[i];
    for (int i = threadIdx.x; i < cells; i += WG_PH_BLOCK) hist[i] = 0u;
    __syncthreads();
    const double xlo = ex[0], ylo = ey[0];
    const double xscale = (double)bins / (ex[bins] - xlo), yscale = (double)bins / (ey[bins] - ylo);
    const int64_t s0 = run * WG_PH_RUN;
    const int64_t s1 = s0 + WG_PH_RUN < n_sites ? s0 + WG_PH_RUN : n_sites;
    const uint8_t* rowa = rows + (size_t)pa[pair] * (size_t)pitch;
    const uint8_t* rowb = rows + (size_t)pb[pair] * (size_t)pitch;
    uint32_t first = 0, last = 0;                    // CORNERS: this thread's sites in cell 0 and in cell cells - 1
    for (int64_t v = s0 / S + threadIdx.x; v * S < s1; v += WG_PH_BLOCK) {
        const uint4 qa = *reinterpret_cast<const uint4*>(rowa + (size_t)v * 16);
        const uint4 qb = *reinterpret_cast<const uint4*>(rowb + (size_t)v * 16);
#pragma unroll
        for (int j = 0; j < S; j++) {
            uint32_t ma, ca, mb, cb;
            wg_ph_site<ELEM>(qa, j, ma, ca);
            wg_ph_site<ELEM>(qb, j, mb, cb);
            const bool in = v * S + j < s1 && (int32_t)(ca < cb ? ca : cb) >= min_cov;
            if (!in) continue;
            const int cx = wg_ph_cell(ex, bins, xlo, xscale, (double)mb / (double)cb);
            const int cy = wg_ph_cell(ey, bins, ylo, yscale, (double)ma / (double)ca);
            if (cx < 0 || cy < 0) continue;
            const int cell = cx * bins + cy;
            if (CORNERS && cell == 0) first++;
            else if (CORNERS && cell == cells - 1) last++;
            else atomicAdd(&hist[cell], 1u);
        }
    }
    if (CORNERS) {                                   // (all 64 lanes are here again: the loop above has ended for the wavefront)
        first = wg_wave_sum_u32(first);
        last = wg_wave_sum_u32(last);
        if ((threadIdx.x & 63) == 0) {
            if (first) atomicAdd(&hist[0], first);
            if (last) atomicAdd(&hist[cells - 1], last);
        }
    }
    __syncthreads();
    unsigned long long* out = counts + (size_t)pair * (size_t)cells;
    for (int i = threadIdx.x; i < cells; i += WG_PH_BLOCK) {
        const uint32_t h = hist[i];
        if (h) atomicAdd(out + i, (unsigned long long)h);
    }
}
