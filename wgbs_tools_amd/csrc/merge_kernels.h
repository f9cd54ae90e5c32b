// merge_kernels.h — the row sum of `wgbstools merge` on gfx950: k_beta_merge adds the rows named site by site and applies the reference's
// saturation rule (merge_plan.h: wg_merge_site, shared with the host).  It reads every row once and writes one row: bound by HBM.
//
// One thread per 16-byte vector of a row (8 sites of uint8 pairs, 4 of uint16 pairs): one 16-byte load per lane and row — a wavefront
// reads 1 KiB of a row per instruction —, four rows' loads issued before the first is used, the sums in registers, and the result's
// sites of the vector written with 16-byte stores (8 bytes where 4 sites become uint8 pairs).  The n_total % S sites behind the last
// whole vector go to the threads behind the last vector thread, one site each, count by count: no load reaches beyond a row's
// 2 * ELEM * n_total bytes, so borrowed rows at the tightest pitch are read like the library's own.  Rows and result are 16-byte aligned
// (wgbsseg_set_betas_device checks base and pitch).  Plain C++ only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "merge_plan.h"

template <int ELEM>
__device__ __forceinline__ void wg_mg_add(const uint4& v, uint32_t (&M)[8 / ELEM], uint32_t (&C)[8 / ELEM])
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 8 / ELEM; j++) {
        if constexpr (ELEM == 1) { const uint32_t p = w[j >> 1] >> ((j & 1) * 16); M[j] += p & 0xffu; C[j] += (p >> 8) & 0xffu; }
        else { M[j] += w[j] & 0xffffu; C[j] += w[j] >> 16; }
    }
}

// ELEM / OUT: bytes per count of the rows / of the result
template <int ELEM, int OUT>
__global__ __launch_bounds__(WG_MG_BLOCK) void k_beta_merge(const uint8_t* __restrict__ rows, int64_t pitch, int64_t n_total, const int32_t* __restrict__ samples,
                                                            int32_t n_rows, int64_t n_vec, uint8_t* __restrict__ out)
{
    constexpr int S = 8 / ELEM;
    constexpr uint32_t MAX = OUT == 1 ? 255u : 65535u;
    const int64_t u = (int64_t)blockIdx.x * WG_MG_BLOCK + threadIdx.x;
    if (u < n_vec) {
        uint32_t M[S] = {}, C[S] = {};
        const uint8_t* at = rows + (size_t)u * 16;
        int32_t r = 0;
        for (; r + 4 <= n_rows; r += 4) {
            uint4 v[4];
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = *reinterpret_cast<const uint4*>(at + (size_t)samples[r + k] * (size_t)pitch);
#pragma unroll
            for (int k = 0; k < 4; k++) wg_mg_add<ELEM>(v[k], M, C);
        }
        for (; r < n_rows; r++) wg_mg_add<ELEM>(*reinterpret_cast<const uint4*>(at + (size_t)samples[r] * (size_t)pitch), M, C);
        uint32_t w[S * OUT / 2];                     // the result's sites of this vector, as 32-bit words
#pragma unroll
        for (int j = 0; j < S; j++) {
            uint32_t m, c;
            wg_merge_site(M[j], C[j], MAX, m, c);
            if constexpr (OUT == 1) {
                const uint32_t p = (m & 0xffu) | ((c & 0xffu) << 8);
                if (j & 1) w[j >> 1] |= p << 16; else w[j >> 1] = p;
            } else {
                w[j] = (m & 0xffffu) | ((c & 0xffffu) << 16);
            }
        }
        uint8_t* dst = out + (size_t)u * (size_t)(S * 2 * OUT);
        if constexpr (S * OUT / 2 == 2) {
            *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
        } else {
#pragma unroll
            for (int k = 0; k < S * OUT / 8; k++) reinterpret_cast<uint4*>(dst)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
        }
        return;
    }
    const int64_t site = n_vec * S + (u - n_vec);
    if (site >= n_total) return;
    uint32_t M = 0, C = 0;
    for (int32_t r = 0; r < n_rows; r++) {
        const uint8_t* row = rows + (size_t)samples[r] * (size_t)pitch;
        if (ELEM == 1) { M += row[2 * site]; C += row[2 * site + 1]; }
        else { const uint16_t* q = reinterpret_cast<const uint16_t*>(row); M += q[2 * site]; C += q[2 * site + 1]; }
    }
    uint32_t m, c;
    wg_merge_site(M, C, MAX, m, c);
    if (OUT == 1) { out[2 * site] = (uint8_t)m; out[2 * site + 1] = (uint8_t)c; }
    else { uint16_t* q = reinterpret_cast<uint16_t*>(out); q[2 * site] = (uint16_t)m; q[2 * site + 1] = (uint16_t)c; }
}
