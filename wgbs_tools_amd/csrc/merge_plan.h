// merge_plan.h — the host plan of the row sum of `wgbstools merge` (wgbsseg_merge_rows), the arithmetic of one site, which the host and
// k_beta_merge (merge_kernels.h) share, and the launch constants.  No HIP here (like stats_plan.h, whose wg_plan_refuse it uses): g++
// compiles it alone, tests/native/merge_host.cpp hands it to the tests.
//
// One site.  M = the sum of meth, C = the sum of cov over the rows named: exact integers, uint32 is enough for WG_MG_MAX_ROWS rows of
// uint16.  With max = 255 (65535 for an .lbeta result): where C > max, M = (int64)trunc(fl(fl((double)M / (double)C) * (double)max)) —
// numpy's float64 division, then the product, then the C cast of the assignment into the integer array, in that order — and C = max.
// Then both wrap to the width of the result, as numpy's astype does: a site whose meth exceeds its cov in the input wraps and is no
// error.  The two IEEE operations stay apart (no fast-math, -ffp-contract=off) and are the reference's own, in its order: the result
// does not rest on a proof that an integer M * max / C would round the same way.
//
// The work is cut in 16-byte vectors of a row (S = 8 sites of uint8 pairs, 4 of uint16 pairs): n_total / S whole vectors, one per lane
// and row, and n_total % S sites behind them that are read count by count: nothing beyond the row's 2 * elem * n_total bytes is read.
#pragma once
#include <cstdint>
#include <string>
#include "bed_fmt.h"                                // WG_HD
#include "block_plan.h"

#define WG_MG_BLOCK 256
#define WG_MG_MAX_ROWS 65536                        // 65,536 x 65,535 < 2^32
#define WG_MG_SLAB (8ll << 20)                      // bytes of one fetch through the page-locked staging buffers

WG_HD void wg_merge_site(uint32_t M, uint32_t C, uint32_t max, uint32_t& m, uint32_t& c)
{
    if (C > max) {
        const double q = (double)M / (double)C;
        const double t = q * (double)max;
        M = (uint32_t)(int64_t)t;                   // (t >= 0, and below 2^32: M < 2^32 and max / C < 1)
        C = max;
    }
    m = M; c = C;                                   // (the caller stores them at the result's width: the wrap)
}

struct MergePlan {
    int32_t n_rows = 0;
    int32_t out_elem = 1;      // bytes per count of the result
    uint32_t max = 255;
    int64_t n_vec = 0;         // whole 16-byte vectors of a row
    int64_t n_tail = 0;        // sites behind them
    int64_t n_threads = 0;     // n_vec + n_tail
    int64_t groups = 0;        // workgroups of WG_MG_BLOCK
    int64_t out_bytes = 0;
};

inline int plan_merge_rows(const int32_t* samples, int32_t n_samples, int32_t n_resident, int64_t n_total, int elem, int32_t lbeta_out, const void* out,
                           MergePlan& p, std::string& msg)
{
    p = MergePlan();
    if (n_samples < 1 || !samples) return wg_plan_refuse(msg, "merge_rows: %d rows named (at least 1)", (int)n_samples);
    if (n_samples > WG_MG_MAX_ROWS) return wg_plan_refuse(msg, "merge_rows: %d rows named (at most %d: the sums are 32 bits wide)", (int)n_samples, WG_MG_MAX_ROWS);
    for (int32_t i = 0; i < n_samples; i++)
        if (samples[i] < 0 || samples[i] >= n_resident) return wg_plan_refuse(msg, "merge_rows: no row %d (%d are resident)", (int)samples[i], (int)n_resident);
    if (!out) return wg_plan_refuse(msg, "merge_rows: out is NULL");
    const int64_t S = 8 / elem;
    p.n_rows = n_samples;
    p.out_elem = lbeta_out ? 2 : 1;
    p.max = lbeta_out ? 65535u : 255u;
    p.n_vec = n_total / S;
    p.n_tail = n_total % S;
    p.n_threads = p.n_vec + p.n_tail;
    p.groups = (p.n_threads + WG_MG_BLOCK - 1) / WG_MG_BLOCK;
    p.out_bytes = n_total * 2 * p.out_elem;
    if (p.groups > 0x7fffffff) return wg_plan_refuse(msg, "merge_rows: too many sites for one call");
    return WGBSSEG_OK;
}

inline int64_t wg_merge_slabs(int64_t len) { return (len + WG_MG_SLAB - 1) / WG_MG_SLAB; }
inline int64_t wg_merge_slab_len(int64_t len, int64_t k) { return len - k * WG_MG_SLAB < WG_MG_SLAB ? len - k * WG_MG_SLAB : WG_MG_SLAB; }
