// stats_plan.h — the host plan of the per-sample statistics (wgbsseg_sample_stats) and the tile constants it shares with
// stats_kernels.h.  No HIP here (like block_plan.h, whose wg_plan_refuse it uses): g++ compiles it alone,
// tests/native/patplan_host.cpp hands it to the tests.
//
// A call's ranges go up in ONE buffer of int64 — StatsPlan::upload — laid out as
//     x0 [n_ranges] | x1 [n_ranges] | cumv [n_ranges + 1]
// cumv[i]: the 16-byte vectors of the ranges before range i (stats_kernels.h says how a range is cut in vectors).
// StatsPlan::view() is the only statement of that layout, for the host copy and the device copy alike.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include "block_plan.h"

#define WG_ST_BLOCK 256
#define WG_ST_VPT 4                                 // 16-byte vectors per thread, all loaded before the first is used
#define WG_ST_TILE (WG_ST_BLOCK * WG_ST_VPT)        // vectors per workgroup: 16 KB of one row

struct StatsPlan {
    int64_t n_ranges = 0;
    int64_t n_sites = 0;       // sites of all ranges
    int64_t n_vec = 0;         // 16-byte vectors they touch, a vector two ranges meet in counted for each; 0: nothing to read
    int64_t n_tiles = 0;       // workgroups per sample: ceil(n_vec / WG_ST_TILE)
    std::vector<int64_t> upload;

    template <class T> struct View { T* x0; T* x1; T* cumv; };
    template <class T> View<T> view(T* base) const { return {base, base + n_ranges, base + 2 * n_ranges}; }
};

// Checks the ranges against n_samples rows of n_total sites (`elem` bytes per count) and cuts them in vectors and tiles.
inline int plan_sample_stats(const int64_t* start0, const int64_t* end0, int64_t n_ranges, int64_t n_total, int elem, int32_t n_samples, StatsPlan& p,
                             std::string& msg)
{
    p = StatsPlan();
    if (n_ranges < 0 || (n_ranges && (!start0 || !end0))) return wg_plan_refuse(msg, "bad arguments to sample_stats");
    const int64_t S = 8 / elem;                                  // sites per 16-byte vector of a row
    p.n_ranges = n_ranges;
    p.upload.resize((size_t)n_ranges * 3 + 1);
    const StatsPlan::View<int64_t> v = p.view(p.upload.data());
    for (int64_t i = 0; i < n_ranges; i++) {
        const int64_t a = start0[i], b = end0[i];
        if (a < 0 || b < a || b > n_total)
            return wg_plan_refuse(msg, "sample_stats: range %lld = sites [%lld, %lld) is outside the %lld resident sites or reversed", (long long)i, (long long)a, (long long)b, (long long)n_total);
        if (i && a < end0[i - 1])
            return wg_plan_refuse(msg, "sample_stats: range %lld = sites [%lld, %lld) begins before range %lld ends (%lld): ranges must be ascending and disjoint",
                                  (long long)i, (long long)a, (long long)b, (long long)(i - 1), (long long)end0[i - 1]);
        v.x0[i] = a; v.x1[i] = b; v.cumv[i] = p.n_vec;
        p.n_sites += b - a;
        if (b > a) p.n_vec += (b + S - 1) / S - a / S;
    }
    v.cumv[n_ranges] = p.n_vec;
    p.n_tiles = (p.n_vec + WG_ST_TILE - 1) / WG_ST_TILE;
    if (p.n_tiles > 0x7fffffff || n_samples > 65535) return wg_plan_refuse(msg, "too many sites / samples for one sample_stats call");
    return WGBSSEG_OK;
}
