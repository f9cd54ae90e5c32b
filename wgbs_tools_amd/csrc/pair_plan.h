// pair_plan.h — what host and device agree on for the pairwise histograms (wgbsseg_pair_ranges, wgbsseg_pair_hist) and the
// checks of their arguments.  No HIP here (like env.h and block_plan.h): g++ compiles it alone, tests/native/san_pair.cpp runs
// the checks under the sanitizers.
//
// LDS of one k_pair_hist workgroup: bins * bins uint32 cells and 2 * (bins + 1) edges as doubles.  101 bins (the command's
// default) take 40,804 + 1,632 bytes; 126 bins take 63,504 + 2,032 = 65,536, all a workgroup can have; 127 do not fit.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

#define WG_PH_RUN 32768                // sites one workgroup takes (a multiple of the 8 sites of a 16-byte vector)
#define WG_PH_LDS 65536                // LDS one workgroup can have
#define WG_PH_MAX_BINS 126             // the largest bins with wg_ph_lds_bytes(bins) <= WG_PH_LDS

constexpr int64_t wg_ph_lds_bytes(int64_t bins) { return 4 * bins * bins + 16 * (bins + 1); }
static_assert(wg_ph_lds_bytes(WG_PH_MAX_BINS) <= WG_PH_LDS && wg_ph_lds_bytes(WG_PH_MAX_BINS + 1) > WG_PH_LDS, "WG_PH_MAX_BINS is what fits");
static_assert(WG_PH_MAX_BINS >= 101, "the command's default must fit");
static_assert(WG_PH_RUN % 8 == 0, "a run begins at a 16-byte vector of uint8 and of uint16 rows");

inline bool wg_pair_refuse(std::string& msg, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return false;
}

// The pair list and the threshold against n_samples resident rows of n_sites sites.  false: `msg` names the offender.
inline bool wg_pair_check_list(const char* who, const int32_t* a, const int32_t* b, int64_t n_pairs, int32_t min_cov, int32_t n_samples, int64_t n_sites,
                               std::string& msg)
{
    if (n_pairs < 1) return wg_pair_refuse(msg, "%s: n_pairs = %lld, at least one pair is needed", who, (long long)n_pairs);
    if (!a || !b) return wg_pair_refuse(msg, "%s: the pair list is NULL", who);
    if (min_cov < 1) return wg_pair_refuse(msg, "%s: min_cov = %d must be at least 1 (a site without coverage has no ratio)", who, (int)min_cov);
    for (int64_t i = 0; i < n_pairs; i++)
        if (a[i] < 0 || a[i] >= n_samples || b[i] < 0 || b[i] >= n_samples)
            return wg_pair_refuse(msg, "%s: pair %lld = (%d, %d) names a sample outside the %d resident samples", who, (long long)i, (int)a[i], (int)b[i], (int)n_samples);
    const int64_t n_runs = (n_sites + WG_PH_RUN - 1) / WG_PH_RUN;
    if (n_runs * n_pairs > 0x7fffffff) return wg_pair_refuse(msg, "%s: too many pairs x sites for one call (%lld pairs of %lld sites)", who, (long long)n_pairs, (long long)n_sites);
    return true;
}

inline bool wg_pair_check_bins(int32_t bins, std::string& msg)
{
    if (bins < 1 || bins > WG_PH_MAX_BINS) return wg_pair_refuse(msg, "pair_hist: bins = %d is outside 1 .. %d (what one workgroup's LDS holds)", (int)bins, WG_PH_MAX_BINS);
    return true;
}

// edges [n_pairs][2][bins + 1]: finite and strictly ascending per pair and axis
inline bool wg_pair_check_edges(const double* edges, int64_t n_pairs, int32_t bins, std::string& msg)
{
    if (!edges) return wg_pair_refuse(msg, "pair_hist: edges is NULL");
    for (int64_t p = 0; p < n_pairs; p++)
        for (int ax = 0; ax < 2; ax++) {
            const double* e = edges + ((size_t)p * 2 + (size_t)ax) * (size_t)(bins + 1);
            for (int k = 0; k <= bins; k++) {
                if (!std::isfinite(e[k])) return wg_pair_refuse(msg, "pair_hist: edge %d of axis %d of pair %lld is not finite", k, ax, (long long)p);
                if (k && !(e[k] > e[k - 1]))
                    return wg_pair_refuse(msg, "pair_hist: edge %d of axis %d of pair %lld (%.17g) does not lie above edge %d (%.17g): edges must be strictly ascending",
                                          k, ax, (long long)p, e[k], k - 1, e[k - 1]);
            }
        }
    return true;
}
