// mask_plan.h — the host plan of `wgbstools mask_pat`'s site mask (wgbsseg_patview_set_mask): the checks of the blocks with their messages,
// the union of the blocks as disjoint ascending intervals — what k_view_mask_fill (view_kernels.h) composes the bitmap of view_core.h's
// wg_view_mask from —, the bitmap's range and size, and the number of hidden sites (the reference's `loaded N sites`, mask_pat.cpp:12-75).
// No HIP here (like frag_plan.h): g++ compiles it alone, tests/native/mask_host.cpp hands it to the tests.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#include "block_plan.h"                // wg_plan_refuse
#include "view_core.h"

#define WG_MASK_MAX_SITE 0x7fffffffLL    // the reference keeps sites as int

struct MaskPlan {
    std::vector<int64_t> starts, ends;   // the union: [starts[k], ends[k]) ascending, ends[k] < starts[k + 1]
    int64_t lo = 0, hi = 0;              // the bitmap covers the sites [lo, hi)
    int64_t n_words = 0;
    int64_t n_hidden = 0;
    int64_t n_intervals() const { return (int64_t)starts.size(); }
};

// The blocks [start_cpg[k], end_cpg[k]) in any order; they may overlap, nest and repeat.  A refusal names the block's index in the list.
inline int plan_mask(const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, MaskPlan& p, std::string& msg)
{
    p = MaskPlan();
    if (n_blocks < 0 || (n_blocks && (!start_cpg || !end_cpg))) return wg_plan_refuse(msg, "bad arguments to patview_set_mask");
    if (n_blocks == 0) return wg_plan_refuse(msg, "mask: no blocks (at least 1)");
    for (int64_t i = 0; i < n_blocks; i++) {
        if (start_cpg[i] < 1) return wg_plan_refuse(msg, "mask: block %lld starts at site %lld (sites count from 1)", (long long)i, (long long)start_cpg[i]);
        if (end_cpg[i] <= start_cpg[i])
            return wg_plan_refuse(msg, "mask: block %lld = sites [%lld, %lld) is empty", (long long)i, (long long)start_cpg[i], (long long)end_cpg[i]);
        if (end_cpg[i] > WG_MASK_MAX_SITE) return wg_plan_refuse(msg, "mask: block %lld ends at site %lld (at most %lld)", (long long)i, (long long)end_cpg[i], WG_MASK_MAX_SITE);
    }
    std::vector<std::pair<int64_t, int64_t>> b((size_t)n_blocks);
    for (int64_t i = 0; i < n_blocks; i++) b[(size_t)i] = {start_cpg[i], end_cpg[i]};
    std::sort(b.begin(), b.end());
    for (const auto& x : b) {
        if (!p.ends.empty() && x.first <= p.ends.back()) p.ends.back() = std::max(p.ends.back(), x.second);     // overlaps or touches the one before
        else { p.starts.push_back(x.first); p.ends.push_back(x.second); }
    }
    for (size_t k = 0; k < p.starts.size(); k++) p.n_hidden += p.ends[k] - p.starts[k];
    p.lo = p.starts.front(); p.hi = p.ends.back();
    p.n_words = wg_view_mask_words(p.lo, p.hi);
    return WGBSSEG_OK;
}

// Word w of the bitmap from the plan's intervals, as k_view_mask_fill composes it: the first interval that ends behind the word's first
// site by binary search, then every interval that begins before the word's end.
WG_HD int64_t wg_mask_first_interval(const int64_t* ends, int64_t n, int64_t site)
{
    int64_t a = 0, b = n;                                           // the first k with ends[k] > site
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (ends[m] > site) b = m; else a = m + 1;
    }
    return a;
}

WG_HD uint32_t wg_mask_word(const int64_t* starts, const int64_t* ends, int64_t n, int64_t lo, int64_t w)
{
    const int64_t first = lo + 32 * w, last = first + 32;
    uint32_t v = 0;
    for (int64_t k = wg_mask_first_interval(ends, n, first); k < n && starts[k] < last; k++) {
        const int64_t from = starts[k] > first ? starts[k] - first : 0, to = ends[k] < last ? ends[k] - first : 32;      // bits [from, to), 0 <= from < to <= 32
        v |= (to - from == 32 ? 0xffffffffu : ((1u << (to - from)) - 1u) << from);
    }
    return v;
}
