// homog_plan.h — the host plan of `wgbstools homog` (wgbsseg_homog_create): the checks of the block table and the bin edges, and
// the three int32 tables k_homog_count reads.  No HIP here (like block_plan.h, whose wg_plan_refuse it uses): g++ compiles it
// alone, tests/native/patplan_host.cpp hands it to the tests.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>
#include "block_plan.h"

#define WG_HOMOG_MAX_BINS 8
#define WG_HOMOG_NO_SITE ((long long)INT64_MIN)      // no read yet (prev_in / prev_out), no line (a round's starts)

struct HomogPlan {
    std::vector<int32_t> s32, e32, pmax;          // startCpG, endCpG, running maximum of endCpG: the blocks in (startCpG, endCpG) order
    int64_t last_end = 0;                         // endCpG of the last block: a read starting there or behind counts nowhere
};

// range: n_bins + 1 edges
inline int plan_homog(const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, const float* range, int32_t n_bins, int32_t min_cpgs, HomogPlan& p,
                      std::string& msg)
{
    p = HomogPlan();
    if (n_blocks < 1 || !start_cpg || !end_cpg) return wg_plan_refuse(msg, "homog: no blocks");
    if (!range || n_bins < 1 || n_bins > WG_HOMOG_MAX_BINS) return wg_plan_refuse(msg, "homog: %d bins (1..%d)", (int)n_bins, WG_HOMOG_MAX_BINS);
    for (int b = 0; b < n_bins; b++)
        if (!(range[b] < range[b + 1])) return wg_plan_refuse(msg, "homog: the range is not ascending");
    if (min_cpgs < 1) return wg_plan_refuse(msg, "homog: min_cpgs %d < 1", (int)min_cpgs);
    p.s32.resize((size_t)n_blocks); p.e32.resize((size_t)n_blocks); p.pmax.resize((size_t)n_blocks);
    int32_t run = 0;
    for (int64_t j = 0; j < n_blocks; j++) {
        const int64_t a = start_cpg[j], b = end_cpg[j];
        if (a < 1) return wg_plan_refuse(msg, "homog: block %lld (in sorted order) has startCpG %lld < 1", (long long)j, (long long)a);
        if (b <= a || b > 0x7fffffffLL) return wg_plan_refuse(msg, "homog: block %lld (in sorted order) has endCpG %lld (startCpG %lld)", (long long)j, (long long)b, (long long)a);
        if (j && (a < start_cpg[j - 1] || (a == start_cpg[j - 1] && b < end_cpg[j - 1])))
            return wg_plan_refuse(msg, "homog: blocks must be given sorted by (startCpG, endCpG) (block %lld)", (long long)j);
        p.s32[(size_t)j] = (int32_t)a; p.e32[(size_t)j] = (int32_t)b;
        run = std::max(run, (int32_t)b);
        p.pmax[(size_t)j] = run;
    }
    p.last_end = end_cpg[n_blocks - 1];
    return WGBSSEG_OK;
}
