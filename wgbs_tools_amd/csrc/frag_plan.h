// frag_plan.h — the host plan of `wgbstools frag_len` (wgbsseg_fraglen_create): the checks of the selecting blocks and of the
// histogram's size, the two int32 tables k_frag_hist searches, and the constants it shares with the kernel.  No HIP here (like
// homog_plan.h, whose WG_HOMOG_NO_SITE and, through block_plan.h, wg_plan_refuse it uses): g++ compiles it alone,
// tests/native/fragplan_host.cpp hands it to the tests.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>
#include "homog_plan.h"

#define WG_FRAG_LDS_BINS 2048            // lengths 1..2048 are counted in LDS (64-bit counters: 16 KB), longer ones in global memory
#define WG_FRAG_MAX_BINS (1 << 20)       // the largest max_frag
#define WG_FRAG_GROUPS 1536              // workgroups of a launch at most: 256 CUs x the 6 whose LDS (the tile + the histogram: ~26 KB) fits one CU

struct FragPlan {
    std::vector<int32_t> start, pmax;             // startCpG and the running maximum of endCpG: the blocks in the order given
    int64_t end_last = 0;                         // endCpG of the block that sorts last: a read starting there or behind is dropped
    int64_t n_blocks = 0;                         // 0: every read is selected
    int32_t max_frag = 0;
    int32_t groups = WG_FRAG_GROUPS;
};

// The blocks arrive in the order `sort -k1,1n` gives the text "startCpG\tendCpG" (startCpG ascending; how equal starts are ordered
// is the caller's business and is kept).  n_blocks == 0: no selection.
inline int plan_frag(const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, int32_t max_frag, FragPlan& p, std::string& msg)
{
    p = FragPlan();
    if (max_frag < 1 || max_frag > WG_FRAG_MAX_BINS) return wg_plan_refuse(msg, "frag_len: max_frag_size %d (1..%d)", (int)max_frag, (int)WG_FRAG_MAX_BINS);
    if (n_blocks < 0 || n_blocks > 0x7fffffffLL || (n_blocks && (!start_cpg || !end_cpg))) return wg_plan_refuse(msg, "frag_len: bad block list");
    p.max_frag = max_frag;
    p.n_blocks = n_blocks;
    p.start.resize((size_t)n_blocks); p.pmax.resize((size_t)n_blocks);
    int32_t run = 0;
    for (int64_t j = 0; j < n_blocks; j++) {
        const int64_t a = start_cpg[j], b = end_cpg[j];
        if (a < 1) return wg_plan_refuse(msg, "frag_len: block %lld (in sorted order) has startCpG %lld < 1", (long long)j, (long long)a);
        if (b <= a || b > 0x7fffffffLL) return wg_plan_refuse(msg, "frag_len: block %lld (in sorted order) has endCpG %lld (startCpG %lld)", (long long)j, (long long)b, (long long)a);
        if (j && a < start_cpg[j - 1]) return wg_plan_refuse(msg, "frag_len: blocks must be given sorted by startCpG (block %lld)", (long long)j);
        p.start[(size_t)j] = (int32_t)a;
        run = std::max(run, (int32_t)b);
        p.pmax[(size_t)j] = run;
    }
    p.end_last = n_blocks ? end_cpg[n_blocks - 1] : 0;
    return WGBSSEG_OK;
}

// the grid's cap: `groups` < 0 -> the default; a small value is the test hook for the tile loop
inline int plan_frag_groups(int32_t groups, FragPlan& p, std::string& msg)
{
    if (groups == 0 || groups > WG_FRAG_GROUPS) return wg_plan_refuse(msg, "frag_len: %d workgroups (1..%d, or -1 for the default)", (int)groups, (int)WG_FRAG_GROUPS);
    p.groups = groups < 0 ? WG_FRAG_GROUPS : groups;
    return WGBSSEG_OK;
}
