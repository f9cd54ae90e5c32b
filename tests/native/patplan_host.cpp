// tests/native/patplan_host.cpp — test shim: the host build of wgbs_tools_amd/csrc/bimodal_plan.h, homog_plan.h and stats_plan.h,
// exported so that tests/test_patplan_cpu.py can compare the plans with numpy restatements and walk the retire / drop rules.
//   g++ -O2 -std=c++17 -shared -fPIC patplan_host.cpp -o libpatplan_host.so
#include <cstring>
#include "../../wgbs_tools_amd/csrc/bimodal_plan.h"
#include "../../wgbs_tools_amd/csrc/homog_plan.h"
#include "../../wgbs_tools_amd/csrc/stats_plan.h"

static_assert(sizeof(wg_bim_meta) == 6 * sizeof(int64_t), "the tests hand k_bim_gather's records over as rows of six int64");

static void put_msg(const std::string& m, char* msg, size_t msglen)
{
    if (msg && msglen) { strncpy(msg, m.c_str(), msglen - 1); msg[msglen - 1] = 0; }
}

extern "C" {

void patplan_constants(int64_t* out)
{
    out[0] = WG_BIM_CTX; out[1] = WG_BIM_LDS_COLS; out[2] = WG_BIM_COL_BYTES; out[3] = WG_BIM_MAX_ITERS; out[4] = WG_BIM_NONE;
    out[5] = WG_HOMOG_MAX_BINS; out[6] = WG_HOMOG_NO_SITE; out[7] = WG_ST_BLOCK; out[8] = WG_ST_VPT; out[9] = WG_ST_TILE;
}

// a plan to walk (nullptr when refused; *rc and msg say why)
void* patplan_bim_new(const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, int32_t min_len, int32_t max_lds_cols, int32_t* rc, char* msg, size_t msglen)
{
    BimodalPlan* p = new BimodalPlan();
    std::string m;
    *rc = plan_bimodal(start_cpg, end_cpg, n_blocks, min_len, max_lds_cols, *p, m);
    put_msg(m, msg, msglen);
    if (*rc != WGBSSEG_OK) { delete p; return nullptr; }
    return p;
}
void patplan_bim_free(void* h) { delete static_cast<BimodalPlan*>(h); }

// s1, s2, by_end: n_blocks entries each; lo_after: n_blocks + 1.  Returns lds_cols.
int32_t patplan_bim_tables(const void* h, int32_t* s1, int32_t* s2, int32_t* by_end, int64_t* lo_after)
{
    const BimodalPlan& p = *static_cast<const BimodalPlan*>(h);
    const size_t nb = (size_t)p.n_blocks;
    if (p.s1.size() != nb || p.s2.size() != nb || p.by_end.size() != nb || p.lo_after.size() != nb + 1) return -1000;
    memcpy(s1, p.s1.data(), nb * 4); memcpy(s2, p.s2.data(), nb * 4); memcpy(by_end, p.by_end.data(), nb * 4);
    memcpy(lo_after, p.lo_after.data(), (nb + 1) * 8);
    return p.lds_cols;
}
int64_t patplan_bim_retire_upto(const void* h, int64_t pending, int64_t last_start) { return static_cast<const BimodalPlan*>(h)->retire_upto(pending, last_start); }
int64_t patplan_bim_drop_below(const void* h, int64_t pending) { return static_cast<const BimodalPlan*>(h)->drop_below(pending); }

void patplan_bim_chunk_bound(int64_t n_bytes, uint64_t* out)
{
    const BimodalChunkBound ub(n_bytes);
    out[0] = ub.lines; out[1] = ub.words;
}

// meta: n rows of {ra, rb, first_ind, ncols, rows, lines}
int patplan_bim_scratch(const int64_t* meta, const int32_t* ids, int64_t n, int32_t lds_cols, int64_t* off, uint64_t* used, char* msg, size_t msglen)
{
    std::string m;
    size_t u = 0;
    const int rc = wg_bim_scratch_layout(reinterpret_cast<const wg_bim_meta*>(meta), ids, n, lds_cols, reinterpret_cast<long long*>(off), u, m);
    put_msg(m, msg, msglen);
    *used = u;
    return rc;
}

// s32, e32, pmax: n_blocks entries each
int patplan_homog(const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, const float* range, int32_t n_bins, int32_t min_cpgs,
                  int32_t* s32, int32_t* e32, int32_t* pmax, int64_t* last_end, char* msg, size_t msglen)
{
    HomogPlan p;
    std::string m;
    const int rc = plan_homog(start_cpg, end_cpg, n_blocks, range, n_bins, min_cpgs, p, m);
    put_msg(m, msg, msglen);
    if (rc != WGBSSEG_OK) return rc;
    const size_t nb = (size_t)n_blocks;
    if (p.s32.size() != nb || p.e32.size() != nb || p.pmax.size() != nb) return 1000;
    memcpy(s32, p.s32.data(), nb * 4); memcpy(e32, p.e32.data(), nb * 4); memcpy(pmax, p.pmax.data(), nb * 4);
    *last_end = p.last_end;
    return rc;
}

// x0, x1: n_ranges entries; cumv: n_ranges + 1; info = {n_sites, n_vec, n_tiles}.  The tables are read through StatsPlan::view(), as the launches read them.
int patplan_stats(const int64_t* start0, const int64_t* end0, int64_t n_ranges, int64_t n_total, int32_t elem, int32_t n_samples,
                  int64_t* x0, int64_t* x1, int64_t* cumv, int64_t* info, char* msg, size_t msglen)
{
    StatsPlan p;
    std::string m;
    const int rc = plan_sample_stats(start0, end0, n_ranges, n_total, elem, n_samples, p, m);
    put_msg(m, msg, msglen);
    if (rc != WGBSSEG_OK) return rc;
    if (p.n_ranges != n_ranges || p.upload.size() != (size_t)n_ranges * 3 + 1) return 1000;
    const StatsPlan::View<const int64_t> v = p.view((const int64_t*)p.upload.data());
    memcpy(x0, v.x0, (size_t)n_ranges * 8); memcpy(x1, v.x1, (size_t)n_ranges * 8); memcpy(cumv, v.cumv, (size_t)(n_ranges + 1) * 8);
    info[0] = p.n_sites; info[1] = p.n_vec; info[2] = p.n_tiles;
    return rc;
}

}  // extern "C"
