// tests/native/fragplan_host.cpp — test shim: the host build of wgbs_tools_amd/csrc/frag_plan.h, exported so that
// tests/test_frag_len_cpu.py can compare the plan with a numpy restatement and read every refusal.
//   g++ -O2 -std=c++17 -shared -fPIC fragplan_host.cpp -o libfragplan_host.so
#include <cstring>
#include "../../wgbs_tools_amd/csrc/frag_plan.h"

static void put_msg(const std::string& m, char* msg, size_t msglen)
{
    if (msg && msglen) { strncpy(msg, m.c_str(), msglen - 1); msg[msglen - 1] = 0; }
}

extern "C" {

void fragplan_constants(int64_t* out)
{
    out[0] = WG_FRAG_LDS_BINS; out[1] = WG_FRAG_MAX_BINS; out[2] = WG_FRAG_GROUPS;
}

// start, pmax: n_blocks entries each; info = {end_last, n_blocks, max_frag, groups}
int fragplan(const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, int32_t max_frag, int32_t groups, int32_t* start, int32_t* pmax,
             int64_t* info, char* msg, size_t msglen)
{
    FragPlan p;
    std::string m;
    int rc = plan_frag(start_cpg, end_cpg, n_blocks, max_frag, p, m);
    if (rc == WGBSSEG_OK) rc = plan_frag_groups(groups, p, m);
    put_msg(m, msg, msglen);
    if (rc != WGBSSEG_OK) return rc;
    const size_t nb = (size_t)n_blocks;
    if (p.start.size() != nb || p.pmax.size() != nb) return 1000;
    if (nb) { memcpy(start, p.start.data(), nb * 4); memcpy(pmax, p.pmax.data(), nb * 4); }
    info[0] = p.end_last; info[1] = p.n_blocks; info[2] = p.max_frag; info[3] = p.groups;
    return rc;
}

}  // extern "C"
