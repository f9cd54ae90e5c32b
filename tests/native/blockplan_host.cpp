// tests/native/blockplan_host.cpp — test shim: the host build of wgbs_tools_amd/csrc/block_plan.h, exported so that
// tests/test_blocks_cpu.py can compare the plan of a block reduction and the two tile rules with a numpy restatement.
//   g++ -O2 -std=c++17 -shared -fPIC blockplan_host.cpp -o libblockplan_host.so
#include <cstring>
#include "../../wgbs_tools_amd/csrc/block_plan.h"

extern "C" {

int64_t blockplan_tile_of(int32_t x0, int32_t x1) { return wg_bsr_tile_of(x0, x1); }
int32_t blockplan_ring_reaches(int32_t x0, int32_t x1, int64_t t) { return wg_bsr_ring_reaches(x0, x1, t) ? 1 : 0; }
void blockplan_constants(int32_t* out) { out[0] = WG_BS_TILE; out[1] = WG_BS_RUN; out[2] = WG_BSR_SPL; out[3] = WG_BSR_TILE; out[4] = WG_BSR_RUN; }

// info = {sorted, monotone, n_tiles, n_direct, words of the upload buffer}.  x0, x1, perm, direct: room for n_blocks entries each;
// tile_first: for tile_cap.  The tables are read through BlockSumPlan::view(), as the launches read them.
int blockplan_run(const int64_t* start0, const int64_t* end0, int64_t n_blocks, int64_t n_total, int32_t elem, int32_t mode, int32_t force_general,
                  int32_t* x0, int32_t* x1, int32_t* perm, int32_t* tile_first, int64_t tile_cap, int32_t* direct, int64_t* info, char* msg, size_t msglen)
{
    BlockSumPlan p;
    std::string m;
    const int rc = plan_block_sums(start0, end0, n_blocks, n_total, elem, mode, force_general != 0, p, m);
    if (msg && msglen) { strncpy(msg, m.c_str(), msglen - 1); msg[msglen - 1] = 0; }
    info[0] = p.sorted; info[1] = p.monotone; info[2] = p.n_tiles; info[3] = p.n_direct; info[4] = (int64_t)p.upload.size();
    if (rc != 0 || p.n_blocks == 0) return rc;
    if (p.upload.size() != p.upload_words() || p.n_tiles + 1 > tile_cap) return 1000;
    const BlockSumPlan::View<const int32_t> v = p.view((const int32_t*)p.upload.data());
    memcpy(x0, v.x0, (size_t)n_blocks * 4);
    memcpy(x1, v.x1, (size_t)n_blocks * 4);
    if (v.perm) memcpy(perm, v.perm, (size_t)n_blocks * 4);
    memcpy(tile_first, v.tile_first, (size_t)(p.n_tiles + 1) * 4);
    if (p.n_direct) memcpy(direct, v.direct, (size_t)p.n_direct * 4);
    return rc;
}

}  // extern "C"
