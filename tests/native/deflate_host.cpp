// tests/native/deflate_host.cpp — test shim: the host build of wgbs_tools_amd/csrc/deflate_core.h (the encoder's serial host twin) and
// deflate_plan.h (the cut, the bound, the checks), exported so that tests/test_deflate_cpu.py can compare them with zlib.
//   g++ -O2 -std=c++17 -shared -fPIC deflate_host.cpp -o libdeflate_host.so
#include <cstring>
#include "../../wgbs_tools_amd/csrc/deflate_plan.h"
#include "../../wgbs_tools_amd/csrc/inflate_core.h"

extern "C" {

// text[0 .. n), n <= 65280 -> the member in out (room for n + 31 bytes); returns its size
uint32_t deflate_twin(const uint8_t* text, uint32_t n, uint8_t* out) { return deflate_member_host(text, n, out); }

// the project's own decoder on a payload
int deflate_inflate_twin(const uint8_t* payload, int64_t n_in, uint8_t* out, uint32_t isize) { return inflate_member_host(payload, n_in, out, isize); }

// CRC32 of text as `lanes` contiguous shares combined (the device runs 64)
uint32_t deflate_crc_shares(const uint8_t* text, uint32_t n, int lanes)
{
    uint32_t r = 0;
    for (int l = 0; l < lanes; l++) r ^= wg_def_crc_share(text, n, l, lanes, wg_def_crc_table_host());
    return r ^ 0xffffffffu;
}

// info = {members, slot_bytes, bound, grid}
int deflate_plan(int64_t n, int64_t cap, int waves, int64_t* info, char* msg, size_t msglen)
{
    DeflatePlan p;
    std::string m;
    static const char some = 0;
    const int rc = plan_deflate(n ? &some : nullptr, n, cap ? &some : nullptr, cap, waves, p, m);
    if (msg && msglen) { strncpy(msg, m.c_str(), msglen - 1); msg[msglen - 1] = 0; }
    info[0] = p.members; info[1] = p.slot_bytes; info[2] = p.bound; info[3] = p.grid;
    return rc;
}

// freq[0 .. n) -> lens[0 .. n) by the encoder's length builder (n <= 288)
void deflate_lengths(const uint32_t* freq, int n, int limit, uint8_t* lens, int two)
{
    static WgDeflateState s;
    WgDefHostEx ex;
    wg_def_lengths(ex, freq, n, limit, lens, s, two != 0);
}

int64_t deflate_bound(int64_t n) { return wg_deflate_bound(n); }
int64_t deflate_members(int64_t n) { return wg_deflate_members(n); }
uint32_t deflate_member_len(int64_t n, int64_t i) { return wg_deflate_member_len(n, i); }
int deflate_pitch(void) { return WG_DEF_PITCH; }
void deflate_eof(uint8_t* out) { memcpy(out, WG_BGZF_EOF, sizeof(WG_BGZF_EOF)); }

// the longest code of the first block when it is dynamic, for the literal/length code (which = 0) or the code-length code (1); -1: not dynamic
int deflate_first_block_depth(const uint8_t* payload, int64_t n_in, int which)
{
    WgInflateTables t;
    WgHostIn in{payload, n_in};
    WgBits<WgHostIn> b(in, n_in);
    const int h = b.bits(3);
    if (h < 0 || (h >> 1) != 2) return -1;
    if (which == 1) {
        const int hd = b.bits(14);
        if (hd < 0) return -1;
        int depth = 0;
        for (int i = 0; i < ((hd >> 10) & 15) + 4; i++) { const int v = b.bits(3); if (v > depth) depth = v; }
        return depth;
    }
    if (wg_inf_dynamic(b, t) != WG_INF_OK) return -1;
    int depth = 0;
    for (int l = 1; l < 16; l++)
        if (t.lcnt[l]) depth = l;
    return depth;
}

}  // extern "C"
