// tests/native/inflate_host.cpp — test shim: the host build of wgbs_tools_amd/csrc/inflate_core.h (the decoder's serial host twin) and
// inflate_plan.h (the BGZF member walk, the line rule), exported so that tests/test_inflate_cpu.py can compare them with zlib and with
// a Python restatement.
//   g++ -O2 -std=c++17 -shared -fPIC inflate_host.cpp -o libinflate_host.so
#include <cstring>
#include "../../wgbs_tools_amd/csrc/inflate_plan.h"

static_assert(sizeof(wg_bgzf_member) == 4 * sizeof(int64_t), "k_bgzf_inflate's member records are 32 bytes");

static void put_msg(const std::string& m, char* msg, size_t msglen)
{
    if (msg && msglen) { strncpy(msg, m.c_str(), msglen - 1); msg[msglen - 1] = 0; }
}

// rows of {in_off, in_len, isize, out_off, file_off}
static void put_members(const std::vector<wg_bgzf_member>& members, int64_t* rows, int64_t cap)
{
    for (size_t i = 0; i < members.size() && (int64_t)i < cap; i++) {
        const wg_bgzf_member& m = members[i];
        int64_t* r = rows + 5 * i;
        r[0] = (int64_t)m.in_off; r[1] = m.in_len; r[2] = m.isize; r[3] = (int64_t)m.out_off; r[4] = (int64_t)m.file_off;
    }
}

extern "C" {

int inflate_twin(const uint8_t* payload, int64_t n_in, uint8_t* out, uint32_t isize) { return inflate_member_host(payload, n_in, out, isize); }

const char* inflate_what(int code) { return wg_inflate_what(code); }

// the longest literal/length code of the stream's first block when that block is dynamic (-1: it is not, or its header is refused)
int inflate_first_block_depth(const uint8_t* payload, int64_t n_in)
{
    WgInflateTables t;
    WgHostIn in{payload, n_in};
    WgBits<WgHostIn> b(in, n_in);
    const int h = b.bits(3);
    if (h < 0 || (h >> 1) != 2 || wg_inf_dynamic(b, t) != WG_INF_OK) return -1;
    int depth = 0;
    for (int l = 1; l < 16; l++)
        if (t.lcnt[l]) depth = l;
    return depth;
}

int inflate_walk(const uint8_t* bytes, int64_t n, uint64_t file_base, int64_t* rows, int64_t cap, int64_t* n_members, int64_t* consumed, char* msg, size_t msglen)
{
    std::vector<wg_bgzf_member> members;
    std::string m;
    const int rc = bgzf_walk(bytes, n, file_base, members, consumed, m);
    put_msg(m, msg, msglen);
    *n_members = (int64_t)members.size();
    put_members(members, rows, cap);
    return rc;
}

// info = {members, consumed, n_dev, comp_bytes, carry_in, text_cap, n_text, length of the new carry}
int inflate_plan(const uint8_t* bytes, int64_t n, uint64_t file_base, const char* carry, int64_t carry_len, int64_t* rows, int64_t cap, int64_t* info,
                 char* new_carry, int64_t new_carry_cap, char* msg, size_t msglen)
{
    BgzfPlan p;
    std::string m;
    const int rc = plan_bgzf(bytes, n, file_base, std::string(carry ? carry : "", (size_t)carry_len), p, m);
    put_msg(m, msg, msglen);
    info[0] = (int64_t)p.members.size(); info[1] = p.consumed; info[2] = p.n_dev; info[3] = p.comp_bytes; info[4] = p.carry_in; info[5] = p.text_cap;
    info[6] = p.n_text; info[7] = (int64_t)p.carry.size();
    put_members(p.members, rows, cap);
    if ((int64_t)p.carry.size() <= new_carry_cap) memcpy(new_carry, p.carry.data(), p.carry.size());
    return rc;
}

}  // extern "C"
