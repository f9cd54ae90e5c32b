// inflate_plan.h — the host plan of a BGZF byte string handed to wgbsseg_*_feed_bgzf / wgbsseg_bgzf_inflate: the walk over its members
// (the SAM specification, 4.1: gzip members whose extra field holds the subfield 'BC' with the member's size - 1), the member table
// k_bgzf_inflate reads, the bytes consumed (a member cut off by the end of the bytes is left to the caller, who hands it in again with
// what follows), and the line rule.  No HIP here: g++ compiles it alone, tests/native/inflate_host.cpp hands it to the tests.
//
// The line rule: a chunk an engine's kernels read ends with a complete line and the host knows its length.  So the plan inflates the
// last member of a call here (inflate_core.h's host twin) and finds its last newline; the text behind it is the new carry, kept on the
// host and put in front of the next call's text.  A last member without a newline joins the carry whole and the member before it is
// asked, and so on; a call without any newline ends up in the carry altogether (rare and slow, and correct).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>
#include "block_plan.h"
#include "inflate_core.h"

#define WG_BGZF_MAX_ISIZE 65536

inline const char* wg_inflate_what(int code)
{
    static const char* const what[WG_INF_CODES] = {
        "no error", "invalid block type", "invalid stored block lengths", "too many length or distance symbols", "invalid code lengths set",
        "invalid bit length repeat (no length before it)", "invalid bit length repeat (past the last length)", "invalid code -- missing end-of-block",
        "invalid literal/lengths set", "invalid distances set", "invalid literal/length code", "invalid distance code", "invalid distance too far back",
        "the compressed data end before the stream does", "more text than the member's ISIZE", "less text than the member's ISIZE"};
    return code >= 0 && code < WG_INF_CODES ? what[code] : "unknown error";
}

// "Invalid gzip data: BGZF member at file offset N: <what>" — the refusal of a member, wherever it was decoded
inline int wg_inflate_refuse(std::string& msg, unsigned long long file_off, int code)
{
    return wg_plan_refuse(msg, "Invalid gzip data: BGZF member at file offset %llu: %s", file_off, wg_inflate_what(code));
}

// The complete members of bytes[0 .. n) (file offset of bytes[0]: file_base): in_off relative to bytes, out_off the running sum of ISIZE
// from 0.  *consumed: the bytes they take; what follows is the beginning of one more member.
inline int bgzf_walk(const uint8_t* bytes, int64_t n, uint64_t file_base, std::vector<wg_bgzf_member>& members, int64_t* consumed, std::string& msg)
{
    members.clear();
    *consumed = 0;
    if (n < 0 || (n && !bytes)) return wg_plan_refuse(msg, "bad arguments to the BGZF walk");
    int64_t pos = 0;
    uint64_t out = 0;
    while (pos < n) {
        const uint8_t* h = bytes + pos;
        const int64_t rem = n - pos;
        const unsigned long long at = (unsigned long long)(file_base + (uint64_t)pos);
        if (h[0] != 0x1f || (rem > 1 && h[1] != 0x8b)) return wg_plan_refuse(msg, "Invalid gzip data: no gzip member at file offset %llu", at);
        if (rem < 12) break;
        if (h[2] != 8 || h[3] != 4) return wg_plan_refuse(msg, "Invalid gzip data: the member at file offset %llu is gzip but not BGZF (no extra field)", at);
        const int64_t xlen = h[10] | (h[11] << 8);
        if (rem < 12 + xlen) break;
        int64_t size = 0;
        for (int64_t q = 12; q + 4 <= 12 + xlen;) {                // the subfields: SI1 SI2 SLEN data
            const int64_t slen = h[q + 2] | (h[q + 3] << 8);
            if (h[q] == 66 && h[q + 1] == 67 && slen == 2 && q + 6 <= 12 + xlen) { size = (h[q + 4] | (h[q + 5] << 8)) + 1; break; }
            q += 4 + slen;
        }
        if (!size) return wg_plan_refuse(msg, "Invalid gzip data: the member at file offset %llu is gzip but not BGZF (no BC subfield)", at);
        if (size < 12 + xlen + 8) return wg_plan_refuse(msg, "Invalid gzip data: BGZF member at file offset %llu: BSIZE %lld is less than its header and trailer", at, (long long)size - 1);
        if (size > rem) break;
        const uint8_t* t = h + size - 4;
        const uint32_t isize = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        if (isize > WG_BGZF_MAX_ISIZE) return wg_plan_refuse(msg, "Invalid gzip data: BGZF member at file offset %llu: ISIZE %u > 65536", at, isize);
        wg_bgzf_member m;
        m.in_off = (uint64_t)(pos + 12 + xlen); m.in_len = (uint32_t)(size - 12 - xlen - 8); m.isize = isize; m.out_off = out; m.file_off = at;
        members.push_back(m);
        out += isize;
        pos += size;
    }
    *consumed = pos;
    return WGBSSEG_OK;
}

struct BgzfPlan {
    std::vector<wg_bgzf_member> members;   // every complete member of the call
    int64_t consumed = 0;                  // the bytes they take
    int64_t n_dev = 0;                     // members[0 .. n_dev) go to the device (out_off counts from the front of the text buffer, behind the carry)
    int64_t comp_bytes = 0;                // they lie in bytes[0 .. comp_bytes)
    int64_t carry_in = 0;                  // the old carry: the front of the text buffer
    int64_t text_cap = 0;                  // carry_in + the text of the device's members
    int64_t n_text = 0;                    // the chunk the engine's kernels read: complete lines only (0: nothing to launch)
    std::string carry;                     // the new carry
};

inline int plan_bgzf(const uint8_t* bytes, int64_t n, uint64_t file_base, const std::string& carry_old, BgzfPlan& p, std::string& msg)
{
    p = BgzfPlan();
    const int rc = bgzf_walk(bytes, n, file_base, p.members, &p.consumed, msg);
    if (rc != WGBSSEG_OK) return rc;
    p.carry_in = (int64_t)carry_old.size();
    const int64_t M = (int64_t)p.members.size();
    std::vector<uint8_t> buf(WG_BGZF_MAX_ISIZE);
    std::string tail;
    int64_t j = M - 1, cut = -1;
    for (; j >= 0; j--) {
        const wg_bgzf_member& m = p.members[(size_t)j];
        const int why = inflate_member_host(bytes + m.in_off, m.in_len, buf.data(), m.isize);
        if (why != WG_INF_OK) return wg_inflate_refuse(msg, (unsigned long long)m.file_off, why);
        for (int64_t q = (int64_t)m.isize - 1; q >= 0; q--)
            if (buf[(size_t)q] == '\n') { cut = q + 1; break; }
        if (cut >= 0) { tail.insert(0, reinterpret_cast<const char*>(buf.data()) + cut, (size_t)(m.isize - cut)); break; }
        tail.insert(0, reinterpret_cast<const char*>(buf.data()), (size_t)m.isize);
    }
    if (j < 0) { p.carry = carry_old + tail; return WGBSSEG_OK; }      // no newline in the whole call
    p.n_dev = j + 1;
    const wg_bgzf_member& last = p.members[(size_t)j];
    p.comp_bytes = (int64_t)(last.in_off + last.in_len + 8);
    for (int64_t i = 0; i < p.n_dev; i++) p.members[(size_t)i].out_off += (uint64_t)p.carry_in;
    p.text_cap = (int64_t)(last.out_off + last.isize);
    p.n_text = (int64_t)last.out_off + cut;
    p.carry = std::move(tail);
    return WGBSSEG_OK;
}
