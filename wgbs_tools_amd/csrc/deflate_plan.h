// deflate_plan.h — the host plan of text that becomes BGZF (wgbsseg_bgzf_deflate, wgbsseg_beta2bed_bgzf, wgbsseg_patview_finish): the cut into members, the
// slot pitch of the member buffer k_bgzf_deflate writes and k_bgzf_pack reads, the bound on the bytes that come out, the end-of-file
// member, and the argument checks with their messages.  No HIP here: g++ compiles it alone, tests/native/deflate_host.cpp hands it to the
// tests.
//
// The cut: n bytes of text are members of WG_DEF_MEMBER (65280) bytes, the last one shorter; member i is text[65280 i ..).  No table is
// needed for that, the kernel derives a member's text from its number.  A member's slot has room for its largest form (the stored one,
// 65311 bytes) and for the 16-byte reads of the pack pass behind it.
#pragma once
#include <cstdint>
#include <string>
#include "block_plan.h"
#include "deflate_core.h"

#define WG_DEF_PITCH 65344               // bytes per member slot: >= 65311 + 20, a multiple of 64

static_assert(WG_DEF_STORED_MAX <= 65536, "BSIZE holds a member's size - 1 in 16 bits");
static_assert(WG_DEF_PITCH >= WG_DEF_STORED_MAX + 20 && WG_DEF_PITCH % 64 == 0, "a slot holds the largest member and what k_bgzf_pack reads behind it");

// the member that ends a BGZF file (the SAM specification, 4.1.2)
static const uint8_t WG_BGZF_EOF[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

inline int64_t wg_deflate_members(int64_t n) { return (n + WG_DEF_MEMBER - 1) / WG_DEF_MEMBER; }

// text bytes of member i of n bytes
inline uint32_t wg_deflate_member_len(int64_t n, int64_t i)
{
    const int64_t left = n - i * WG_DEF_MEMBER;
    return (uint32_t)(left < 0 ? 0 : left < WG_DEF_MEMBER ? left : WG_DEF_MEMBER);
}

// the most bytes n bytes of text can become, the end-of-file member included: every member stored
inline int64_t wg_deflate_bound(int64_t n)
{
    return n + wg_deflate_members(n) * (WG_DEF_HEAD + 5 + WG_DEF_TAIL) + (int64_t)sizeof(WG_BGZF_EOF);
}

struct DeflatePlan {
    int64_t n = 0;                         // bytes of text
    int64_t members = 0;
    int64_t slot_bytes = 0;                // members * WG_DEF_PITCH
    int64_t bound = 0;                     // wg_deflate_bound(n)
    int grid = 0;                          // workgroups of k_bgzf_deflate (waves_per_group members each)
};

// wgbsseg_bgzf_deflate's checks.  The room is asked for in advance, since the size is known only once the device is done.
inline int plan_deflate(const void* text, int64_t n, const void* out, int64_t cap, int waves_per_group, DeflatePlan& p, std::string& msg)
{
    p = DeflatePlan();
    if (n < 0 || cap < 0 || (n && !text) || (cap && !out) || waves_per_group < 1) return wg_plan_refuse(msg, "bad arguments to bgzf_deflate");
    p.n = n;
    p.members = wg_deflate_members(n);
    p.slot_bytes = p.members * WG_DEF_PITCH;
    p.bound = wg_deflate_bound(n);
    if (cap < p.bound) {
        (void)wg_plan_refuse(msg, "bgzf_deflate: room for %lld bytes, %lld bytes of text may need %lld (wgbsseg_bgzf_deflate_bound)", (long long)cap, (long long)n, (long long)p.bound);
        return WGBSSEG_E_CAPACITY;
    }
    const int64_t grid = (p.members + waves_per_group - 1) / waves_per_group;
    if (grid > 0x7fffffff) return wg_plan_refuse(msg, "bgzf_deflate: too much text for one call");
    p.grid = (int)grid;
    return WGBSSEG_OK;
}
