// bed2beta_plan.h — the host plan of `wgbstools bed2beta`'s engine (wgbsseg_bedbeta): the checks of the chromosome table and of the loci
// with their messages, the chromosomes in the byte order of their names — the arena, offsets and site ranges that wg_bb_find_chrom
// (bed2beta_core.h) searches —, the flags, the limit on the bytes of one file, and the text of every refusal of a line by its reason
// code.  No HIP here (like mask_plan.h): g++ compiles it alone, tests/native/bed2beta_host.cpp hands it to the tests.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>
#include "block_plan.h"                // wg_plan_refuse
#include "view_core.h"                 // wg_view_cmp_bytes: the byte order of names, a prefix first
#include "bed2beta_core.h"

#define WG_BB_MAX_CHROMS 65535
#define WG_BB_UNPACK_SITES 8           // k_bedbeta_unpack: sites per thread (eight words in, one 16-byte store out)

struct BedBetaPlan {
    int32_t n = 0;                     // chromosomes
    int64_t n_sites = 0;
    int64_t n_words = 0;               // the table: n_sites rounded up to a multiple of WG_BB_UNPACK_SITES
    std::vector<uint32_t> off;         // n + 1: rank r's name is arena[off[r], off[r + 1])
    std::vector<int32_t> lo, hi;       // its sites [lo[r], hi[r])
    std::vector<int32_t> order;        // the caller's index of rank r
    std::string arena;
    wg_bb_chroms view() const { return {arena.data(), off.data(), lo.data(), hi.data(), n}; }
    // one upload: off | lo | hi | arena
    size_t upload_bytes() const { return ((size_t)n + 1) * 4 + (size_t)n * 8 + arena.size(); }
    void upload_to(char* dst) const
    {
        memcpy(dst, off.data(), ((size_t)n + 1) * 4);
        memcpy(dst + ((size_t)n + 1) * 4, lo.data(), (size_t)n * 4);
        memcpy(dst + ((size_t)n + 1) * 4 + (size_t)n * 4, hi.data(), (size_t)n * 4);
        memcpy(dst + ((size_t)n + 1) * 4 + (size_t)n * 8, arena.data(), arena.size());
    }
    wg_bb_chroms view_at(const char* base) const
    {
        const uint32_t* o = reinterpret_cast<const uint32_t*>(base);
        const int32_t* l = reinterpret_cast<const int32_t*>(base + ((size_t)n + 1) * 4);
        return {base + ((size_t)n + 1) * 4 + (size_t)n * 8, o, l, l + n, n};
    }
};

inline int plan_bedbeta_flags(int32_t flags, std::string& msg)
{
    if (flags & ~WG_BB_FLAGS_ALL) return wg_plan_refuse(msg, "bedbeta: unknown flags %d (ADD_ONE = 1, HEADER = 2)", (int)flags);
    return WGBSSEG_OK;
}

// chromosome k: the name chrom_names[k], the sites [chrom_lo[k], chrom_hi[k]) of loci[0, n_sites) (0-based; an empty range is allowed)
inline int plan_bedbeta(const uint32_t* loci, int64_t n_sites, const char* const* chrom_names, const int64_t* chrom_lo, const int64_t* chrom_hi,
                        int32_t n_chroms, int32_t flags, BedBetaPlan& p, std::string& msg)
{
    p = BedBetaPlan();
    if (n_sites < 1 || n_sites > 0x7fffffffLL) return wg_plan_refuse(msg, "bedbeta: %lld sites (1 .. 2^31 - 1)", (long long)n_sites);
    if (n_chroms < 1 || n_chroms > WG_BB_MAX_CHROMS) return wg_plan_refuse(msg, "bedbeta: %d chromosomes (1 .. %d)", (int)n_chroms, WG_BB_MAX_CHROMS);
    if (!loci || !chrom_names || !chrom_lo || !chrom_hi) return wg_plan_refuse(msg, "bad arguments to bedbeta_create");
    const int rc = plan_bedbeta_flags(flags, msg);
    if (rc != WGBSSEG_OK) return rc;
    std::vector<size_t> len((size_t)n_chroms);
    for (int32_t k = 0; k < n_chroms; k++) {
        const char* s = chrom_names[k];
        if (!s || !*s) return wg_plan_refuse(msg, "bedbeta: chromosome %d has an empty name", (int)k);
        len[(size_t)k] = strlen(s);
        if (memchr(s, '\t', len[(size_t)k]) || memchr(s, '\n', len[(size_t)k])) return wg_plan_refuse(msg, "bedbeta: the name of chromosome %d holds a tab or a newline", (int)k);
        if (chrom_lo[k] < 0 || chrom_hi[k] < chrom_lo[k] || chrom_hi[k] > n_sites)
            return wg_plan_refuse(msg, "bedbeta: chromosome %d (%s) has the sites [%lld, %lld) (inside [0, %lld))", (int)k, s, (long long)chrom_lo[k], (long long)chrom_hi[k], (long long)n_sites);
    }
    p.order.resize((size_t)n_chroms);
    std::iota(p.order.begin(), p.order.end(), 0);
    const auto cmp = [&](int32_t a, int32_t b) {
        return wg_view_cmp_bytes(chrom_names[a], (uint32_t)len[(size_t)a], chrom_names[b], (uint32_t)len[(size_t)b]);
    };
    std::sort(p.order.begin(), p.order.end(), [&](int32_t a, int32_t b) { const int d = cmp(a, b); return d ? d < 0 : a < b; });
    for (int32_t r = 1; r < n_chroms; r++)
        if (cmp(p.order[(size_t)r - 1], p.order[(size_t)r]) == 0)
            return wg_plan_refuse(msg, "bedbeta: chromosomes %d and %d have the same name (%s)", (int)p.order[(size_t)r - 1], (int)p.order[(size_t)r], chrom_names[p.order[(size_t)r]]);
    {   // the ranges are disjoint: in order of their first site, each ends at or before the next one's first
        std::vector<int32_t> by_lo;
        for (int32_t k = 0; k < n_chroms; k++)
            if (chrom_hi[k] > chrom_lo[k]) by_lo.push_back(k);
        std::sort(by_lo.begin(), by_lo.end(), [&](int32_t a, int32_t b) { return chrom_lo[a] != chrom_lo[b] ? chrom_lo[a] < chrom_lo[b] : a < b; });
        for (size_t i = 1; i < by_lo.size(); i++)
            if (chrom_hi[by_lo[i - 1]] > chrom_lo[by_lo[i]])
                return wg_plan_refuse(msg, "bedbeta: the sites of chromosomes %d and %d overlap", (int)std::min(by_lo[i - 1], by_lo[i]), (int)std::max(by_lo[i - 1], by_lo[i]));
    }
    for (int32_t k = 0; k < n_chroms; k++)
        for (int64_t i = chrom_lo[k] + 1; i < chrom_hi[k]; i++)
            if (loci[i] <= loci[i - 1])
                return wg_plan_refuse(msg, "bedbeta: the loci of chromosome %d (%s) do not ascend at site %lld (%u after %u)", (int)k, chrom_names[k], (long long)i,
                                      (unsigned)loci[i], (unsigned)loci[i - 1]);
    p.n = n_chroms;
    p.n_sites = n_sites;
    p.n_words = (n_sites + WG_BB_UNPACK_SITES - 1) / WG_BB_UNPACK_SITES * WG_BB_UNPACK_SITES;
    p.off.resize((size_t)n_chroms + 1);
    p.lo.resize((size_t)n_chroms); p.hi.resize((size_t)n_chroms);
    for (int32_t r = 0; r < n_chroms; r++) {
        const int32_t k = p.order[(size_t)r];
        p.off[(size_t)r] = (uint32_t)p.arena.size();
        p.arena.append(chrom_names[k], len[(size_t)k]);
        p.lo[(size_t)r] = (int32_t)chrom_lo[k]; p.hi[(size_t)r] = (int32_t)chrom_hi[k];
    }
    p.off[(size_t)n_chroms] = (uint32_t)p.arena.size();
    return WGBSSEG_OK;
}

// a chunk of n_bytes behind `fed` bytes of the file: every line's offset must stay below 2^47
inline int plan_bedbeta_chunk(unsigned long long fed, int64_t n_bytes, std::string& msg)
{
    if (fed + (unsigned long long)n_bytes > WG_BB_MAX_FED) return wg_plan_refuse(msg, "bedbeta_feed: more than 2^47 bytes of text in one file");
    return WGBSSEG_OK;
}

// the report word of the scan: (byte offset of the lowest refused line << 8) | its reason; ~0: none
inline unsigned long long wg_bb_report(unsigned long long off, int why) { return (off << 8) | (unsigned long long)why; }

// finish(): the refusal of the line the report word names; false (msg untouched) when there is none
inline bool wg_bb_refusal(unsigned long long report, std::string& msg)
{
    if (report == ~0ULL) return false;
    const unsigned long long off = report >> 8;
    const char* what = "is malformed";
    switch ((int)(report & 0xff)) {
    case WG_BB_FEW_FIELDS: what = "has fewer than five tab-separated fields"; break;
    case WG_BB_NOT_NUMBER: what = "has a start, #meth or #total that is not 1 to 18 decimal digits and nothing else"; break;
    case WG_BB_TOTAL_RANGE: what = "has a #total above 2^31 - 1"; break;
    case WG_BB_METH_GT_TOTAL: what = "has #meth above #total"; break;
    }
    (void)wg_plan_refuse(msg, "failed in bed2beta: the line at byte offset %llu of the input %s", off, what);
    return true;
}
