// bed_plan.h — the host plan of the per-site BED export (wgbsseg_beta2bed, `wgbstools beta2bed`) and what host and device agree
// on: the workgroup size, the longest line, the staging rule, the slabs, the tables' layouts.  No HIP here (like pair_plan.h and block_plan.h): g++
// compiles it alone, tests/native/bed_host.cpp hands it to the tests and tests/native/san_bed.cpp runs it under the sanitizers.
//
// A line is  name \t loc-1 \t loc+1 \t meth \t cov \n  or, with `mean`,  name \t loc-1 \t loc+1 \t R \n  (R: bed_fmt.h).  loc is a
// uint32, so loc-1 takes at most 10 characters ("-1" for loc 0) and loc+1 at most 10 (4294967296); a count at most 5; R at most
// WG_G3_MAX_LEN = 8: a line is never longer than the name + WG_BED_LINE_TAIL bytes.
//
// THE STAGING RULE (stated here once, used by k_bed_emit through wg_bed_staged): a workgroup of WG_BED_BLOCK sites whose bytes
// — every line times its multiplicity — are at most `stage_bytes` formats them into LDS and copies them out with aligned 16-byte
// stores; one with more (only -L multiplicities get there) writes each copy straight to global memory.  stage_bytes is at
// most WG_BED_STAGE_BYTES, what WG_BED_BLOCK lines of the longest kind take, so without multiplicities every workgroup is staged.
#pragma once
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/wgbsseg.h"
#include "bed_fmt.h"

#define WG_BED_BLOCK 256                       // sites (= threads) of one workgroup
#define WG_BED_MAX_NAME 31                     // longest chromosome name, in bytes
#define WG_BED_NAME_REC 32                     // a name's record on the device: its bytes, zero-padded; byte 31 holds the length
#define WG_BED_LINE_TAIL 35                    // \t 10 \t 10 \t 5 \t 5 \n
#define WG_BED_MAX_LINE (WG_BED_MAX_NAME + WG_BED_LINE_TAIL)
#define WG_BED_STAGE_BYTES (WG_BED_BLOCK * WG_BED_MAX_LINE)      // 16,896
#define WG_BED_LDS_CHROMS 64                   // chromosome tables up to this many entries are read from LDS, longer ones from global memory
#define WG_BED_DEFAULT_SLAB (1 << 20)          // sites per slab: 4096 workgroup totals, which ONE workgroup scans in 16 steps
#define WG_BED_MAX_SLAB (1 << 24)
#define WG_BED_MULT_TOO_MANY 65535             // reserved multiplicity: "more overlapping rows than a uint16 counts"
#define WG_BED_MAX_SLAB_BYTES (1ull << 32)     // a slab's text must stay below this (only multiplicities can reach it)
#define WG_BED_TEXT_SLACK 16                   // what the device's text buffer has beyond the text: k_bed_emit copies out in 16-byte vectors

static_assert(WG_BED_MAX_NAME < WG_BED_NAME_REC, "the record's last byte is the length");
static_assert(WG_BED_LINE_TAIL >= 1 + 10 + 1 + 10 + 1 + WG_G3_MAX_LEN + 1, "the mean line is the shorter one");
static_assert((uint64_t)WG_BED_BLOCK * WG_BED_MAX_LINE * 65534ull < (1ull << 32), "a workgroup's bytes fit its 32-bit scan");
static_assert(WG_BED_MAX_SLAB % WG_BED_BLOCK == 0 && WG_BED_DEFAULT_SLAB <= WG_BED_MAX_SLAB, "slab limits");

// the staging rule
WG_HD bool wg_bed_staged(uint32_t wg_bytes, uint32_t stage_bytes) { return wg_bytes <= stage_bytes; }

// the longest line a chromosome name of name_len bytes can head (bed_plan.h's head comment)
constexpr int64_t wg_bed_line_bound(int64_t name_len) { return name_len + WG_BED_LINE_TAIL; }

inline int wg_bed_refuse(std::string& msg, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    msg = buf;
    return WGBSSEG_E_ARG;
}

struct BedPlan {
    int64_t start0 = 0, end0 = 0;      // the selection, resident sites [start0, end0)
    int64_t slab_sites = 0;            // sites per slab (the last one may hold fewer)
    int64_t n_slabs = 0;
    int32_t stage_bytes = 0;           // the staging rule's threshold
    int32_t max_name = 0;              // the longest chromosome name of the call

    int64_t slab_first(int64_t k) const { return start0 + k * slab_sites; }
    int64_t slab_count(int64_t k) const { const int64_t left = end0 - slab_first(k); return left < slab_sites ? left : slab_sites; }
    static int64_t workgroups(int64_t sites) { return (sites + WG_BED_BLOCK - 1) / WG_BED_BLOCK; }
    // what a slab's text can take without multiplicities: the first size of its two buffers
    int64_t slab_bytes_bound(int64_t k) const { return slab_count(k) * wg_bed_line_bound(max_name); }
};

// Two slabs are in flight, slab k in the buffers and between the events of parity k & 1: this function is the only place that says so.
constexpr int wg_bed_parity(int64_t k) { return (int)(k & 1); }

// The text buffers of a slab whose text has `tot` bytes, of a call whose first slab is bounded by `first_bound` (BedPlan::slab_bytes_bound(0):
// what every slab needs without multiplicities, so no regrowth slab by slab): the page-locked one at home and the device's.
struct BedTextCap { size_t home, device; };
inline BedTextCap wg_bed_text_capacity(uint64_t tot, int64_t first_bound)
{
    const size_t n = tot > (uint64_t)first_bound ? (size_t)tot : (size_t)first_bound;
    return {n, n + WG_BED_TEXT_SLACK};
}

// The workgroup table of a slab of up to max_wgs workgroups, in 64-bit words: k_bed_len's bytes and lines per workgroup, k_bed_scan's
// first byte of every workgroup and, behind them, the slab's two totals (bytes, lines), which travel home together.
struct BedWgTable {
    int64_t bytes, lines, base, tot_bytes, tot_lines, words;
    size_t size() const { return (size_t)words * 8; }
};
constexpr BedWgTable wg_bed_wg_table(int64_t max_wgs) { return {0, max_wgs, 2 * max_wgs, 3 * max_wgs, 3 * max_wgs + 1, 3 * max_wgs + 2}; }

// The chromosome table as the device reads it (wg_bed_args::cum, ::names), for a table wg_bed_plan has accepted: n_chroms cumulative
// counts, then n_chroms records of WG_BED_NAME_REC bytes, the name zero-padded and its length in the last byte.  Byte offsets.
struct BedChromTable { size_t cum, names, size; };
constexpr BedChromTable wg_bed_chrom_table(int32_t n_chroms) { return {0, (size_t)n_chroms * 8, (size_t)n_chroms * (8 + WG_BED_NAME_REC)}; }
inline std::vector<char> wg_bed_pack_chroms(const int64_t* chrom_cum, const char* const* chrom_names, int32_t n_chroms)
{
    const BedChromTable t = wg_bed_chrom_table(n_chroms);
    std::vector<char> tab(t.size, 0);
    memcpy(tab.data() + t.cum, chrom_cum, (size_t)n_chroms * 8);
    for (int32_t i = 0; i < n_chroms; i++) {
        char* rec = tab.data() + t.names + (size_t)i * WG_BED_NAME_REC;
        const size_t len = strlen(chrom_names[i]);
        memcpy(rec, chrom_names[i], len);
        rec[WG_BED_NAME_REC - 1] = (char)len;
    }
    return tab;
}

// The arguments of wgbsseg_beta2bed against n_samples resident rows of n_total sites.  WGBSSEG_OK and a filled plan, or
// WGBSSEG_E_ARG and a message naming the offender.
inline int wg_bed_plan(int32_t sample, int32_t n_samples, int64_t start0, int64_t end0, int64_t n_total, const int64_t* chrom_cum,
                       const char* const* chrom_names, int32_t n_chroms, const wgbsseg_bed_opts* o, BedPlan& p, std::string& msg)
{
    if (!o) return wg_bed_refuse(msg, "beta2bed: opts is NULL");
    if (sample < 0 || sample >= n_samples) return wg_bed_refuse(msg, "beta2bed: sample %d is outside the %d resident samples", (int)sample, (int)n_samples);
    if (start0 < 0 || end0 < start0 || end0 > n_total)
        return wg_bed_refuse(msg, "beta2bed: sites [%lld, %lld) are outside the %lld resident sites or reversed", (long long)start0, (long long)end0, (long long)n_total);
    if (o->min_cov < 1) return wg_bed_refuse(msg, "beta2bed: min_cov = %d must be at least 1", (int)o->min_cov);
    if (o->stage_bytes < 0 || o->stage_bytes > WG_BED_STAGE_BYTES)
        return wg_bed_refuse(msg, "beta2bed: stage_bytes = %d is outside 0 .. %d (0: the default, all of it)", (int)o->stage_bytes, WG_BED_STAGE_BYTES);
    if (o->slab_sites < 0 || o->slab_sites > WG_BED_MAX_SLAB)
        return wg_bed_refuse(msg, "beta2bed: slab_sites = %lld is outside 0 .. %d (0: the default, %d)", (long long)o->slab_sites, WG_BED_MAX_SLAB, WG_BED_DEFAULT_SLAB);
    if (n_chroms < 1 || !chrom_cum || !chrom_names) return wg_bed_refuse(msg, "beta2bed: the chromosome table is empty or NULL");
    int max_name = 0;
    for (int32_t i = 0; i < n_chroms; i++) {
        if (chrom_cum[i] < (i ? chrom_cum[i - 1] : 0)) return wg_bed_refuse(msg, "beta2bed: chrom_cum[%d] = %lld descends", (int)i, (long long)chrom_cum[i]);
        if (!chrom_names[i] || !chrom_names[i][0]) return wg_bed_refuse(msg, "beta2bed: chromosome %d has no name", (int)i);
        const size_t len = strlen(chrom_names[i]);
        if (len > WG_BED_MAX_NAME)
            return wg_bed_refuse(msg, "beta2bed: the name of chromosome %d (%.40s...) has %lld bytes, at most %d are supported", (int)i, chrom_names[i], (long long)len, WG_BED_MAX_NAME);
        if ((int)len > max_name) max_name = (int)len;
    }
    if (chrom_cum[n_chroms - 1] != n_total)
        return wg_bed_refuse(msg, "beta2bed: chrom_cum ends at %lld, the resident rows have %lld sites", (long long)chrom_cum[n_chroms - 1], (long long)n_total);
    p.start0 = start0;
    p.end0 = end0;
    p.slab_sites = o->slab_sites ? o->slab_sites : WG_BED_DEFAULT_SLAB;
    p.n_slabs = (end0 - start0 + p.slab_sites - 1) / p.slab_sites;
    p.stage_bytes = o->stage_bytes ? o->stage_bytes : WG_BED_STAGE_BYTES;
    p.max_name = max_name;
    return WGBSSEG_OK;
}

// the multiplicities of the selection: none may be the reserved value
inline int wg_bed_check_mult(const uint16_t* mult, int64_t n, int64_t start0, std::string& msg)
{
    for (int64_t i = 0; mult && i < n; i++)
        if (mult[i] == WG_BED_MULT_TOO_MANY)
            return wg_bed_refuse(msg, "beta2bed: site %lld has multiplicity %d, the value reserved for more overlapping rows than can be counted", (long long)(start0 + i), WG_BED_MULT_TOO_MANY);
    return WGBSSEG_OK;
}

// a slab whose text has `bytes` bytes: WGBSSEG_E_CAPACITY from 4 GiB on
inline int wg_bed_check_slab_bytes(uint64_t bytes, int64_t slab, int64_t slab_sites, std::string& msg)
{
    if (bytes < WG_BED_MAX_SLAB_BYTES) return WGBSSEG_OK;
    wg_bed_refuse(msg, "beta2bed: slab %lld (%lld sites) would write %llu bytes, 4 GiB or more: pass a smaller slab_sites", (long long)slab, (long long)slab_sites, (unsigned long long)bytes);
    return WGBSSEG_E_CAPACITY;
}
