// sam_plan.h — the host plan of `wgbstools bam2pat`'s side of the view engine (wgbsseg_patview_set_sam): the checks of the parameters
// and of the engine's state with their messages, the chromosome table (bed2beta_plan.h's: the same arena, offsets and site ranges, the
// same lookup), what a chunk of L lines needs on the device, and the check of what a chunk adds.  No HIP here (like view_plan.h): g++
// compiles it alone, tests/native/sam_host.cpp hands it to the tests.
#pragma once
#include <cstdint>
#include <string>
#include "bed2beta_plan.h"
#include "view_plan.h"
#include "sam_core.h"

#define WG_SAM_BLOCK 256               // lines (= threads) of one workgroup of the per-line kernels

struct SamPlan {
    BedBetaPlan chroms;
    wg_sam_params par = {};
};

// set_sam(): once, after create() and before the first feed, on a sorting engine without a mask and without labels
inline int plan_sam_state(bool already, bool fed, bool finished, bool masked, bool labelled, int view_flags, std::string& msg)
{
    int rc = WGBSSEG_OK;
    if (already) { (void)wg_plan_refuse(msg, "patview_set_sam: called twice"); rc = WGBSSEG_E_STATE; }
    else if (fed || finished) { (void)wg_plan_refuse(msg, "patview_set_sam: called after the first feed"); rc = WGBSSEG_E_STATE; }
    else if (masked || labelled) { (void)wg_plan_refuse(msg, "patview_set_sam: the engine has %s: SAM text does not go with it", masked ? "a mask" : "labels"); rc = WGBSSEG_E_STATE; }
    else if ((view_flags & WG_VIEW_FLAGS_ALL) != WG_VIEW_SORT) rc = wg_plan_refuse(msg, "patview_set_sam: the engine must be created with WGBSSEG_VIEW_SORT and no other flag (got %d)", view_flags);
    return rc;
}

inline int plan_sam(const uint32_t* loci, int64_t n_sites, const char* const* chrom_names, const int64_t* chrom_lo, const int64_t* chrom_hi, int32_t n_chroms,
                    int32_t paired, int64_t exclude_flags, int64_t include_flags, int32_t mapq, int32_t strand, int32_t clip, int32_t min_cpg, SamPlan& p, std::string& msg)
{
    p = SamPlan();
    if (exclude_flags < 0 || exclude_flags > 0xffff || include_flags < 0 || include_flags > 0xffff)
        return wg_plan_refuse(msg, "patview_set_sam: flags %lld / %lld (0 .. 65535)", (long long)exclude_flags, (long long)include_flags);
    if (mapq < 0 || mapq > 255) return wg_plan_refuse(msg, "patview_set_sam: mapq %d (0 .. 255)", (int)mapq);
    if (strand < WG_SAM_BOTH || strand > WG_SAM_BOTTOM) return wg_plan_refuse(msg, "patview_set_sam: strand %d (0 both, 1 top, 2 bottom)", (int)strand);
    if (clip < 0) return wg_plan_refuse(msg, "patview_set_sam: clip %d (at least 0)", (int)clip);
    if (min_cpg < 0) return wg_plan_refuse(msg, "patview_set_sam: min_cpg %d (at least 0)", (int)min_cpg);
    if (paired != 0 && paired != 1) return wg_plan_refuse(msg, "patview_set_sam: paired %d (0 or 1)", (int)paired);
    const int rc = plan_bedbeta(loci, n_sites, chrom_names, chrom_lo, chrom_hi, n_chroms, 0, p.chroms, msg);
    if (rc != WGBSSEG_OK) return rc;
    p.par = wg_sam_params{(uint32_t)exclude_flags, (uint32_t)include_flags, mapq, paired, strand, clip, min_cpg};
    return WGBSSEG_OK;
}

// A chunk of L lines (L comes home from the line count): the workgroups of the per-line kernels, and the words of the one table they
// share — per workgroup six 64-bit words (k_sam_eval's kept lines, their first place; k_sam_heads' run heads, their first run;
// k_sam_measure's records and arena bytes and the two firsts) and, behind them, the totals.
struct SamChunk {
    int64_t lines = 0, groups = 0;
    int64_t wg_words() const { return 8 * groups + 8; }
};

inline int plan_sam_lines(int64_t n_bytes, int64_t lines, SamChunk& c, std::string& msg)
{
    c = SamChunk();
    if (n_bytes > WG_VIEW_MAX_CHUNK) return wg_plan_refuse(msg, "view: a chunk of %lld bytes (at most %lld)", (long long)n_bytes, WG_VIEW_MAX_CHUNK);
    if (lines < 0 || lines > n_bytes) return wg_plan_refuse(msg, "view: %lld lines in a chunk of %lld bytes", (long long)lines, (long long)n_bytes);
    c.lines = lines;
    c.groups = (lines + WG_SAM_BLOCK - 1) / WG_SAM_BLOCK;
    return WGBSSEG_OK;
}

// what the chunk adds to the record table: refused at 2^31 records, as a chunk of pat text is
inline int plan_sam_records(int64_t n_records, int64_t added, std::string& msg)
{
    if (added < 0 || n_records + added > WG_VIEW_MAX_RECORDS) {
        (void)wg_plan_refuse(msg, "view: more than %lld reads selected", WG_VIEW_MAX_RECORDS);
        return WGBSSEG_E_CAPACITY;
    }
    return WGBSSEG_OK;
}
