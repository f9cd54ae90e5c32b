// tests/native/sam_run.h — `wgbstools bam2pat` on the host by the functions the kernels call (csrc/sam_core.h, the chromosome table of
// csrc/sam_plan.h): the lines one after the other, every line's wg_sam_read, the runs of equal names cut into pairs by their places, every
// pair through wg_sam_merge, the results sorted and counted.  Shared by sam_host.cpp (the tests' library) and san_bam2pat.cpp (the
// stand-alone program of the sanitizer run).  Every array has exactly its size.
#pragma once
#include <map>
#include <string>
#include <tuple>
#include <vector>
#include "../../wgbs_tools_amd/csrc/sam_plan.h"

// text[0, n) (its last line may lack the newline) -> the collapsed pat text; stats[WG_SAM_COUNTERS]
inline std::string sam_run_host(const char* text, int64_t n, const SamPlan& plan, const uint32_t* loci, int64_t* stats)
{
    std::vector<char> own(text, text + n);                          // exactly n bytes (+ the newline the feed would add)
    if (n && own.back() != '\n') own.push_back('\n');
    const wg_sam_text T = {own.data()};
    const int64_t N = (int64_t)own.size();
    const wg_bb_chroms chroms = plan.chroms.view();
    const wg_sam_params& a = plan.par;
    for (int k = 0; k < WG_SAM_COUNTERS; k++) stats[k] = 0;
    std::vector<wg_sam_read> kept;
    for (int64_t p = 0; p < N;) {
        int64_t e = p;
        while (own[(size_t)e] != '\n') e++;
        if (e > p) {
            const wg_sam_read r = wg_sam_eval(T, p, N, a, chroms, loci);
            stats[WG_SAM_N_LINES]++;
            if (r.state == WG_SAM_HEADER) stats[WG_SAM_N_HEADER]++;
            if (r.state == WG_SAM_FILTERED) stats[WG_SAM_N_FILTERED]++;
            if (r.state == WG_SAM_UNKNOWN) stats[WG_SAM_N_UNKNOWN]++;
            if (r.state == WG_SAM_INVALID) stats[WG_SAM_N_INVALID]++;
            if (r.state == WG_SAM_EMPTY) stats[WG_SAM_N_EMPTY]++;
            if (wg_sam_participates(r.state)) kept.push_back(r);
        }
        p = e + 1;
    }
    std::map<std::tuple<int64_t, std::string, std::string>, int64_t> out;
    const auto pat_of = [&](const wg_sam_read& r) {
        return wg_sam_pat_begin(T, wg_sam_geom_again(T, (int64_t)r.line, N, r.bottom != 0), loci, r.start - 1, (int64_t)a.clip);
    };
    const auto emit = [&](const wg_sam_read& r, int64_t rs, const std::string& pat) {
        if ((int64_t)pat.size() < (int64_t)a.min_cpg) { stats[WG_SAM_N_SHORT]++; return; }
        out[std::make_tuple(rs, pat, std::string(chroms.arena + chroms.off[r.rank], chroms.off[r.rank + 1] - chroms.off[r.rank]))]++;
    };
    const auto single = [&](const wg_sam_read& r) {
        if (r.state != WG_SAM_PAT) return;
        std::string pat(r.plen, '?');
        auto src = pat_of(r);
        for (uint32_t i = 0; i < r.plen; i++) pat[i] = src((int64_t)i);
        emit(r, r.start, pat);
    };
    uint64_t place = 0;
    for (size_t k = 0; k < kept.size(); k++) {
        const wg_sam_read& r = kept[k];
        const bool same_as_before = a.paired && k > 0 && wg_sam_same_read(T, kept[k - 1].line, kept[k - 1].qlen, kept[k - 1].rank, T, r.line, r.qlen, r.rank);
        place = same_as_before ? place + 1 : 0;
        if (!wg_sam_is_first(place)) continue;                      // the second of its pair: done with the first
        const bool mate = a.paired && k + 1 < kept.size() && wg_sam_same_read(T, r.line, r.qlen, r.rank, T, kept[k + 1].line, kept[k + 1].qlen, kept[k + 1].rank);
        if (!mate) {
            if (a.paired) stats[WG_SAM_N_LEFT_SINGLE]++;
            single(r);
            continue;
        }
        const wg_sam_read& s = kept[k + 1];
        stats[WG_SAM_N_PAIRS]++;
        if (r.state == WG_SAM_PAT && s.state == WG_SAM_PAT) {
            std::string span;
            const wg_sam_merged m = wg_sam_merge(r.start, r.plen, pat_of(r), s.start, s.plen, pat_of(s), [&](int64_t, char c) { span.push_back(c); });
            if (m.why == WG_SAM_MERGE_TOO_LONG) stats[WG_SAM_N_TOO_LONG]++;
            else if (m.why == WG_SAM_MERGE_EMPTY) stats[WG_SAM_N_EMPTY]++;
            else emit(r, m.rs, span.substr((size_t)m.first, (size_t)m.len));
        } else {
            single(r);
            single(s);
        }
    }
    std::string res;
    for (const auto& kv : out)
        res += std::get<2>(kv.first) + "\t" + std::to_string(std::get<0>(kv.first)) + "\t" + std::get<1>(kv.first) + "\t" + std::to_string(kv.second) + "\n";
    return res;
}
