// tests/native/bed2beta_run.h — the whole of `wgbstools bed2beta` on the host by the functions the kernels call (bed2beta_core.h through
// bed2beta_plan.h): every non-empty line of the text through wg_bb_line_to_site, the table of one word per site lowered to the minimum,
// the lowest refused line as the report word, the four counters, then the table unpacked with wg_bb_pair.  Shared by
// bed2beta_host.cpp (the tests' library) and san_bed2beta.cpp (the stand-alone program for the sanitizers).  The table and the result are
// arrays of exactly their size.
#pragma once
#include <cstdlib>
#include "../../wgbs_tools_amd/csrc/bed2beta_plan.h"

// out: n_sites * 2 bytes; stats[6] as wgbsseg_bedbeta_finish's; *report: the report word (~0: no line refused; out and stats are then valid)
inline void bb_run_host(const char* text, int64_t n, const BedBetaPlan& plan, const uint32_t* loci, int32_t flags, uint8_t* out, int64_t* stats,
                        unsigned long long* report)
{
    const wg_bb_host_text T = {text};
    const wg_bb_chroms chroms = plan.view();
    uint64_t* table = static_cast<uint64_t*>(malloc((size_t)plan.n_sites * 8));
    for (int64_t i = 0; i < plan.n_sites; i++) table[i] = WG_BB_EMPTY;
    unsigned long long bad = ~0ULL;
    int64_t cnt[4] = {0, 0, 0, 0};
    int32_t hint = -1;
    for (int64_t p = 0; p < n;) {
        int64_t e = p;
        while (e < n && text[e] != '\n') e++;
        if (e > p && !((flags & WG_BB_HEADER) && p == 0)) {
            cnt[0]++;
            int64_t site = -1;
            uint64_t word = 0;
            const int what = wg_bb_line_to_site(T, p, n, (uint64_t)p, chroms, loci, (flags & WG_BB_ADD_ONE) ? 1 : 0, hint, site, word);
            if (what < 0) { const unsigned long long r = wg_bb_report((unsigned long long)p, -what); if (r < bad) bad = r; }
            else {
                if (what == WG_BB_MATCHED && word < table[site]) table[site] = word;
                cnt[1 + what]++;
            }
        }
        p = e + 1;
    }
    int64_t set = 0;
    for (int64_t i = 0; i < plan.n_sites; i++) {
        const uint32_t pr = wg_bb_pair(table[i]);
        out[2 * i] = (uint8_t)(pr & 0xffu); out[2 * i + 1] = (uint8_t)(pr >> 8);
        set += table[i] != WG_BB_EMPTY;
    }
    free(table);
    stats[0] = cnt[0]; stats[1] = cnt[1]; stats[2] = cnt[2]; stats[3] = cnt[3]; stats[4] = cnt[1] - set; stats[5] = set;
    *report = bad;
}
