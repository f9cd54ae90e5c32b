// bimodal_plan.h — what host and device agree on for `wgbstools test_bimodal` (the state and per-block records of
// bimodal_kernels.h, the columns a wavefront keeps in LDS, the bytes of scratch per column beyond) and what the host decides
// between two chunks: which blocks retire, which reads may go, how large a chunk's tables can get, where the wide blocks'
// scratch lies.  No HIP here (like block_plan.h, whose wg_plan_refuse it uses): g++ compiles it alone,
// tests/native/patplan_host.cpp hands it to the tests.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>
#include <vector>
#include "block_plan.h"

#define WG_BIM_LDS_COLS 256           // LDS path: 256 columns x WG_BIM_COL_BYTES = 12 KiB per wavefront (13 wavefronts per CU by LDS)
#define WG_BIM_COL_BYTES 48           // k_bim_em's tables per column: four log2 values (doubles) and four counts (uint32), in LDS or in scratch
#define WG_BIM_MAX_ITERS 100000       // the reference has no cap: a strictly rising sequence over finitely many assignments ends
#define WG_BIM_CTX 150                // MAX_PAT_LEN (utils_wgbs.py:38): how far before s1 the reference's tabix query starts
#define WG_BIM_NONE ((long long)INT64_MIN)

// device-side state of a bimodal run (one per accumulator)
struct wg_bim_state {
    long long R, W;                   // live reads / pattern words in the current table
    long long R0;                     // R before the last chunk was appended
    long long last_start;             // start of the last read seen (WG_BIM_NONE: none yet)
    long long head, whead;            // reads / words dropped by the last k_bim_drop_find
    unsigned long long bad, neg, desc;      // lowest byte offsets: malformed line, negative count, descending start (~0: none)
    unsigned long long em_cap;        // a block that reached WG_BIM_MAX_ITERS (its index + 1; 0: none)
};

// per retired block, from k_bim_gather
struct wg_bim_meta {
    long long ra, rb;                 // table rows with start in [max(1, s1 - 150), s2 - 1]
    long long first_ind, ncols, rows, lines;
};

// Upper bounds on the good lines of a chunk of n_bytes and on their pattern words; they size both read tables and the chunk's
// line offsets.  A good line has >= 6 bytes (three tabs, a newline, a digit each of site and count); a pattern of L sites takes
// ceil(L / 16) <= L / 16 + 1 words and the patterns of a chunk have at most n_bytes sites together.
struct BimodalChunkBound {
    size_t lines, words;
    explicit BimodalChunkBound(int64_t n_bytes) : lines((size_t)n_bytes / 6 + 1), words((size_t)n_bytes / 16 + lines + 1) {}
};

struct BimodalPlan {
    int64_t n_blocks = 0;
    int lds_cols = WG_BIM_LDS_COLS;               // columns k_bim_em keeps in LDS (the caller's wish, at most WG_BIM_LDS_COLS)
    std::vector<int32_t> s1, s2, by_end;          // the blocks as given; by_end: block indexes in (endCpG, file) order
    std::vector<int64_t> lo_after;                // lo_after[p]: min over by_end[p..] of max(1, s1 - WG_BIM_CTX) (INT64_MAX past the end)

    // by_end[pending .. retire_upto) are the blocks whose reads have all been seen: a read starting at or after endCpG has come
    int64_t retire_upto(int64_t pending, long long last_start) const
    {
        int64_t p1 = pending;
        if (last_start != WG_BIM_NONE)
            while (p1 < n_blocks && (long long)s2[(size_t)by_end[(size_t)p1]] <= last_start) p1++;
        return p1;
    }
    // reads starting below this can reach no block of by_end[pending ..] (nothing pending: every read, starts being below 2^31)
    long long drop_below(int64_t pending) const
    {
        const int64_t lo = lo_after[(size_t)pending];
        return lo == INT64_MAX ? (long long)INT32_MAX + 1 : (long long)lo;
    }
};

// Checks the blocks and orders them by endCpG.  max_lds_cols < 0: the default.
inline int plan_bimodal(const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, int32_t min_len, int32_t max_lds_cols, BimodalPlan& p,
                        std::string& msg)
{
    p = BimodalPlan();
    if (n_blocks < 1 || n_blocks > 0x7fffffffLL || !start_cpg || !end_cpg) return wg_plan_refuse(msg, "test_bimodal: no blocks");
    if (min_len < 1) return wg_plan_refuse(msg, "test_bimodal: min_len %d < 1", (int)min_len);
    for (int64_t j = 0; j < n_blocks; j++) {
        const int64_t a = start_cpg[j], e = end_cpg[j];
        if (a < 1 || e <= a || e > 0x7fffffffLL)
            return wg_plan_refuse(msg, "test_bimodal: block %lld has startCpG %lld, endCpG %lld (1 <= startCpG < endCpG < 2^31)", (long long)j + 1, (long long)a, (long long)e);
    }
    p.n_blocks = n_blocks;
    p.lds_cols = max_lds_cols < 0 ? WG_BIM_LDS_COLS : std::min<int32_t>(max_lds_cols, WG_BIM_LDS_COLS);
    const size_t nb = (size_t)n_blocks;
    p.s1.resize(nb); p.s2.resize(nb); p.by_end.resize(nb); p.lo_after.assign(nb + 1, INT64_MAX);
    for (size_t j = 0; j < nb; j++) { p.s1[j] = (int32_t)start_cpg[j]; p.s2[j] = (int32_t)end_cpg[j]; p.by_end[j] = (int32_t)j; }
    std::stable_sort(p.by_end.begin(), p.by_end.end(), [&](int32_t x, int32_t y) { return p.s2[(size_t)x] < p.s2[(size_t)y]; });
    for (size_t q = nb; q-- > 0;) p.lo_after[q] = std::min<int64_t>(p.lo_after[q + 1], std::max<int64_t>(1, (int64_t)p.s1[(size_t)p.by_end[q]] - WG_BIM_CTX));
    return WGBSSEG_OK;
}

// Where k_bim_em finds the scratch of each of the n blocks being retired (m: k_bim_gather's records, ids: their rows in by_end):
// off[g] = the byte offset of a block with rows and more than lds_cols columns, 0 for the others; used = the bytes in all.
inline int wg_bim_scratch_layout(const wg_bim_meta* m, const int32_t* ids, int64_t n, int lds_cols, long long* off, size_t& used, std::string& msg)
{
    used = 0;
    for (int64_t g = 0; g < n; g++) {
        if (m[g].rows > 0x7fffffffLL) {
            wg_plan_refuse(msg, "test_bimodal: block %lld (row %d of the blocks) has %lld rows: more than 2^31 - 1", (long long)g, (int)ids[g] + 1, m[g].rows);
            return WGBSSEG_E_CAPACITY;
        }
        off[g] = 0;
        if (m[g].rows > 0 && m[g].ncols > lds_cols) { off[g] = (long long)used; used += (size_t)m[g].ncols * WG_BIM_COL_BYTES; }
    }
    return WGBSSEG_OK;
}
