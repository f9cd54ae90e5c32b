// tests/native/mask_host.cpp — test shim: the host build of wgbs_tools_amd/csrc/mask_plan.h and of view_core.h's mask (wg_view_mask,
// wg_view_hidden, wg_view_hidden64, the masked cut), exported so that tests/test_mask_pat_cpu.py can compare them with the restatement
// tests/mask_ref.py and read every refusal of the plan.
//   g++ -O2 -std=c++17 -shared -fPIC mask_host.cpp -o libmask_host.so
#include <cstring>
#include <vector>
#include "../../wgbs_tools_amd/csrc/mask_plan.h"

static void put_msg(const std::string& m, char* msg, size_t msglen)
{
    if (msg && msglen) { strncpy(msg, m.c_str(), msglen - 1); msg[msglen - 1] = 0; }
}

// a plan and the bitmap k_view_mask_fill would write from it
struct Mask {
    MaskPlan plan;
    std::vector<uint32_t> words;
    wg_view_mask view() const { return {words.data(), plan.lo, plan.hi}; }
};

extern "C" {

// info = {lo, hi, n_words, n_hidden, n_intervals}; *out: the mask (free it with mask_free), nullptr when refused
int mask_plan(const int64_t* starts, const int64_t* ends, int64_t n, int64_t* info, Mask** out, char* msg, size_t msglen)
{
    Mask* m = new Mask();
    std::string text;
    const int rc = plan_mask(starts, ends, n, m->plan, text);
    put_msg(text, msg, msglen);
    *out = nullptr;
    if (rc != WGBSSEG_OK) { delete m; return rc; }
    const MaskPlan& p = m->plan;
    info[0] = p.lo; info[1] = p.hi; info[2] = p.n_words; info[3] = p.n_hidden; info[4] = p.n_intervals();
    m->words.resize((size_t)p.n_words);
    for (int64_t w = 0; w < p.n_words; w++) m->words[(size_t)w] = wg_mask_word(p.starts.data(), p.ends.data(), p.n_intervals(), p.lo, w);
    *out = m;
    return rc;
}

void mask_free(Mask* m) { delete m; }
void mask_intervals(const Mask* m, int64_t* starts, int64_t* ends)
{
    memcpy(starts, m->plan.starts.data(), m->plan.starts.size() * 8);
    memcpy(ends, m->plan.ends.data(), m->plan.ends.size() * 8);
}
void mask_words(const Mask* m, uint32_t* out) { memcpy(out, m->words.data(), m->words.size() * 4); }
int mask_hidden(const Mask* m, int64_t site) { return wg_view_hidden(m->view(), site) ? 1 : 0; }
uint64_t mask_hidden64(const Mask* m, int64_t site) { return wg_view_hidden64(m->view(), site); }

// the masked cut of the read `rs, pat[0, plen)`: out = {rs', first, len}; masked receives the read's bytes as the mask leaves them
void mask_cut(const Mask* m, int64_t rs, const char* pat, int64_t plen, int64_t s, int64_t e, int32_t flags, int64_t min_len, int64_t* out, char* masked)
{
    const wg_view_mask v = m->view();
    const wg_view_cut c = wg_view_cut_read_masked(rs, plen, [&](int64_t k) { return pat[k]; }, v, s, e, flags, min_len);
    out[0] = c.rs; out[1] = c.first; out[2] = c.len;
    wg_view_window w = {-1, 0};
    for (int64_t i = 0; i < plen; i++) masked[i] = wg_view_masked_byte(v, w, rs, i, [&](int64_t k) { return pat[k]; });
}

// n reads, each against its own set of hidden sites: read i is `rs[i], pats[off[i], off[i + 1])`, bit k of subset[i] hides site first + k
// (the bitmap's lo at `lo`); out[3 i ..] = {rs', first, len} of its masked cut
void mask_cut_many(int64_t n, const int64_t* rs, const int64_t* off, const char* pats, const uint32_t* subset, int64_t first, int window, int64_t lo,
                   int32_t flags, int64_t s, int64_t e, int64_t* out)
{
    const int64_t hi = first + window > lo ? first + window : lo + 1;
    std::vector<uint32_t> words((size_t)wg_view_mask_words(lo, hi));
    for (int64_t i = 0; i < n; i++) {
        std::fill(words.begin(), words.end(), 0u);
        for (int k = 0; k < window; k++)
            if ((subset[i] >> k & 1u) && first + k >= lo) words[(size_t)((first + k - lo) >> 5)] |= 1u << ((first + k - lo) & 31);
        const wg_view_mask v = {words.data(), lo, hi};
        const char* pat = pats + off[i];
        const wg_view_cut c = wg_view_cut_read_masked(rs[i], off[i + 1] - off[i], [&](int64_t k) { return pat[k]; }, v, s, e, flags, 1);
        out[3 * i] = c.rs; out[3 * i + 1] = c.first; out[3 * i + 2] = c.len;
    }
}

// The exhaustive sweep: every pattern over {C, T, .} of length 1 .. max_len at every start in [first, first + window), against every
// subset of hidden sites of that window (bit k of `subset`: site first + k, the bitmap's lo at `lo`), for the flags given.  The sweep
// holds the masked cut against the cut of the read masked byte by byte with wg_view_hidden — two routes through the header — and
// returns the number of reads whose two cuts differ (0), counting the reads into *n_reads.  A read's cut depends on the hidden sites
// among its own only: tests/test_mask_pat_cpu.py holds mask_cut_many against tests/mask_ref.py for every pattern, every start and every
// subset of the read's own sites, so the two together cover the sweep against the restatement.
int64_t mask_sweep(int64_t first, int window, int max_len, int64_t lo, int32_t flags, int64_t s, int64_t e, int64_t* n_reads)
{
    int64_t differ = 0, reads = 0;
    const int64_t hi = first + window > lo ? first + window : lo + 1;
    std::vector<uint32_t> words((size_t)wg_view_mask_words(lo, hi));
    for (uint32_t subset = 0; subset < (1u << window); subset++) {
        std::fill(words.begin(), words.end(), 0u);
        for (int k = 0; k < window; k++)
            if ((subset >> k & 1u) && first + k >= lo) words[(size_t)((first + k - lo) >> 5)] |= 1u << ((first + k - lo) & 31);
        const wg_view_mask v = {words.data(), lo, hi};
        for (int len = 1; len <= max_len; len++) {
            int64_t combos = 1;
            for (int k = 0; k < len; k++) combos *= 3;
            for (int64_t code = 0; code < combos; code++) {
                char pat[16], byway[16];
                int64_t c = code;
                for (int k = 0; k < len; k++, c /= 3) pat[k] = "CT."[c % 3];
                for (int64_t rs = first; rs < first + window; rs++) {
                    for (int k = 0; k < len; k++) byway[k] = wg_view_hidden(v, rs + k) ? '.' : pat[k];
                    const wg_view_cut a = wg_view_cut_read_masked(rs, len, [&](int64_t k) { return pat[k]; }, v, s, e, flags, 1);
                    const wg_view_cut b = wg_view_cut_read(rs, len, [&](int64_t k) { return byway[k]; }, s, e, flags, 1);
                    reads++;
                    if (a.len != b.len || (a.len && (a.rs != b.rs || a.first != b.first))) differ++;
                }
            }
        }
    }
    *n_reads = reads;
    return differ;
}

}  // extern "C"
