// tests/native/sam_host.cpp — test shim: the host build of wgbs_tools_amd/csrc/sam_plan.h and sam_core.h, exported so that
// tests/test_bam2pat_cpu.py can read every refusal of the plan and hold the field split, the numbers, the filter, the CIGAR check and
// cursor, a line's pat, the mate rule and the merge against tests/bam2pat_ref.py, and run whole files through the functions the kernels
// call (sam_run.h).
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC sam_host.cpp -o libsam_host.so
#include <cstring>
#include "sam_run.h"

static void put_msg(const std::string& m, char* msg, size_t msglen)
{
    if (msg && msglen) { strncpy(msg, m.c_str(), msglen - 1); msg[msglen - 1] = 0; }
}

extern "C" {

// *out: the plan (free it with sam_free), nullptr when refused
int sam_plan(const uint32_t* loci, int64_t n_sites, const char* const* names, const int64_t* lo, const int64_t* hi, int32_t n_chroms, int32_t paired,
             int64_t exclude, int64_t include, int32_t mapq, int32_t strand, int32_t clip, int32_t min_cpg, SamPlan** out, char* msg, size_t msglen)
{
    SamPlan* p = new SamPlan();
    std::string text;
    const int rc = plan_sam(loci, n_sites, names, lo, hi, n_chroms, paired, exclude, include, mapq, strand, clip, min_cpg, *p, text);
    put_msg(text, msg, msglen);
    *out = nullptr;
    if (rc != WGBSSEG_OK) { delete p; return rc; }
    *out = p;
    return rc;
}

void sam_free(SamPlan* p) { delete p; }

int sam_state(int already, int fed, int finished, int masked, int labelled, int flags, char* msg, size_t msglen)
{
    std::string text;
    const int rc = plan_sam_state(already != 0, fed != 0, finished != 0, masked != 0, labelled != 0, flags, text);
    put_msg(text, msg, msglen);
    return rc;
}

// out = {lines, groups, words}
int sam_lines(int64_t n_bytes, int64_t lines, int64_t* out, char* msg, size_t msglen)
{
    SamChunk c;
    std::string text;
    const int rc = plan_sam_lines(n_bytes, lines, c, text);
    put_msg(text, msg, msglen);
    out[0] = c.lines; out[1] = c.groups; out[2] = c.wg_words();
    return rc;
}

int sam_records(int64_t n_records, int64_t added, char* msg, size_t msglen)
{
    std::string text;
    const int rc = plan_sam_records(n_records, added, text);
    put_msg(text, msg, msglen);
    return rc;
}

// the tokens of the line at byte p; bounds[2 k], bounds[2 k + 1]: field k < min(tokens, 10), relative to p
int sam_split(const char* text, int64_t n, int64_t p, uint32_t* bounds)
{
    const wg_sam_text T = {text};
    uint32_t fb[10] = {0}, fe[10] = {0};
    const int nf = wg_sam_split(T, p, n, fb, fe);
    for (int k = 0; k < 10; k++) { bounds[2 * k] = fb[k]; bounds[2 * k + 1] = fe[k]; }
    return nf;
}

// the n bytes at `field` as a number of at most `max`: the value, -1 when refused
int64_t sam_number(const char* field, int64_t n, int64_t max)
{
    const wg_sam_text T = {field};
    int64_t v = -1;
    return wg_sam_number(T, 0, n, max, v) ? v : -1;
}

int sam_keep(uint32_t flag, int64_t mapq, const SamPlan* p) { return wg_sam_keep(flag, mapq, p->par) ? 1 : 0; }
int sam_is_bottom(uint32_t flag, int paired) { return wg_sam_is_bottom(flag, paired != 0) ? 1 : 0; }

// the CIGAR over a SEQ: the adjusted length, -1 when refused; adj (when given): the adjusted sequence through the cursor, read to
// adj_len + 2 (the two bytes behind its end are 0)
int64_t sam_cigar(const char* cigar, int64_t nc, const char* seq, int64_t ns, char* adj)
{
    std::string both(cigar, (size_t)nc);
    both.append(seq, (size_t)ns);
    const wg_sam_text T = {both.data()};
    int64_t len = -1;
    if (!wg_sam_cigar_check(T, 0, nc, ns, len)) return -1;
    if (adj) {
        const wg_sam_geom g = {0, nc, nc, 0, len, false};
        wg_sam_cursor<wg_sam_text> cur = wg_sam_begin(T, g);
        for (int64_t i = 0; i < len + 2; i++) adj[i] = cur.at(i);
    }
    return len;
}

// the line at byte p: out = {state, caller's chromosome index or -1, qlen, start, plen, bottom}; pat (when given and room >= plen): its bytes
void sam_eval(const SamPlan* plan, const uint32_t* loci, const char* text, int64_t n, int64_t p, int64_t* out, char* pat, int64_t room)
{
    const wg_sam_text T = {text};
    const wg_sam_read r = wg_sam_eval(T, p, n, plan->par, plan->chroms.view(), loci);
    out[0] = r.state; out[1] = r.rank < 0 ? -1 : plan->chroms.order[(size_t)r.rank]; out[2] = r.qlen; out[3] = r.start; out[4] = r.plen; out[5] = r.bottom;
    if (r.state == WG_SAM_PAT && pat && room >= (int64_t)r.plen) {
        auto src = wg_sam_pat_begin(T, wg_sam_geom_again(T, p, n, r.bottom != 0), loci, r.start - 1, (int64_t)plan->par.clip);
        for (uint32_t i = 0; i < r.plen; i++) pat[i] = src((int64_t)i);
    }
}

// merge_PE of two pats in memory: out = {why, rs, first, len}; span (room for 300 bytes): the bytes before the dots go
void sam_merge(int64_t sa, const char* pa, int64_t la, int64_t sb, const char* pb, int64_t lb, int64_t* out, char* span)
{
    const wg_sam_merged m = wg_sam_merge(sa, la, wg_sam_pat_of_bytes{pa}, sb, lb, wg_sam_pat_of_bytes{pb}, [&](int64_t k, char c) { span[k] = c; });
    out[0] = m.why; out[1] = m.rs; out[2] = m.first; out[3] = m.len;
}

int sam_same_read(const char* a, uint32_t la, int32_t rank_a, const char* b, uint32_t lb, int32_t rank_b)
{
    return wg_sam_same_read(wg_sam_text{a}, 0, la, rank_a, wg_sam_text{b}, 0, lb, rank_b) ? 1 : 0;
}

// sizes the kernels and the host agree on
void sam_sizes(int64_t* out) { out[0] = (int64_t)sizeof(wg_sam_read); out[1] = (int64_t)sizeof(wg_sam_carry); out[2] = WG_SAM_COUNTERS; out[3] = WG_SAM_BLOCK; }

// a whole file on the host (sam_run.h): the text to out (room bytes); returns its length, -1 when it does not fit; stats[WG_SAM_COUNTERS]
int64_t sam_run(const SamPlan* plan, const uint32_t* loci, const char* text, int64_t n, char* out, int64_t room, int64_t* stats)
{
    const std::string res = sam_run_host(text, n, *plan, loci, stats);
    if ((int64_t)res.size() > room) return -1;
    memcpy(out, res.data(), res.size());
    return (int64_t)res.size();
}

}  // extern "C"
