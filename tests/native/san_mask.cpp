// tests/native/san_mask.cpp — a stand-alone program over wgbs_tools_amd/csrc/mask_plan.h, view_core.h and view_plan.h for the sanitizers
// (tests/test_mask_pat_cpu.py builds it plain and with -fsanitize=address,undefined and runs it directly): the whole of `mask_pat` on the
// host, by the functions the kernels call — plan the blocks, compose the bitmap word by word into an array of exactly its size, cut every
// line with the masked cut, keep records and arena bytes ('.' where a site is hidden; the arena grown by the plan's rule), sort the
// permutation with wg_view_less, find the run heads, sum, and write every line with wg_view_line_len / wg_view_int_put.
//   san_mask PAT BLOCKS s e flags     (PAT: well-formed pat lines; BLOCKS: lines "startCpG endCpG"; flags: view_core.h's)
//   -> the output text on stdout, "loaded N sites ..." on stderr
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>
#include "view_plan.h"
#include "mask_plan.h"

static bool slurp(const char* path, std::string& text)
{
    FILE* f = fopen(path, "rb");
    if (!f) { perror(path); return false; }
    char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    fclose(f);
    return true;
}

int main(int argc, char** argv)
{
    if (argc != 6) { fprintf(stderr, "usage: san_mask PAT BLOCKS s e flags\n"); return 2; }
    std::string text, table;
    if (!slurp(argv[1], text) || !slurp(argv[2], table)) return 2;
    ViewPlan plan;
    std::string msg;
    if (plan_view(atoll(argv[3]), atoll(argv[4]), atoi(argv[5]), 1, 4, plan, msg) != WGBSSEG_OK) { fprintf(stderr, "%s\n", msg.c_str()); return 3; }
    std::vector<int64_t> bs, be;
    for (const char* p = table.c_str(); *p;) {
        char* q;
        const long long a = strtoll(p, &q, 10);
        if (q == p) break;
        const long long b = strtoll(q, &q, 10);
        bs.push_back(a); be.push_back(b);
        p = q;
        while (*p == '\n' || *p == ' ') p++;
    }
    MaskPlan mp;
    if (plan_mask(bs.data(), be.data(), (int64_t)bs.size(), mp, msg) != WGBSSEG_OK) { fprintf(stderr, "%s\n", msg.c_str()); return 3; }
    uint32_t* words = static_cast<uint32_t*>(malloc((size_t)mp.n_words * 4));      // exactly the bitmap: a word too many is seen
    for (int64_t w = 0; w < mp.n_words; w++) words[w] = wg_mask_word(mp.starts.data(), mp.ends.data(), mp.n_intervals(), mp.lo, w);
    const wg_view_mask mask = {words, mp.lo, mp.hi};
    std::vector<wg_view_rec> recs;
    int64_t cap = 16, used = 0, grown = 0;                         // the arena: exactly `cap` bytes, so that a byte too many is seen
    char* arena = static_cast<char*>(malloc((size_t)cap));
    size_t pos = 0;
    while (pos < text.size()) {
        size_t end = text.find('\n', pos);
        if (end == std::string::npos) end = text.size();
        if (end > pos) {
            const char* line = text.data() + pos;
            const char* t1 = static_cast<const char*>(memchr(line, '\t', end - pos));
            const char* t2 = t1 ? static_cast<const char*>(memchr(t1 + 1, '\t', line + (end - pos) - t1 - 1)) : nullptr;
            const char* t3 = t2 ? static_cast<const char*>(memchr(t2 + 1, '\t', line + (end - pos) - t2 - 1)) : nullptr;
            if (!t3 || t3 == t2 + 1) { fprintf(stderr, "malformed line at %zu\n", pos); return 4; }
            const int64_t rs = atoll(t1 + 1), plen = t3 - t2 - 1;
            const char* pat = t2 + 1;
            const auto byte = [&](int64_t k) { return pat[k]; };
            const wg_view_cut c = wg_view_cut_read_masked(rs, plen, byte, mask, plan.s, plan.e, plan.flags, plan.min_len);
            if (c.len > 0) {
                wg_view_rec r = {};
                r.off = (uint64_t)used; r.rs = c.rs; r.count = (int32_t)atoll(t3 + 1); r.clen = (uint32_t)(t1 - line); r.plen = (uint32_t)c.len;
                const int64_t need = used + r.clen + r.plen, to = wg_view_grow(cap, need);
                if (to != cap) {
                    char* fresh = static_cast<char*>(malloc((size_t)to));
                    memcpy(fresh, arena, (size_t)used);
                    free(arena);
                    arena = fresh; cap = to; grown++;
                }
                memcpy(arena + used, line, r.clen);
                wg_view_window w = {-1, 0};                        // (as the pack pass writes the pattern)
                for (int64_t j = 0; j < c.len; j++) arena[used + r.clen + j] = wg_view_masked_byte(mask, w, rs, c.first + j, byte);
                used = need;
                recs.push_back(r);
            }
        }
        pos = end + 1;
    }
    const size_t n = recs.size();
    std::vector<uint32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0u);
    if (plan.flags & WG_VIEW_SORT) std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return wg_view_less(recs.data(), a, b, arena); });
    std::string out;
    for (size_t i = 0; i < n;) {
        size_t j = i + 1;
        int64_t sum = recs[perm[i]].count;
        while (j < n && !wg_view_run_head(recs[perm[j - 1]], recs[perm[j]], arena)) sum += recs[perm[j++]].count;
        const wg_view_rec& r = recs[perm[j - 1]];
        const uint32_t len = wg_view_line_len(r, sum);
        if (len) {
            std::vector<char> line(len);                           // exactly the length the emit kernel is given
            char* d = line.data();
            memcpy(d, arena + r.off, r.clen); d += r.clen;
            *d++ = '\t';
            d += wg_view_int_put(d, r.rs);
            *d++ = '\t';
            memcpy(d, arena + r.off + r.clen, r.plen); d += r.plen;
            *d++ = '\t';
            d += wg_dec_put(d, (uint64_t)sum);
            *d++ = '\n';
            if (d != line.data() + len) { fprintf(stderr, "line length %u, %td bytes written\n", len, d - line.data()); return 5; }
            out.append(line.data(), len);
        }
        i = j;
    }
    fwrite(out.data(), 1, out.size(), stdout);
    fprintf(stderr, "loaded %lld sites words %lld records %zu arena %lld grown %lld\n", (long long)mp.n_hidden, (long long)mp.n_words, n, (long long)used, (long long)grown);
    free(arena);
    free(words);
    return 0;
}
