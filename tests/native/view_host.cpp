// tests/native/view_host.cpp — test shim: the host build of wgbs_tools_amd/csrc/view_core.h and view_plan.h, exported so that
// tests/test_view_cpu.py can compare the cut rule, the comparator, the run-head test and the line length with the restatement
// tests/view_ref.py, and read every refusal of the plan.
//   g++ -O2 -std=c++17 -shared -fPIC view_host.cpp -o libview_host.so
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>
#include "../../wgbs_tools_amd/csrc/view_plan.h"

static void put_msg(const std::string& m, char* msg, size_t msglen)
{
    if (msg && msglen) { strncpy(msg, m.c_str(), msglen - 1); msg[msglen - 1] = 0; }
}

struct Table {
    std::vector<wg_view_rec> recs;
    std::string arena;
};

extern "C" {

void view_constants(int64_t* out)
{
    out[0] = WG_VIEW_RUN; out[1] = WG_VIEW_MERGE_ITEMS; out[2] = WG_VIEW_SLAB; out[3] = WG_VIEW_DEFAULT_RECORDS; out[4] = WG_VIEW_MIN_LINE;
    out[5] = WG_VIEW_MAX_SUM; out[6] = WG_VIEW_MAX_RECORDS; out[7] = (int64_t)sizeof(wg_view_rec);
}

// out = {rs', first, len}
void view_cut(int64_t rs, const char* pat, int64_t plen, int64_t s, int64_t e, int32_t flags, int64_t min_len, int64_t* out)
{
    const wg_view_cut c = wg_view_cut_read(rs, plen, [&](int64_t k) { return pat[k]; }, s, e, flags, min_len);
    out[0] = c.rs; out[1] = c.first; out[2] = c.len;
}

// n lines: chroms / pats hold their bytes one after the other
Table* view_table(int64_t n, const char* chroms, const uint32_t* clen, const char* pats, const uint32_t* plen, const int64_t* rs, const int32_t* count)
{
    Table* t = new Table();
    for (int64_t i = 0; i < n; i++) {
        wg_view_rec r = {};
        r.off = t->arena.size(); r.rs = rs[i]; r.count = count[i]; r.clen = clen[i]; r.plen = plen[i];
        t->arena.append(chroms, clen[i]); t->arena.append(pats, plen[i]);
        chroms += clen[i]; pats += plen[i];
        t->recs.push_back(r);
    }
    return t;
}

void view_table_free(Table* t) { delete t; }

int view_cmp(const Table* t, uint32_t i, uint32_t j) { const int d = wg_view_cmp(t->recs[i], t->recs[j], t->arena.data()); return d < 0 ? -1 : d > 0 ? 1 : 0; }
int view_less(const Table* t, uint32_t i, uint32_t j) { return wg_view_less(t->recs.data(), i, j, t->arena.data()) ? 1 : 0; }
int view_run_head(const Table* t, uint32_t i, uint32_t j) { return wg_view_run_head(t->recs[i], t->recs[j], t->arena.data()) ? 1 : 0; }
uint32_t view_line_len(const Table* t, uint32_t i, int64_t sum) { return wg_view_line_len(t->recs[i], sum); }

// the permutation std::sort gives with wg_view_less (a strict total order: no stability needed)
void view_sort(const Table* t, uint32_t* perm)
{
    std::iota(perm, perm + t->recs.size(), 0u);
    std::sort(perm, perm + t->recs.size(), [&](uint32_t a, uint32_t b) { return wg_view_less(t->recs.data(), a, b, t->arena.data()); });
}

// the text of start `v` as the emit kernel writes it -> its length
int view_int_text(int64_t v, char* out) { return wg_view_int_put(out, v) == wg_view_int_len(v) ? wg_view_int_len(v) : -1; }

// info = {s, e, flags, min_len, initial_records}
int view_plan(int64_t s, int64_t e, int32_t flags, int32_t min_len, int64_t initial_records, int64_t* info, char* msg, size_t msglen)
{
    ViewPlan p;
    std::string m;
    const int rc = plan_view(s, e, flags, min_len, initial_records, p, m);
    put_msg(m, msg, msglen);
    if (rc == WGBSSEG_OK) { info[0] = p.s; info[1] = p.e; info[2] = p.flags; info[3] = p.min_len; info[4] = p.initial_records; }
    return rc;
}

int view_plan_chunk(int64_t n_records, int64_t n_bytes, char* msg, size_t msglen)
{
    std::string m;
    const int rc = plan_view_chunk(n_records, n_bytes, m);
    put_msg(m, msg, msglen);
    return rc;
}

int view_plan_read(int64_t offset, int64_t len, int64_t total, int has_buf, char* msg, size_t msglen)
{
    std::string m;
    const int rc = plan_view_read(offset, len, total, has_buf ? (const void*)msg : nullptr, m);
    put_msg(m, msg, msglen);
    return rc;
}

int64_t view_chunk_records(int64_t n_bytes) { return wg_view_chunk_records(n_bytes); }
int64_t view_grow(int64_t cap, int64_t need) { return wg_view_grow(cap, need); }
int64_t view_runs(int64_t n) { return wg_view_runs(n); }
int view_merge_passes(int64_t n) { return wg_view_merge_passes(n); }
int64_t view_slabs(int64_t len) { return wg_view_slabs(len); }
int64_t view_slab_len(int64_t len, int64_t k) { return wg_view_slab_len(len, k); }

}  // extern "C"
