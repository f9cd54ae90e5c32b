// tests/native/merge_host.cpp — test shim: the host build of wgbs_tools_amd/csrc/merge_plan.h (the plan of wgbsseg_merge_rows and the
// arithmetic of one site, which k_beta_merge shares) and of the file table of view_plan.h (wgbsseg_patview_next_file), exported so that
// tests/test_merge_cpu.py can compare them with the restatement tests/merge_ref.py and read every refusal.
//   g++ -O2 -std=c++17 -ffp-contract=off -shared -fPIC merge_host.cpp -o libmerge_host.so
#include <cstring>
#include <vector>
#include "../../wgbs_tools_amd/csrc/merge_plan.h"
#include "../../wgbs_tools_amd/csrc/view_plan.h"

static void put_msg(const std::string& m, char* msg, size_t msglen)
{
    if (msg && msglen) { strncpy(msg, m.c_str(), msglen - 1); msg[msglen - 1] = 0; }
}

extern "C" {

void merge_constants(int64_t* out) { out[0] = WG_MG_BLOCK; out[1] = WG_MG_MAX_ROWS; out[2] = WG_MG_SLAB; }

// n sites: out[2 i], out[2 i + 1] = wg_merge_site of (M[i], C[i]), wrapped to `width` bytes as the kernel's stores wrap them
void merge_sites(const uint32_t* M, const uint32_t* C, int64_t n, uint32_t max, int width, uint32_t* out)
{
    const uint32_t mask = width == 1 ? 0xffu : 0xffffu;
    for (int64_t i = 0; i < n; i++) {
        uint32_t m, c;
        wg_merge_site(M[i], C[i], max, m, c);
        out[2 * i] = m & mask; out[2 * i + 1] = c & mask;
    }
}

// info = {n_rows, out_elem, max, n_vec, n_tail, n_threads, groups, out_bytes}
int merge_plan(const int32_t* samples, int32_t n_samples, int32_t n_resident, int64_t n_total, int elem, int32_t lbeta_out, int has_out,
               int64_t* info, char* msg, size_t msglen)
{
    MergePlan p;
    std::string m;
    const int rc = plan_merge_rows(samples, n_samples, n_resident, n_total, elem, lbeta_out, has_out ? (const void*)info : nullptr, p, m);
    put_msg(m, msg, msglen);
    if (rc == WGBSSEG_OK) {
        info[0] = p.n_rows; info[1] = p.out_elem; info[2] = p.max; info[3] = p.n_vec; info[4] = p.n_tail; info[5] = p.n_threads;
        info[6] = p.groups; info[7] = p.out_bytes;
    }
    return rc;
}

int64_t merge_slabs(int64_t len) { return wg_merge_slabs(len); }
int64_t merge_slab_len(int64_t len, int64_t k) { return wg_merge_slab_len(len, k); }

// the boundary table: n files closed at end_bytes[k] / end_recs[k]
ViewFiles* files_new(const int64_t* end_bytes, const int64_t* end_recs, int64_t n)
{
    ViewFiles* f = new ViewFiles();
    for (int64_t k = 0; k < n; k++) f->close(end_bytes[k], end_recs[k]);
    return f;
}
void files_free(ViewFiles* f) { delete f; }
int files_several(const ViewFiles* f) { return f->several() ? 1 : 0; }
int64_t files_open(const ViewFiles* f) { return f->open_file(); }
// out = {file, offset inside it}
void files_locate(const ViewFiles* f, uint64_t off, int64_t* out)
{
    int64_t file = 0;
    uint64_t inside = 0;
    f->locate(off, file, inside);
    out[0] = file; out[1] = (int64_t)inside;
}
// why: 0 malformed, 1 descending, 2 count below 1
void files_refusal(const ViewFiles* f, int why, uint64_t off, char* msg, size_t msglen)
{
    put_msg(wg_view_file_refusal(*f, why == 0 ? ViewRefusal::bad_line : why == 1 ? ViewRefusal::unsorted : ViewRefusal::low_count, off), msg, msglen);
}
int files_next(int finished, int64_t left, int64_t file, char* msg, size_t msglen)
{
    std::string m;
    const int rc = plan_view_next_file(finished != 0, left, file, m);
    put_msg(m, msg, msglen);
    return rc;
}

}  // extern "C"
