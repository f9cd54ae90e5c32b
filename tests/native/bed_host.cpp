// Host twin of the beta2bed kernels' text rule and the call's host plan (TEST INFRASTRUCTURE): csrc/bed_fmt.h — the "%.3g" of
// meth / cov from the two counts, the decimal digits — and csrc/bed_plan.h — the argument checks, the line bound, the staging
// rule, the slabs, the chromosome and workgroup tables, the text buffers' capacity, the slab parity — compiled for the CPU as they are, so that tests/test_beta2bed_cpu.py can hold them against Python's own
// '%.3g' and against the fixture without a GPU.
#include <cstring>
#include "../../wgbs_tools_amd/csrc/bed_plan.h"

extern "C" {

// text [n][8] (zero-padded) and len [n] of wg_fmt_g3(m[i], c[i])
void bed_g3(const uint32_t* m, const uint32_t* c, int64_t n, char* text, int32_t* len)
{
    for (int64_t i = 0; i < n; i++) {
        int l = 0;
        const uint64_t v = wg_fmt_g3(m[i], c[i], &l);
        memcpy(text + 8 * i, &v, 8);
        len[i] = l;
    }
}

// wg_dec_put(v[i]) into text [n][20], len [n]
void bed_dec(const uint64_t* v, int64_t n, char* text, int32_t* len)
{
    for (int64_t i = 0; i < n; i++) len[i] = wg_dec_put(text + 20 * i, v[i]);
}

// wg_bed_plan; out = {slab_sites, n_slabs, stage_bytes, max_name}
int bed_plan(int32_t sample, int32_t n_samples, int64_t start0, int64_t end0, int64_t n_total, const int64_t* chrom_cum, const char* const* chrom_names,
             int32_t n_chroms, const wgbsseg_bed_opts* o, int64_t* out, char* msg, size_t msglen)
{
    BedPlan p;
    std::string m;
    const int rc = wg_bed_plan(sample, n_samples, start0, end0, n_total, chrom_cum, chrom_names, n_chroms, o, p, m);
    snprintf(msg, msglen, "%s", m.c_str());
    if (rc == WGBSSEG_OK) { out[0] = p.slab_sites; out[1] = p.n_slabs; out[2] = p.stage_bytes; out[3] = p.max_name; }
    return rc;
}

// slab k of a selection [start0, end0) cut every slab_sites: {first site, sites, workgroups, byte bound at max_name}
void bed_slab(int64_t start0, int64_t end0, int64_t slab_sites, int32_t max_name, int64_t k, int64_t* out)
{
    BedPlan p;
    p.start0 = start0; p.end0 = end0; p.slab_sites = slab_sites; p.max_name = max_name;
    p.n_slabs = (end0 - start0 + slab_sites - 1) / slab_sites;
    out[0] = p.slab_first(k); out[1] = p.slab_count(k); out[2] = BedPlan::workgroups(p.slab_count(k)); out[3] = p.slab_bytes_bound(k);
}

int bed_check_mult(const uint16_t* mult, int64_t n, int64_t start0, char* msg, size_t msglen)
{
    std::string m;
    const int rc = wg_bed_check_mult(mult, n, start0, m);
    snprintf(msg, msglen, "%s", m.c_str());
    return rc;
}

int bed_check_slab_bytes(uint64_t bytes, int64_t slab, int64_t slab_sites, char* msg, size_t msglen)
{
    std::string m;
    const int rc = wg_bed_check_slab_bytes(bytes, slab, slab_sites, m);
    snprintf(msg, msglen, "%s", m.c_str());
    return rc;
}

// wg_bed_pack_chroms into out (cap bytes) -> the table's size; offs = {cum, names} of wg_bed_chrom_table
int64_t bed_chrom_table(const int64_t* chrom_cum, const char* const* chrom_names, int32_t n_chroms, char* out, int64_t cap, int64_t* offs)
{
    const BedChromTable t = wg_bed_chrom_table(n_chroms);
    const std::vector<char> tab = wg_bed_pack_chroms(chrom_cum, chrom_names, n_chroms);
    offs[0] = (int64_t)t.cum; offs[1] = (int64_t)t.names;
    if (tab.size() != t.size || (int64_t)tab.size() > cap) return -1;
    memcpy(out, tab.data(), tab.size());
    return (int64_t)tab.size();
}

// wg_bed_wg_table(max_wgs): out = {bytes, lines, base, tot_bytes, tot_lines, words, size in bytes}
void bed_wg_table(int64_t max_wgs, int64_t* out)
{
    const BedWgTable t = wg_bed_wg_table(max_wgs);
    out[0] = t.bytes; out[1] = t.lines; out[2] = t.base; out[3] = t.tot_bytes; out[4] = t.tot_lines; out[5] = t.words; out[6] = (int64_t)t.size();
}

// wg_bed_text_capacity: out = {home, device}
void bed_text_capacity(uint64_t tot, int64_t first_bound, uint64_t* out)
{
    const BedTextCap c = wg_bed_text_capacity(tot, first_bound);
    out[0] = c.home; out[1] = c.device;
}

int bed_parity(int64_t k) { return wg_bed_parity(k); }

int64_t bed_line_bound(int64_t name_len) { return wg_bed_line_bound(name_len); }
int bed_staged(uint32_t wg_bytes, uint32_t stage_bytes) { return wg_bed_staged(wg_bytes, stage_bytes) ? 1 : 0; }
// {block, max name, max line, stage bytes, default slab, max slab, reserved multiplicity, LDS chromosomes}
void bed_constants(int64_t* out)
{
    out[0] = WG_BED_BLOCK; out[1] = WG_BED_MAX_NAME; out[2] = WG_BED_MAX_LINE; out[3] = WG_BED_STAGE_BYTES;
    out[4] = WG_BED_DEFAULT_SLAB; out[5] = WG_BED_MAX_SLAB; out[6] = WG_BED_MULT_TOO_MANY; out[7] = WG_BED_LDS_CHROMS;
}

}  // extern "C"
