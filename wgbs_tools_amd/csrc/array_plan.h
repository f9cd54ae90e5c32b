// array_plan.h — the host plan of the probe table (wgbsseg_site_counts, wgbsseg_site_table, `wgbstools beta_to_450k`) and what host
// and device agree on: the workgroup size, the longest field, the text of a value, the slabs.  No HIP here (like bed_plan.h): g++
// compiles it alone, tests/native/array_host.cpp runs it plain and under the sanitizers.
//
// The table has a row per probe: row r is  label_r , v , v , ... v \n  with a value per column; a column is a resident sample.  The
// text passes work on FIELDS, n_cols + 1 per row in row-major order: field 0 is the label and a comma, field f >= 1 the value of
// column f - 1 and a comma, or a line break behind the last one.  A label has at most WG_SITE_MAX_LABEL bytes, a value at most
// WG_F3_MAX_LEN: no field is longer than WG_SITE_MAX_FIELD bytes, so the WG_SITE_BLOCK fields of a workgroup ALWAYS fit its LDS
// stage of WG_SITE_STAGE_BYTES and the emit pass has no other path.
//
// A value (wg_site_value): NA where cov < min_cov; else the "%.3f" of the double meth / cov (bed_fmt.h: wg_fmt_f3).  min_cov 0
// lets cov = 0 through, as numpy's division does: 0 / 0 is NA, m / 0 with m > 0 is inf.
#pragma once
#include "bed_plan.h"

#define WG_SITE_BLOCK 256                      // fields (= threads) of one workgroup of the text passes, cells of one of the gather
#define WG_SITE_MAX_LABEL 63                   // longest label, in bytes
#define WG_SITE_MAX_FIELD (WG_SITE_MAX_LABEL + 1)
#define WG_SITE_STAGE_BYTES (WG_SITE_BLOCK * WG_SITE_MAX_FIELD)     // 16,384
#define WG_SITE_MAX_COLS 4096
#define WG_SITE_DEFAULT_SLAB_ROWS (1 << 16)    // rows per slab when the caller says 0 ...
#define WG_SITE_DEFAULT_SLAB_FIELDS (1 << 21)  // ... but no more rows than hold this many fields: 8192 workgroup totals, ONE workgroup scans them in 32 steps
#define WG_SITE_MAX_SLAB_ROWS (1 << 22)
#define WG_SITE_MAX_SLAB_FIELDS (1 << 26)      // a slab's fields fit an int32 and its text (below 37 bytes per field on average) 4 GiB

static_assert(WG_SITE_BLOCK == WG_BED_BLOCK, "k_bed_scan and wg_bed_block_scan serve both exports");
static_assert(WG_F3_MAX_LEN + 1 <= WG_SITE_MAX_FIELD, "a value and its separator are a field");
static_assert((uint64_t)WG_SITE_MAX_SLAB_FIELDS * 37 < (1ull << 32), "a slab's text stays below 4 GiB");

// The text of one value: its length (2: NA, 3: inf, else a "%.3f" of wg_f3_len(*q) bytes) and, for the last kind, q.
WG_HD int wg_site_value(uint32_t meth, uint32_t cov, uint32_t min_cov, uint32_t* q)
{
    *q = 0;
    if (cov < min_cov) return 2;
    if (cov == 0) return meth ? 3 : 2;
    *q = wg_fmt_f3(meth, cov);
    return wg_f3_len(*q);
}

// ... and its bytes at dst: `len` and `q` as wg_site_value gave them
template <class P>
WG_HD void wg_site_value_put(P dst, int len, uint32_t q)
{
    if (len == 2) { dst[0] = 'N'; dst[1] = 'A'; }
    else if (len == 3) { dst[0] = 'i'; dst[1] = 'n'; dst[2] = 'f'; }
    else wg_f3_put(dst, q);
}

struct SitePlan {
    int64_t n_rows = 0;
    int32_t n_cols = 0;
    int64_t slab_rows = 0;             // rows per slab (the last one may hold fewer)
    int64_t n_slabs = 0;
    int32_t min_cov = 0;
    int32_t max_label = 0;             // the longest label of the call

    int64_t slab_first(int64_t k) const { return k * slab_rows; }
    int64_t slab_count(int64_t k) const { const int64_t left = n_rows - slab_first(k); return left < slab_rows ? left : slab_rows; }
    int64_t fields(int64_t rows) const { return rows * ((int64_t)n_cols + 1); }
    int64_t cells(int64_t rows) const { return rows * (int64_t)n_cols; }
    static int64_t workgroups(int64_t items) { return (items + WG_SITE_BLOCK - 1) / WG_SITE_BLOCK; }
    // what a slab's text can take: the first size of its two buffers
    int64_t slab_bytes_bound(int64_t k) const { return slab_count(k) * ((int64_t)max_label + 1 + (int64_t)n_cols * (WG_F3_MAX_LEN + 1)); }
};

// rows per slab when the caller leaves the choice: WG_SITE_DEFAULT_SLAB_ROWS, fewer for wide rows
constexpr int64_t wg_site_default_slab_rows(int32_t n_cols)
{
    return WG_SITE_DEFAULT_SLAB_FIELDS / ((int64_t)n_cols + 1) < WG_SITE_DEFAULT_SLAB_ROWS
               ? (WG_SITE_DEFAULT_SLAB_FIELDS / ((int64_t)n_cols + 1) > 0 ? WG_SITE_DEFAULT_SLAB_FIELDS / ((int64_t)n_cols + 1) : 1)
               : WG_SITE_DEFAULT_SLAB_ROWS;
}

// What both calls gather: the rows' sites and the columns' samples against n_samples resident rows of n_total sites.
inline int wg_site_check_gather(const char* who, const int64_t* site0, int64_t n_rows, const int32_t* samples, int32_t n_cols, int32_t n_samples,
                                int64_t n_total, std::string& msg)
{
    if (n_rows < 0) return wg_bed_refuse(msg, "%s: n_rows = %lld is negative", who, (long long)n_rows);
    if (n_cols < 1 || n_cols > WG_SITE_MAX_COLS) return wg_bed_refuse(msg, "%s: n_cols = %d is outside 1 .. %d", who, (int)n_cols, WG_SITE_MAX_COLS);
    if (!samples) return wg_bed_refuse(msg, "%s: samples is NULL", who);
    if (n_rows > 0 && !site0) return wg_bed_refuse(msg, "%s: site0 is NULL", who);
    for (int32_t j = 0; j < n_cols; j++)
        if (samples[j] < 0 || samples[j] >= n_samples)
            return wg_bed_refuse(msg, "%s: column %d: sample %d is outside the %d resident samples", who, (int)j, (int)samples[j], (int)n_samples);
    for (int64_t r = 0; r < n_rows; r++)
        if (site0[r] < 0 || site0[r] >= n_total)
            return wg_bed_refuse(msg, "%s: row %lld: site %lld is outside the %lld resident sites", who, (long long)r, (long long)site0[r], (long long)n_total);
    return WGBSSEG_OK;
}

// The arguments of wgbsseg_site_table beyond wg_site_check_gather's.  WGBSSEG_OK and a filled plan, or WGBSSEG_E_ARG and a message
// naming the offender.
inline int wg_site_plan(int64_t n_rows, int32_t n_cols, const char* labels, const int64_t* label_off, const wgbsseg_site_table_opts* o, SitePlan& p,
                        std::string& msg)
{
    const char* who = "site_table";
    if (!o) return wg_bed_refuse(msg, "%s: opts is NULL", who);
    if (o->min_cov < 0) return wg_bed_refuse(msg, "%s: min_cov = %d is negative", who, (int)o->min_cov);
    if (o->slab_rows < 0 || o->slab_rows > WG_SITE_MAX_SLAB_ROWS)
        return wg_bed_refuse(msg, "%s: slab_rows = %lld is outside 0 .. %d (0: the default, at most %d)", who, (long long)o->slab_rows, WG_SITE_MAX_SLAB_ROWS, WG_SITE_DEFAULT_SLAB_ROWS);
    if (o->slab_rows * ((int64_t)n_cols + 1) > WG_SITE_MAX_SLAB_FIELDS)
        return wg_bed_refuse(msg, "%s: slab_rows = %lld rows of %d fields are more than %d fields in a slab", who, (long long)o->slab_rows, (int)n_cols + 1, WG_SITE_MAX_SLAB_FIELDS);
    if (!label_off) return wg_bed_refuse(msg, "%s: label_off is NULL", who);
    int32_t max_label = 0;
    for (int64_t r = 0; r < n_rows; r++) {
        const int64_t len = label_off[r + 1] - label_off[r];
        if (len < 0) return wg_bed_refuse(msg, "%s: label_off[%lld] = %lld descends", who, (long long)(r + 1), (long long)label_off[r + 1]);
        if (len > WG_SITE_MAX_LABEL) return wg_bed_refuse(msg, "%s: the label of row %lld has %lld bytes, at most %d are supported", who, (long long)r, (long long)len, WG_SITE_MAX_LABEL);
        if (len > max_label) max_label = (int32_t)len;
    }
    if (label_off[0] < 0) return wg_bed_refuse(msg, "%s: label_off[0] = %lld is negative", who, (long long)label_off[0]);
    if (n_rows > 0 && label_off[n_rows] > label_off[0] && !labels) return wg_bed_refuse(msg, "%s: labels is NULL", who);
    p.n_rows = n_rows;
    p.n_cols = n_cols;
    p.slab_rows = o->slab_rows ? o->slab_rows : wg_site_default_slab_rows(n_cols);
    p.n_slabs = (n_rows + p.slab_rows - 1) / p.slab_rows;
    p.min_cov = o->min_cov;
    p.max_label = max_label;
    return WGBSSEG_OK;
}
