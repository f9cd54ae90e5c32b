// Host twin of the probe table's text rule and host plan (TEST INFRASTRUCTURE), a stand-alone program: csrc/bed_fmt.h's wg_fmt_f3 —
// the "%.3f" of meth / cov from the two counts — against snprintf on every uint8 pair, on every exact tie of the 16-bit pairs'
// first odd multiples and on 10^6 seeded random 16-bit pairs; csrc/array_plan.h — the text of a value, the slab arithmetic, every
// refusal that needs no device.  tests/test_450k_cpu.py builds it plain and with AddressSanitizer + UndefinedBehaviorSanitizer, runs
// both and reads what they print.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <numeric>
#include "../../wgbs_tools_amd/csrc/array_plan.h"

static long long g_checked = 0, g_bad = 0;

static void check_f3(uint32_t m, uint32_t c)
{
    char want[32], got[32];
    snprintf(want, sizeof want, "%.3f", (double)m / (double)c);
    const uint32_t q = wg_fmt_f3(m, c);
    const int n = wg_f3_put(got, q);
    got[n] = 0;
    g_checked++;
    if (n != wg_f3_len(q) || n > WG_F3_MAX_LEN || strcmp(want, got)) {
        if (g_bad++ < 5) printf("MISMATCH %u / %u: %s, snprintf says %s\n", m, c, got, want);
    }
}

static void report(const char* what)
{
    printf("%s: %lld checked, %lld mismatches\n", what, g_checked, g_bad);
    g_checked = g_bad = 0;
}

static std::string value(uint32_t m, uint32_t c, uint32_t min_cov)
{
    char buf[16];
    uint32_t q;
    const int n = wg_site_value(m, c, min_cov, &q);
    wg_site_value_put(buf, n, q);
    return std::string(buf, (size_t)n);
}

struct Call {
    std::vector<int64_t> site0 = {0, 2999, 5, 5};
    std::vector<int32_t> samples = {0, 1, 0};
    std::vector<int64_t> off = {0, 3, 3, 10, 73};
    std::string labels = std::string(73, 'x');
    wgbsseg_site_table_opts o = {3, 0, 0};
    int32_t n_samples = 2;
    int64_t n_total = 3000;
    bool null_sites = false, null_samples = false, null_off = false, null_labels = false, null_opts = false;
    int64_t n_rows = 4;
    int32_t n_cols = 3;
};

static void plan(const char* what, const Call& k)
{
    SitePlan p;
    std::string msg;
    int rc = wg_site_check_gather("site_table", k.null_sites ? nullptr : k.site0.data(), k.n_rows, k.null_samples ? nullptr : k.samples.data(), k.n_cols,
                                  k.n_samples, k.n_total, msg);
    if (rc == WGBSSEG_OK)
        rc = wg_site_plan(k.n_rows, k.n_cols, k.null_labels ? nullptr : k.labels.data(), k.null_off ? nullptr : k.off.data(), k.null_opts ? nullptr : &k.o, p, msg);
    if (rc == WGBSSEG_OK)
        printf("%s: accepted: %" PRId64 " rows x %d, slabs of %" PRId64 ": %" PRId64 ", longest label %d, bound of slab 0: %" PRId64 "\n", what, p.n_rows, p.n_cols,
               p.slab_rows, p.n_slabs, p.max_label, p.slab_bytes_bound(0));
    else
        printf("%s: refused (%d): %s\n", what, rc, msg.c_str());
}

int main()
{
    for (uint32_t m = 0; m < 256; m++) for (uint32_t c = 1; c < 256; c++) check_f3(m, c);
    report("every 8-bit pair");
    // 2000 m = k c, k odd: 16 divides c, m = j c / gcd(c, 2000) for odd j (tests/array_cases.py: tie_pairs, here with twenty multiples)
    for (uint32_t c = 16; c < 65536; c += 16) {
        const uint32_t g = std::gcd(c, 2000u);
        for (uint32_t j = 1; j < 40; j += 2) {
            const uint64_t m = (uint64_t)j * (c / g);
            if (m > 65535) break;
            if ((2000 * m) % c != 0 || ((2000 * m) / c) % 2 != 1) { printf("not a tie: %" PRIu64 " / %u\n", m, c); return 1; }
            check_f3((uint32_t)m, c);
        }
    }
    report("exact ties");
    uint64_t s = 20261102;                                       // splitmix64
    for (int i = 0; i < 1000000; i++) {
        s += 0x9e3779b97f4a7c15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        check_f3((uint32_t)(z & 0xffff), (uint32_t)((z >> 16) % 65535) + 1);
    }
    report("random 16-bit pairs");

    printf("values: %s %s %s %s %s %s %s %s %s\n", value(1, 2, 3).c_str(), value(3, 3, 3).c_str(), value(0, 0, 0).c_str(), value(7, 0, 0).c_str(),
           value(7, 0, 1).c_str(), value(5, 2, 0).c_str(), value(65535, 1, 1).c_str(), value(1, 65535, 70000).c_str(), value(1, 16, 1).c_str());
    printf("constants: block %d, label %d, field %d, stage %d, cols %d, slab rows %d / %d, slab fields %d / %d\n", WG_SITE_BLOCK, WG_SITE_MAX_LABEL, WG_SITE_MAX_FIELD,
           WG_SITE_STAGE_BYTES, WG_SITE_MAX_COLS, WG_SITE_DEFAULT_SLAB_ROWS, WG_SITE_MAX_SLAB_ROWS, WG_SITE_DEFAULT_SLAB_FIELDS, WG_SITE_MAX_SLAB_FIELDS);
    printf("default slab rows: %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", wg_site_default_slab_rows(1), wg_site_default_slab_rows(31), wg_site_default_slab_rows(32),
           wg_site_default_slab_rows(WG_SITE_MAX_COLS));

    Call k;
    plan("as it is", k);
    { Call b = k; b.o.slab_rows = 3; plan("slabs of 3", b); }
    { Call b = k; b.n_rows = 0; plan("no rows", b); }
    { Call b = k; b.n_rows = -1; plan("n_rows -1", b); }
    { Call b = k; b.n_cols = 0; plan("n_cols 0", b); }
    { Call b = k; b.n_cols = WG_SITE_MAX_COLS + 1; plan("n_cols above", b); }
    { Call b = k; b.null_sites = true; plan("site0 NULL", b); }
    { Call b = k; b.null_samples = true; plan("samples NULL", b); }
    { Call b = k; b.null_off = true; plan("label_off NULL", b); }
    { Call b = k; b.null_labels = true; plan("labels NULL", b); }
    { Call b = k; b.null_opts = true; plan("opts NULL", b); }
    { Call b = k; b.samples[1] = 2; plan("sample 2", b); }
    { Call b = k; b.samples[2] = -1; plan("sample -1", b); }
    { Call b = k; b.site0[1] = 3000; plan("site 3000", b); }
    { Call b = k; b.site0[3] = -1; plan("site -1", b); }
    { Call b = k; b.o.min_cov = -1; plan("min_cov -1", b); }
    { Call b = k; b.off[2] = 2; plan("offsets descend", b); }
    { Call b = k; b.off[4] = 75; b.labels = std::string(75, 'x'); plan("label of 65 bytes", b); }
    { Call b = k; b.o.slab_rows = -1; plan("slab_rows -1", b); }
    { Call b = k; b.o.slab_rows = WG_SITE_MAX_SLAB_ROWS + 1; plan("slab_rows above", b); }
    { Call b = k; b.o.slab_rows = WG_SITE_MAX_SLAB_ROWS; plan("the largest slab", b); }
    { Call b = k; b.o.slab_rows = WG_SITE_MAX_SLAB_ROWS; b.n_cols = 16; b.samples.assign(16, 1); plan("too many fields", b); }

    SitePlan p;
    p.n_rows = 1000; p.n_cols = 33; p.slab_rows = 300; p.n_slabs = 4; p.max_label = 10;
    int64_t at = 0;
    for (int64_t s2 = 0; s2 < p.n_slabs; s2++) {
        printf("slab %" PRId64 ": first %" PRId64 " rows %" PRId64 " fields %" PRId64 " cells %" PRId64 " workgroups %" PRId64 " bound %" PRId64 "\n", s2, p.slab_first(s2), p.slab_count(s2),
               p.fields(p.slab_count(s2)), p.cells(p.slab_count(s2)), SitePlan::workgroups(p.fields(p.slab_count(s2))), p.slab_bytes_bound(s2));
        at += p.slab_count(s2);
    }
    printf("rows in slabs: %" PRId64 "\n", at);
    return 0;
}
