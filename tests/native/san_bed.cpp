// Sanitizer harness for the host-only part of beta2bed (TEST INFRASTRUCTURE): csrc/bed_fmt.h — every uint8 pair and a sweep of
// uint16 pairs through the "%.3g" rule, against the C library's own printf — and csrc/bed_plan.h — the argument checks on
// fixed inputs, every array heap-allocated at its exact size so that a read past an end is seen; the chromosome table packed
// from exact-size names (the longest one last), the workgroup table's layout, the text buffers' capacity, the slab parity.
// tests/test_beta2bed_cpu.py builds it plain and with AddressSanitizer + UndefinedBehaviorSanitizer and compares the lines.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "bed_plan.h"

static long check_g3(uint32_t m, uint32_t c)
{
    int len = 0;
    const uint64_t v = wg_fmt_g3(m, c, &len);
    char got[9] = {0}, want[32];
    memcpy(got, &v, 8);
    snprintf(want, sizeof want, "%.3g", (double)m / (double)c);
    return (len == (int)strlen(want) && !strcmp(got, want)) ? 0 : 1;
}

static void plan_case(const char* what, int32_t sample, int32_t n_samples, int64_t start0, int64_t end0, int64_t n_total, std::vector<int64_t> cum,
                      std::vector<const char*> names, wgbsseg_bed_opts o, bool null_opts = false)
{
    BedPlan p;
    std::string msg;
    const int rc = wg_bed_plan(sample, n_samples, start0, end0, n_total, cum.data(), names.data(), (int32_t)cum.size(), null_opts ? nullptr : &o, p, msg);
    if (rc == WGBSSEG_OK) printf("%s: accepted: %lld slabs of %lld, stage %d, longest name %d\n", what, (long long)p.n_slabs, (long long)p.slab_sites, (int)p.stage_bytes, (int)p.max_name);
    else printf("%s: refused (%d): %s\n", what, rc, msg.c_str());
}

// the packed chromosome table of `names` (each copied into a heap array of exactly its length + 1): its size, offsets and a checksum
static void table_case(const char* what, const std::vector<std::string>& names)
{
    std::vector<std::vector<char>> held;
    std::vector<const char*> ptr;
    std::vector<int64_t> cum;
    for (const std::string& n : names) {
        held.emplace_back(n.c_str(), n.c_str() + n.size() + 1);
        cum.push_back((int64_t)(cum.size() + 1) * 1000);
    }
    for (const auto& h : held) ptr.push_back(h.data());
    const int32_t n = (int32_t)names.size();
    const BedChromTable t = wg_bed_chrom_table(n);
    const std::vector<char> tab = wg_bed_pack_chroms(cum.data(), ptr.data(), n);
    unsigned long sum = 0;
    for (char c : tab) sum = sum * 31 + (unsigned char)c;
    const char* last = tab.data() + t.names + (size_t)(n - 1) * WG_BED_NAME_REC;
    printf("%s: %zu bytes (cum %zu, names %zu), last record %d bytes, checksum %lu\n", what, tab.size(), t.cum, t.names, (int)last[WG_BED_NAME_REC - 1], sum);
}

int main()
{
    long bad = 0;
    for (uint32_t m = 0; m < 256; m++) for (uint32_t c = 1; c < 256; c++) bad += check_g3(m, c);
    for (uint32_t m = 1; m < 65536; m += 97) for (uint32_t c = 1; c < 65536; c += 89) bad += check_g3(m, c);
    for (uint32_t c : {16u, 32u, 64u, 2000u, 4000u, 62500u, 64000u}) for (uint32_t m = 1; m < 65536; m++) bad += check_g3(m, c);
    bad += check_g3(1, 65535) + check_g3(65535, 1) + check_g3(65535, 65535) + check_g3(1000, 1);
    printf("g3 mismatches: %ld\n", bad);
    char digits[20];
    printf("digits: %d %d %d\n", wg_dec_put(digits, 0), wg_dec_put(digits, 4294967296ull), wg_dec_put(digits, 18446744073709551615ull));

    const wgbsseg_bed_opts plain = {1, 0, 0, 0, 0};
    const std::string long_name(WG_BED_MAX_NAME + 1, 'c'), top_name(WG_BED_MAX_NAME, 'c');
    plan_case("plain", 0, 1, 0, 3000, 3000, {1, 256, 513, 3000}, {"chr1", "MT", top_name.c_str(), "chrX"}, plain);
    plan_case("slabs of 257", 2, 3, 5, 2999, 3000, {3000}, {"chr1"}, {10, 1, 1, 64, 257});
    plan_case("nothing selected", 0, 1, 7, 7, 3000, {3000}, {"chr1"}, plain);
    plan_case("null opts", 0, 1, 0, 3000, 3000, {3000}, {"chr1"}, plain, true);
    plan_case("sample", 3, 3, 0, 3000, 3000, {3000}, {"chr1"}, plain);
    plan_case("sample below", -1, 3, 0, 3000, 3000, {3000}, {"chr1"}, plain);
    plan_case("range past the rows", 0, 1, 0, 3001, 3000, {3000}, {"chr1"}, plain);
    plan_case("range reversed", 0, 1, 10, 9, 3000, {3000}, {"chr1"}, plain);
    plan_case("min_cov", 0, 1, 0, 3000, 3000, {3000}, {"chr1"}, {0, 0, 0, 0, 0});
    plan_case("stage", 0, 1, 0, 3000, 3000, {3000}, {"chr1"}, {1, 0, 0, WG_BED_STAGE_BYTES + 1, 0});
    plan_case("slab", 0, 1, 0, 3000, 3000, {3000}, {"chr1"}, {1, 0, 0, 0, (int64_t)WG_BED_MAX_SLAB + 1});
    plan_case("cum short", 0, 1, 0, 3000, 3000, {1, 2999}, {"chr1", "chr2"}, plain);
    plan_case("cum descends", 0, 1, 0, 3000, 3000, {10, 9, 3000}, {"chr1", "chr2", "chr3"}, plain);
    plan_case("long name", 0, 1, 0, 3000, 3000, {1, 3000}, {"chr1", long_name.c_str()}, plain);
    plan_case("no name", 0, 1, 0, 3000, 3000, {1, 3000}, {"chr1", ""}, plain);
    plan_case("no table", 0, 1, 0, 3000, 3000, {}, {}, plain);

    std::string msg;
    std::vector<uint16_t> mult(1000, 3);
    printf("mult: %d\n", wg_bed_check_mult(mult.data(), (int64_t)mult.size(), 40, msg));
    mult[999] = WG_BED_MULT_TOO_MANY;
    const int rc = wg_bed_check_mult(mult.data(), (int64_t)mult.size(), 40, msg);
    printf("mult: %d %s\n", rc, msg.c_str());
    printf("mult: %d\n", wg_bed_check_mult(nullptr, 1000, 0, msg));
    printf("slab bytes: %d", wg_bed_check_slab_bytes(WG_BED_MAX_SLAB_BYTES - 1, 3, 1000, msg));
    const int rc2 = wg_bed_check_slab_bytes(WG_BED_MAX_SLAB_BYTES, 3, 1000, msg);
    printf(" %d %s\n", rc2, msg.c_str());

    table_case("table of 1", {"c"});
    table_case("table of 4", {"chr1", "MT", "chrX", top_name});
    std::vector<std::string> many;
    for (int i = 0; i < WG_BED_LDS_CHROMS + 1; i++) many.push_back(i % 2 ? "c" + std::to_string(i) : std::string(WG_BED_MAX_NAME - i % 3, 'x'));
    many.back() = top_name;
    table_case("table of 65", many);
    for (int64_t wgs : {1ll, 2ll, 4096ll}) {
        const BedWgTable t = wg_bed_wg_table(wgs);
        printf("wg table of %lld: %lld %lld %lld %lld %lld, %lld words, %zu bytes\n", (long long)wgs, (long long)t.bytes, (long long)t.lines, (long long)t.base,
               (long long)t.tot_bytes, (long long)t.tot_lines, (long long)t.words, t.size());
    }
    for (uint64_t tot : {0ull, 9999ull, 10000ull, 10001ull, (unsigned long long)WG_BED_MAX_SLAB_BYTES - 1}) {
        const BedTextCap c = wg_bed_text_capacity(tot, 10000);
        printf("capacity for %llu of 10000: %zu at home, %zu on the device\n", (unsigned long long)tot, c.home, c.device);
    }
    printf("parity: %d %d %d %d\n", wg_bed_parity(0), wg_bed_parity(1), wg_bed_parity(2), wg_bed_parity(4097));
    return bad ? 1 : 0;
}
