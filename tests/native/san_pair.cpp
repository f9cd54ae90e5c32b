// Sanitizer harness for the host-only part of the pairwise histograms (TEST INFRASTRUCTURE): csrc/pair_plan.h — the limits
// host and device share and the checks of a call's pair list, threshold, bins and edges — on fixed inputs, every array
// heap-allocated at its exact size so that a read past an end is seen.  tests/test_compare_cpu.py builds it plain and with
// AddressSanitizer + UndefinedBehaviorSanitizer and compares the lines.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "pair_plan.h"

static void say(bool ok, const std::string& msg) { printf("%s%s\n", ok ? "accepted: " : "refused: ", ok ? "" : msg.c_str()); }

static void list_case(std::vector<int32_t> a, std::vector<int32_t> b, int64_t n_pairs, int32_t min_cov, int32_t n_samples, int64_t n_sites, bool null_a = false)
{
    std::string msg;
    say(wg_pair_check_list("pair_ranges", null_a ? nullptr : a.data(), b.data(), n_pairs, min_cov, n_samples, n_sites, msg), msg);
}

static std::vector<double> linear_edges(int64_t n_pairs, int bins)
{
    std::vector<double> e((size_t)n_pairs * 2 * (size_t)(bins + 1));
    for (int64_t p = 0; p < n_pairs; p++)
        for (int ax = 0; ax < 2; ax++)
            for (int k = 0; k <= bins; k++) e[((size_t)p * 2 + (size_t)ax) * (size_t)(bins + 1) + (size_t)k] = -0.5 * ax + (double)k / bins + 1e-3 * (double)p;
    return e;
}

static void edge_case(const std::vector<double>& e, int64_t n_pairs, int bins, bool null_e = false)
{
    std::string msg;
    say(wg_pair_check_edges(null_e ? nullptr : e.data(), n_pairs, bins, msg), msg);
}

int main()
{
    printf("limits: bins %d run %d lds %lld\n", WG_PH_MAX_BINS, WG_PH_RUN, (long long)wg_ph_lds_bytes(WG_PH_MAX_BINS));
    // the pair list
    list_case({0, 1, 1, 2, 2, 2}, {0, 0, 1, 0, 1, 2}, 6, 10, 3, 70001);
    list_case({4}, {4}, 1, 1, 5, 1);
    list_case({0, 1}, {1, 0}, 2, 65536, 2, 28217448);
    list_case({0}, {0}, 1, 0, 1, 10);
    list_case({0}, {0}, 1, -7, 1, 10);
    list_case({}, {}, 0, 1, 3, 10);
    list_case({0}, {0}, -2, 1, 3, 10);
    list_case({0, 1, 1}, {0, 0, 5}, 3, 1, 5, 10);
    list_case({-1}, {0}, 1, 1, 5, 10);
    list_case({0}, {0}, 1, 1, 1, 10, true);
    list_case(std::vector<int32_t>(70000, 0), std::vector<int32_t>(70000, 0), 70000, 1, 1, 2000000000);
    // bins
    for (int bins : {0, -1, WG_PH_MAX_BINS + 1, 1, WG_PH_MAX_BINS}) {
        std::string msg;
        say(wg_pair_check_bins(bins, msg), msg);
    }
    // edges
    edge_case(linear_edges(3, 7), 3, 7);
    edge_case(linear_edges(1, 7), 1, 7, true);
    { std::vector<double> e = linear_edges(3, 7); e[(2 * 2 + 1) * 8 + 4] = std::nan(""); edge_case(e, 3, 7); }
    { std::vector<double> e = linear_edges(3, 7); e[(2 * 2 + 1) * 8 + 4] = std::numeric_limits<double>::infinity(); edge_case(e, 3, 7); }
    { std::vector<double> e = linear_edges(2, 1); e[1] = e[0]; edge_case(e, 2, 1); }
    { std::vector<double> e = linear_edges(2, WG_PH_MAX_BINS); e[e.size() - 1] = e[e.size() - 3]; edge_case(e, 2, WG_PH_MAX_BINS); }
    return 0;
}
