// share_plan.h — the host plan of a share group (wgbsseg_plan_shares[_weighted], wgbsseg_group_*): which chunks a share owns and which
// sites it keeps resident, which share a range of a batch goes to, and which items a share may run while its bytes are still arriving.
// No HIP here (like block_plan.h and pair_plan.h): g++ compiles it alone, tests/native/san_host.cpp runs it under the sanitizers.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>
#include "../../include/wgbsseg.h"

namespace wgshare {

struct Span {                     // one share of the chunk grid, in 0-based sites
    int64_t own_lo = 0, own_hi = 0;      // [lo, hi) of the chunks the share owns (hi == lo: none)
    int64_t win_lo = 0, win_hi = 0;      // its resident window: the owned sites +- halo, inside [0, n_sites); empty for a share without chunks
    int64_t chunks = 0, work = 0;
    bool resident() const { return win_hi > win_lo; }
};
struct Range { int64_t lo, hi; };        // 0-based sites [lo, hi)

template <class F>
void parallel_for(int64_t n, int max_threads, F f)
{
    const int T = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(max_threads, (int64_t)std::thread::hardware_concurrency()), n));
    if (T <= 1) { for (int64_t i = 0; i < n; i++) f(i); return; }
    std::atomic<int64_t> next(0);
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back([&]() { for (int64_t i; (i = next.fetch_add(1)) < n;) f(i); });
    for (auto& x : th) x.join();
}

// number of scored blocks of a chunk: sum over its sites k of F_k (segmentor.cpp:111-117), by two pointers
inline int64_t chunk_work(const uint32_t* loci, int64_t lo, int64_t hi, uint32_t max_cpg, uint32_t max_bp)
{
    int64_t w = 0, e = lo;
    for (int64_t k = lo; k < hi; k++) {
        if (e < k + 1) e = k + 1;
        while (e < hi && e - k < (int64_t)max_cpg && loci[e] >= loci[k] && (uint64_t)loci[e] - loci[k] <= max_bp) e++;
        w += e - k;
    }
    return w;
}

// the halo a caller leaves to the library (halo < 0): a chunk, at least 4096 sites
inline int64_t resolve_halo(int64_t halo, int64_t chunk_size) { return halo < 0 ? std::max<int64_t>(chunk_size, 4096) : halo; }

inline int refuse(std::string& msg, const std::string& why) { msg = why; return WGBSSEG_E_ARG; }

// Cuts the chunk grid of the regions (1-based half-open, ascending, disjoint) into n_shares contiguous runs of chunks whose work is
// proportional to weights (NULL: equal).  WGBSSEG_OK and one Span per share, or WGBSSEG_E_ARG and `msg`.
inline int plan_shares(const uint32_t* loci, int64_t n_sites, const int64_t* region_start, const int64_t* region_end, int64_t n_regions, int64_t chunk_size,
                       const wgbsseg_params* P, int32_t n_shares, const double* weights, int64_t halo, std::vector<Span>& spans, std::string& msg)
{
    if (!loci || n_sites < 1 || !region_start || !region_end || n_regions < 1 || chunk_size < 1 || !P || n_shares < 1) return refuse(msg, "bad arguments to plan_shares");
    if (P->max_bp == 0 || P->max_cpg < 1) return refuse(msg, "max_bp and max_cpg must be >= 1");
    const int G = n_shares;
    struct Ck { int64_t lo, hi, w; };
    std::vector<Ck> cks;
    for (int64_t r = 0; r < n_regions; r++) {
        const int64_t a = region_start[r], b = region_end[r];
        if (a < 1 || b <= a || b - 1 > n_sites)
            return refuse(msg, "region " + std::to_string(r) + " = [" + std::to_string(a) + ", " + std::to_string(b) + ") is empty or outside the " + std::to_string(n_sites) + " sites");
        if (r && a < region_end[r - 1]) return refuse(msg, "plan_shares: regions must be ascending and disjoint");
        for (int64_t s0 = a; s0 < b; s0 += chunk_size) cks.push_back({s0 - 1, std::min(s0 + chunk_size, b) - 1, 0});
    }
    // share d's target: weights[d] / sum(weights) of the work (NULL: equal shares)
    std::vector<double> upto((size_t)G);
    {
        double sum = 0;
        for (int d = 0; d < G; d++) {
            const double w = weights ? weights[d] : 1.0;
            if (!(w >= 0.0)) return refuse(msg, "plan_shares: weights must be >= 0");
            sum += w; upto[(size_t)d] = sum;
        }
        if (!(sum > 0.0)) return refuse(msg, "plan_shares: all weights are zero");
        for (auto& u : upto) u /= sum;
    }
    if (G == 1) {
        for (auto& c : cks) c.w = c.hi - c.lo;                  // nothing to balance: do not walk the loci
    } else {
        parallel_for((int64_t)cks.size(), 32, [&](int64_t i) {
            Ck& c = cks[(size_t)i];
            c.w = chunk_work(loci, c.lo, c.hi, P->max_cpg, P->max_bp) + 4 * (c.hi - c.lo);     // + the per-site passes (scan, windows, recurrence)
        });
    }
    int64_t total = 0;
    for (auto& c : cks) total += c.w;
    halo = resolve_halo(halo, chunk_size);
    spans.assign((size_t)G, Span());
    {   // contiguous runs of chunks: share d ends where the cumulative work passes (d+1)/G of the total
        int d = 0;
        int64_t acc = 0;
        for (auto& c : cks) {
            while (d < G - 1 && (double)acc >= (double)total * (weights ? upto[(size_t)d] : (double)(d + 1) / G)) d++;
            Span& s = spans[(size_t)d];
            if (!s.chunks) s.own_lo = c.lo;
            s.own_hi = c.hi;
            s.chunks++; s.work += c.w;
            acc += c.w;
        }
    }
    for (int q = 0; q < G; q++) {
        Span& s = spans[(size_t)q];
        if (!s.chunks) s.own_lo = s.own_hi = q ? spans[(size_t)q - 1].own_hi : cks.front().lo;
        if (s.own_hi <= s.own_lo) continue;
        // window: owned sites +- halo, the lower edge on a multiple of 128 sites (views into one device buffer stay 256-byte aligned)
        s.win_lo = std::max<int64_t>(0, s.own_lo - halo) & ~127LL;
        s.win_hi = std::min<int64_t>(n_sites, s.own_hi + halo);
    }
    return WGBSSEG_OK;
}

// The share whose resident window holds the sites [lo, hi) of a batch item, or -1.  The owner of the first site (own_lo ascends: the last
// share that begins at or before it, stepping back over shares that own nothing), then the share after it, then the one before: a junction
// patch reaches into a neighbour's first or last chunk, which the halo of a window covers.  -1: the patch outgrew the halo.
// shares: a vector of records, span_of(record) their Span (the group keeps a share's span with its context).
template <class Shares, class SpanOf>
int route(const Shares& shares, SpanOf span_of, int64_t lo, int64_t hi)
{
    const int G = (int)shares.size();
    int d = (int)(std::upper_bound(shares.begin(), shares.end(), lo, [&](int64_t x, const auto& s) { return x < span_of(s).own_lo; }) - shares.begin()) - 1;
    d = std::max(d, 0);
    while (d > 0 && span_of(shares[(size_t)d]).own_hi <= span_of(shares[(size_t)d]).own_lo) d--;
    for (int q : {d, d + 1, d - 1}) {
        if (q < 0 || q >= G) continue;
        const Span& s = span_of(shares[(size_t)q]);
        if (s.win_lo <= lo && hi <= s.win_hi && s.resident()) return q;
    }
    return -1;
}

// Streaming upload: a share's bytes arrive front to back, and its items run in order of their last site while the rest is on its way.
// A sub-batch is worth a launch when a fair part of the share has landed behind the first site of the next item:
inline int64_t min_take(int64_t chunk_size, const Span& s) { return std::max<int64_t>(4 * chunk_size, (s.win_hi - s.win_lo) / 5); }

// items: ordered by hi; items[pos] is the next to run; the sites [s.win_lo, resident_hi) are resident.  Returns the end of the run of items
// that may be taken now — pos when the wait goes on: items[pos] is not all there yet, or fewer than min_take sites behind its first are.
inline size_t take_upto(const std::vector<Range>& items, size_t pos, int64_t resident_hi, int64_t min_take)
{
    if (resident_hi < items[pos].hi || resident_hi - items[pos].lo < min_take) return pos;
    size_t end = pos;
    while (end < items.size() && items[end].hi <= resident_hi) end++;
    return end;
}

}  // namespace wgshare
