// Sanitizer harness for the host-side C++ of the library (TEST INFRASTRUCTURE): csrc/block_plan.h (the plan of a block reduction),
// csrc/share_plan.h (the plan of a share group, its router and the rule of its streaming upload), csrc/bimodal_plan.h, csrc/homog_plan.h and
// csrc/stats_plan.h (the plans of test_bimodal, homog and sample_stats), csrc/stitch.h (chunk grid, junction rehearsal, pairwise trees on the thread pool, flattening) and csrc/add_loci.h (BED rows), driven by a toy chunk engine that is a pure
// function of the site range — as the real DP is — so that junction patches share borders with their chunks or, where the toy
// makes them disagree, force the patch to double.  Built by tests/test_sanitizers_cpu.py three times (plain, ASan + UBSan,
// TSan); every build must print the same checksum lines.
//     san_host <threads> <out.bed>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <unistd.h>
#include <cmath>
#include <algorithm>
#include <set>
#include <utility>
#include "stitch.h"
#include "add_loci.h"
#include "table_io.h"
#include "block_plan.h"
#include "share_plan.h"
#include "bimodal_plan.h"
#include "homog_plan.h"
#include "stats_plan.h"

static uint64_t mix(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33; return x; }

// borders of the "DP" over sites [a, b): a, b, and every x in between that the toy rule likes.  The rule looks at x alone, except
// near the START of a range (first `fuzzy` sites), where it also depends on where the range began — like the real DP, whose
// first borders depend on its left edge — so first-attempt patches do not always agree with the left chunk.
static void toy_borders(int64_t a, int64_t b, int fuzzy, std::vector<int32_t>& out)
{
    out.clear();
    out.push_back(0);
    for (int64_t x = a + 1; x < b; x++) {
        const bool near = x - a <= fuzzy;
        const uint64_t h = near ? mix((uint64_t)x * 31 + (uint64_t)(a % 97)) : mix((uint64_t)x);
        if (h % 9 == 0) out.push_back((int32_t)(x - a));
    }
    out.push_back((int32_t)(b - a));
}

// the regions of a toy world (1-based half-open, one behind the other); returns one past the last site
static int64_t world_regions(int n_regions, int64_t region_len, std::vector<int64_t>& rs, std::vector<int64_t>& re)
{
    rs.assign((size_t)n_regions, 0); re.assign((size_t)n_regions, 0);
    int64_t pos = 1;
    for (int r = 0; r < n_regions; r++) { rs[(size_t)r] = pos; pos += region_len + 37 * r; re[(size_t)r] = pos; }
    return pos;
}

static uint64_t run_world(int n_regions, int64_t region_len, int64_t chunk, int fuzzy, bool speculate, std::vector<int64_t>& starts_out,
                          std::vector<int64_t>& ends_out)
{
    std::vector<int64_t> rs, re;
    const int64_t pos = world_regions(n_regions, region_len, rs, re);
    int64_t n_batches = 0;
    wgstitch::BatchFn fn = [&](const std::vector<wgstitch::Sites>& todo, wgstitch::BatchResult& res, std::string&) -> int {
        res.ptr.resize(todo.size()); res.cnt.resize(todo.size());
        std::vector<int32_t> tmp;
        for (size_t i = 0; i < todo.size(); i++) {
            toy_borders(todo[i].first, todo[i].second, fuzzy, tmp);
            std::unique_ptr<int32_t[]> own(new int32_t[tmp.size()]);
            memcpy(own.get(), tmp.data(), tmp.size() * 4);
            res.ptr[i] = own.get(); res.cnt[i] = (int64_t)tmp.size();
            res.owned.push_back(std::move(own));
        }
        n_batches++;
        return 0;
    };
    const int64_t cap = pos + n_regions;
    std::vector<int32_t> borders((size_t)cap);
    std::vector<int64_t> off((size_t)n_regions + 1);
    int64_t stats[8] = {0};
    std::string err;
    const int rc = wgstitch::segment_regions(rs.data(), re.data(), n_regions, chunk, fn, borders.data(), cap, off.data(), stats, err, speculate);
    if (rc != 0) { printf("world regions=%d len=%lld chunk=%lld fuzzy=%d spec=%d: rc %d (%s)\n", n_regions, (long long)region_len, (long long)chunk, fuzzy, (int)speculate, rc, err.c_str()); return 0; }
    uint64_t h = 1469598103934665603ULL;
    for (int r = 0; r < n_regions; r++) {
        for (int64_t q = off[(size_t)r]; q < off[(size_t)r + 1]; q++) { h = (h ^ (uint64_t)(uint32_t)borders[(size_t)q]) * 1099511628211ULL; }
        for (int64_t q = off[(size_t)r]; q + 1 < off[(size_t)r + 1]; q++) { starts_out.push_back(borders[(size_t)q]); ends_out.push_back(borders[(size_t)q + 1]); }
    }
    printf("world regions=%d len=%lld chunk=%lld fuzzy=%d spec=%d: %lld borders, %lld chunks, %lld patch DPs, checksum %016llx\n", n_regions,
           (long long)region_len, (long long)chunk, fuzzy, (int)speculate, (long long)off[(size_t)n_regions], (long long)stats[0], (long long)stats[1],
           (unsigned long long)h);
    return h;
}

// The plans of the block reduction (block_plan.h) over the tables of tests/block_tables.py, built here again: 17,413 sites, an edge at every multiple
// of 896 and 1024 (-1, 0, +1), blocks of 1024, 1025 and 2,500 sites with blocks fanning in and out of them, empty blocks at both ends; ordered,
// shuffled, with a nested block, one row forty times; uint8 and uint16 rows, the general kernel forced; and the refusals.  One line: a checksum.
static void block_plan_line()
{
    typedef std::pair<int64_t, int64_t> Row;
    const int64_t N = 17413, LONG[3][2] = {{1500, 2524}, {4000, 5025}, {8191, 10691}};
    std::set<int64_t> edges, cuts{0, N};
    for (int64_t tile : {896, 1024}) for (int64_t m = tile; m < N; m += tile) for (int64_t d = -1; d <= 1; d++) edges.insert(m + d);
    std::vector<Row> rows{{0, 0}, {N - 1, N}, {N, N}};
    for (int64_t x : edges) { bool in = false; for (auto& L : LONG) in |= L[0] < x && x < L[1]; if (!in) cuts.insert(x); }
    for (auto& L : LONG) {
        std::vector<int64_t> inside;
        for (int64_t x : edges) if (L[0] < x && x < L[1]) inside.push_back(x);
        const int64_t m = (int64_t)inside.size();
        cuts.insert(L[0] - 1 - m); cuts.insert(L[0]); cuts.insert(L[1]);
        for (int64_t j = 0; j < m; j++) { rows.push_back({L[0] - m + j, inside[(size_t)j]}); rows.push_back({inside[(size_t)j], L[1]}); }
    }
    for (auto it = cuts.begin(), nx = std::next(it); nx != cuts.end(); ++it, ++nx) rows.push_back({*it, *nx});
    std::sort(rows.begin(), rows.end());
    std::vector<std::vector<Row>> tables{rows};
    std::vector<Row> sh = rows;                                               // a fixed shuffle (ties in the first site fall as they fall: the sort is stable)
    for (size_t i = sh.size() - 1; i > 0; i--) std::swap(sh[i], sh[(size_t)(mix(i * 7919 + 11) % (i + 1))]);
    tables.push_back(sh);
    std::vector<Row> nest = rows;
    nest.insert(std::lower_bound(nest.begin(), nest.end(), Row(100, 0)), Row(100, 9000));
    tables.push_back(nest);
    tables.push_back(std::vector<Row>(40, Row(700, 1900)));
    tables.push_back({{5, 9}, {-1, 3}});                                      // the refusals: negative start, reversed, beyond the rows, too long for uint16 sums
    tables.push_back({{5, 9}, {9, 3}});
    tables.push_back({{5, N + 1}});
    tables.push_back({{0, 9}, {3, 3 + 65537}});
    uint64_t h = 1469598103934665603ULL;
    auto fold = [&](uint64_t v) { h = (h ^ v) * 1099511628211ULL; };
    int n_ok = 0, n_refused = 0;
    for (size_t k = 0; k < tables.size(); k++) {
        std::vector<int64_t> s0, e0;
        for (auto& r : tables[k]) { s0.push_back(r.first); e0.push_back(r.second); }
        for (int var = 0; var < 3; var++) {                                   // uint8 rows | the general kernel forced | uint16 rows, mode 0
            BlockSumPlan p;
            std::string msg;
            const int rc = plan_block_sums(s0.data(), e0.data(), (int64_t)s0.size(), k == 7 ? 70000 : N, var == 2 ? 2 : 1, 0, var == 1, p, msg);
            fold((uint64_t)(int64_t)rc); for (char ch : msg) fold((uint64_t)(unsigned char)ch);
            if (rc != WGBSSEG_OK) { n_refused++; continue; }
            n_ok++;
            fold((uint64_t)p.sorted); fold((uint64_t)p.monotone); fold((uint64_t)p.n_tiles); fold((uint64_t)p.n_direct);
            if (p.upload.size() != p.upload_words()) fold(0xbadULL);
            const BlockSumPlan::View<const int32_t> v = p.view((const int32_t*)p.upload.data());
            for (int64_t i = 0; i < p.n_blocks; i++) { fold((uint64_t)v.x0[i]); fold((uint64_t)v.x1[i]); if (v.perm) fold((uint64_t)v.perm[i]); }
            for (int64_t t = 0; t <= p.n_tiles; t++) fold((uint64_t)v.tile_first[t]);
            for (int64_t i = 0; i < p.n_direct; i++) fold((uint64_t)v.direct[i]);
        }
    }
    printf("block_plan: %zu tables of up to %zu blocks, %d plans, %d refusals, checksum %016llx\n", tables.size(), nest.size(), n_ok, n_refused, (unsigned long long)h);
}

// The rule of wgshare::route, stated by scanning: the last share that begins at or before `lo`, stepping back over shares that own nothing; that
// share, the next, the one before - the first of them whose window is not empty and holds [lo, hi).
static int route_by_scan(const std::vector<wgshare::Span>& sp, int64_t lo, int64_t hi)
{
    int d = 0;
    for (int q = 0; q < (int)sp.size(); q++) if (sp[(size_t)q].own_lo <= lo) d = q;
    while (d > 0 && sp[(size_t)d].own_hi == sp[(size_t)d].own_lo) d--;
    const int cand[3] = {d, d + 1, d - 1};
    for (int q : cand) {
        if (q < 0 || q >= (int)sp.size()) continue;
        const wgshare::Span& s = sp[(size_t)q];
        if (s.win_hi > s.win_lo && s.win_lo <= lo && hi <= s.win_hi) return q;
    }
    return -1;
}

static const wgshare::Span& same_span(const wgshare::Span& s) { return s; }

// wgshare::route on span sets made by hand, for the steps of the rule that no plan over contiguous regions reaches; the answers are written down here:
// the share whose window holds the range, the owner of its first site before its neighbours.  Returns the number of wrong answers.
static long route_by_hand(long& n_cases)
{
    typedef std::vector<wgshare::Span> Spans;                   // {own_lo, own_hi, win_lo, win_hi, chunks, work}
    // two shares that own nothing between two regions with a gap: sites in the gap "belong" to the last of them; the rule steps back over both
    const Spans gap{{0, 100, 0, 150, 1, 1}, {100, 100, 0, 0, 0, 0}, {100, 100, 0, 0, 0, 0}, {300, 400, 250, 450, 1, 1}};
    // a short middle share whose neighbours' windows reach further than its own (hand-made: a plan's windows do not nest like this)
    const Spans nest{{0, 1000, 0, 3000, 1, 1}, {1000, 1100, 896, 1200, 1, 1}, {1100, 2000, 1024, 2100, 1, 1}};
    // the first share owns nothing and the regions begin at site 5: sites before it fall to share 0, whose empty window [0, 0) must hold nothing
    const Spans lead{{5, 5, 0, 0, 0, 0}, {5, 100, 0, 150, 1, 1}};
    const struct { const Spans* sp; int64_t lo, hi; int want; } cases[] = {
        {&gap, 120, 140, 0}, {&gap, 100, 150, 0}, {&gap, 120, 151, -1}, {&gap, 260, 299, -1}, {&gap, 300, 310, 3}, {&gap, 90, 100, 0}, {&gap, 320, 451, -1},
        {&nest, 1050, 1150, 1}, {&nest, 1050, 1300, 2}, {&nest, 1000, 1300, 0}, {&nest, 1000, 3001, -1}, {&nest, 900, 1150, 0}, {&nest, 1100, 2100, 2}, {&nest, 1100, 2101, -1},
        {&lead, 0, 0, 1}, {&lead, 2, 50, 1}, {&lead, 5, 150, 1}, {&lead, 5, 151, -1},
    };
    long wrong = 0;
    for (auto& c : cases) { n_cases++; wrong += wgshare::route(*c.sp, same_span, c.lo, c.hi) != c.want; }
    return wrong;
}

// The take rule walked the way the polling loop walks it, over every number of resident sites from none to the whole window: wgshare::take_upto
// against the rule stated by scanning - nothing while the next item's last site is not resident or fewer than min_take sites behind its first site
// are, else every item up to the first whose last site is not resident.  Every item is taken once, in order of its last site, never before that
// site is resident.  Returns the number of violations.
static long walk_take_rule(const std::vector<wgshare::Range>& items, const wgshare::Span& s, int64_t mt, long& n_subs, uint64_t& h)
{
    long bad = 0;
    std::vector<int> taken(items.size(), 0);
    size_t pos = 0;
    for (int64_t R = s.win_lo; R <= s.win_hi && pos < items.size(); R++)
        for (;;) {                                                  // (after a sub-batch the loop asks again, maybe at the same count)
            const size_t end = wgshare::take_upto(items, pos, R, mt);
            size_t want = pos;
            if (items[pos].hi <= R && R - items[pos].lo >= mt) while (want < items.size() && items[want].hi <= R) want++;
            bad += end != want;
            if (end <= pos || end > items.size()) { bad += end != pos; break; }
            for (size_t k = pos; k < end; k++) { taken[k]++; bad += items[k].hi > R || R - items[pos].lo < mt || (k && items[k].hi < items[k - 1].hi); }
            n_subs++; h = (h ^ (uint64_t)end) * 1099511628211ULL; h = (h ^ (uint64_t)R) * 1099511628211ULL;
            pos = end;
            if (pos == items.size()) break;
        }
    // what min_take still holds back when every site is resident goes when the uploader has finished: the caller's step, not the rule's
    for (size_t k = 0; k < items.size(); k++) bad += taken[k] != (k < pos ? 1 : 0);
    for (size_t k = pos; k < items.size(); k++) bad += !(s.win_hi - items[pos].lo < mt);
    return bad;
}

// The plans of the share groups (share_plan.h) over the toy worlds of main(), with positions that restart at every region: 1 to 64 shares (more
// than the 62, 54, 13 and 3 chunks of the worlds), even and weighted (one weight zero), a halo of 6000 sites and one of 10.  Every plan must
// tile the chunk grid; every chunk and every junction range of +-50 and +-5000 sites around a share boundary is routed and compared with the rule
// stated by scanning (a chunk: with its owner); the router's hand-made cases; the refusals; and the take rule.  One line.
static void share_plan_line()
{
    const struct { int n_regions; int64_t len, chunk; } worlds[4] = {{7, 40000, 5000}, {5, 30000, 3000}, {1, 9000, 700}, {3, 500, 60000}};
    const wgbsseg_params P = {15.0f, 50, 300};
    uint64_t h = 1469598103934665603ULL;
    auto fold = [&](uint64_t v) { h = (h ^ v) * 1099511628211ULL; };
    long n_plans = 0, n_chunks_routed = 0, n_routed = 0, n_unroutable = 0, n_refused = 0, bad = 0, n_idle = 0, n_hand = 0;
    bad += route_by_hand(n_hand);
    std::vector<wgshare::Span> kept;                           // world 0 over 3 shares at the large halo: the take rule's
    std::vector<wgshare::Range> kept_chunks;
    for (int w = 0; w < 4; w++) {
        std::vector<int64_t> rs, re;
        const int64_t n_sites = world_regions(worlds[w].n_regions, worlds[w].len, rs, re) - 1;
        std::vector<uint32_t> loci((size_t)n_sites);
        for (int r = 0; r < worlds[w].n_regions; r++)
            for (int64_t i = rs[(size_t)r] - 1; i < re[(size_t)r] - 1; i++) loci[(size_t)i] = (uint32_t)(100 + 13 * (i - rs[(size_t)r] + 1) + (int64_t)(mix((uint64_t)i) % 7));
        std::vector<wgshare::Range> chunks;
        for (int r = 0; r < worlds[w].n_regions; r++)
            for (int64_t s0 = rs[(size_t)r]; s0 < re[(size_t)r]; s0 += worlds[w].chunk) chunks.push_back({s0 - 1, std::min(s0 + worlds[w].chunk, re[(size_t)r]) - 1});
        for (int G : {1, 2, 3, 5, 8, 64})
            for (int weighted = 0; weighted < 2; weighted++)
                for (int64_t halo : {(int64_t)6000, (int64_t)10}) {
                    std::vector<double> wt((size_t)G);
                    for (int d = 0; d < G; d++) wt[(size_t)d] = d % 4 == 1 ? 0.0 : 0.5 + (double)(d % 3);
                    if (G == 1) wt[0] = 1.0;
                    std::vector<wgshare::Span> sp;
                    std::string msg;
                    const int rc = wgshare::plan_shares(loci.data(), n_sites, rs.data(), re.data(), worlds[w].n_regions, worlds[w].chunk, &P, G, weighted ? wt.data() : nullptr, halo, sp, msg);
                    if (rc != WGBSSEG_OK || (int)sp.size() != G) { bad++; continue; }
                    n_plans++;
                    // the shares' runs tile the grid, in order; windows: the run +- halo inside the sites, the lower edge on a multiple of 128
                    size_t c = 0;
                    for (int d = 0; d < G; d++) {
                        const wgshare::Span& s = sp[(size_t)d];
                        fold((uint64_t)s.own_lo); fold((uint64_t)s.own_hi); fold((uint64_t)s.win_lo); fold((uint64_t)s.win_hi); fold((uint64_t)s.chunks); fold((uint64_t)s.work);
                        if (!s.chunks) { n_idle++; bad += s.own_lo != s.own_hi || s.win_lo != 0 || s.win_hi != 0; continue; }
                        bad += c + (size_t)s.chunks > chunks.size() || s.own_lo != chunks[c].lo || s.own_hi != chunks[c + (size_t)s.chunks - 1].hi;
                        bad += s.win_lo % 128 != 0 || s.win_lo > std::max<int64_t>(0, s.own_lo - halo) || s.win_lo + 128 <= std::max<int64_t>(0, s.own_lo - halo);
                        bad += s.win_hi != std::min(n_sites, s.own_hi + halo);
                        c += (size_t)s.chunks;
                    }
                    bad += c != chunks.size();
                    auto route = [&](int64_t lo, int64_t hi, int owner) {
                        const int got = wgshare::route(sp, same_span, lo, hi), want = route_by_scan(sp, lo, hi);
                        bad += got != want || (owner >= 0 && got != owner);
                        if (got >= 0) bad += !(sp[(size_t)got].win_lo <= lo && hi <= sp[(size_t)got].win_hi);
                        else for (auto& o : sp) bad += o.own_lo <= lo && lo < o.own_hi && o.win_lo <= lo && hi <= o.win_hi;      // (refused: the owner does not hold it)
                        if (owner >= 0) n_chunks_routed++;
                        else (got >= 0 ? n_routed : n_unroutable)++;
                        fold((uint64_t)(int64_t)got);
                    };
                    c = 0;
                    for (int d = 0; d < G; d++)
                        for (int64_t k = 0; k < sp[(size_t)d].chunks; k++, c++) route(chunks[c].lo, chunks[c].hi, d);
                    for (int d = 0; d < G; d++) {
                        const int64_t b = sp[(size_t)d].own_hi;
                        if (!sp[(size_t)d].chunks || b == chunks.back().hi) continue;
                        for (int64_t reach : {(int64_t)50, (int64_t)5000}) route(std::max<int64_t>(0, b - reach), std::min(n_sites, b + reach), -1);
                    }
                    if (w == 0 && G == 3 && !weighted && halo == 6000) { kept = sp; kept_chunks = chunks; }
                }
        if (w == 0) {                                              // the refusals: arguments, max_bp 0, an empty region, regions out of order, a negative weight, weights all zero
            const wgbsseg_params P0 = {15.0f, 50, 0};
            const int64_t es[2] = {1, 500}, ee[2] = {500, 500}, ds[2] = {500, 1}, de[2] = {900, 500};
            const double neg[2] = {1.0, -1.0}, zero[2] = {0.0, 0.0};
            std::vector<wgshare::Span> sp;
            std::string msg;
            for (int k = 0; k < 6; k++) {
                const int rc = k == 0 ? wgshare::plan_shares(loci.data(), n_sites, rs.data(), re.data(), worlds[w].n_regions, worlds[w].chunk, &P, 0, nullptr, -1, sp, msg)
                             : k == 1 ? wgshare::plan_shares(loci.data(), n_sites, rs.data(), re.data(), worlds[w].n_regions, worlds[w].chunk, &P0, 2, nullptr, -1, sp, msg)
                             : k == 2 ? wgshare::plan_shares(loci.data(), n_sites, es, ee, 2, worlds[w].chunk, &P, 2, nullptr, -1, sp, msg)
                             : k == 3 ? wgshare::plan_shares(loci.data(), n_sites, ds, de, 2, worlds[w].chunk, &P, 2, nullptr, -1, sp, msg)
                             : wgshare::plan_shares(loci.data(), n_sites, rs.data(), re.data(), worlds[w].n_regions, worlds[w].chunk, &P, 2, k == 4 ? neg : zero, -1, sp, msg);
                n_refused += rc == WGBSSEG_E_ARG && !msg.empty();
                for (char ch : msg) fold((uint64_t)(unsigned char)ch);
            }
        }
    }
    // the take rule: the middle share's chunks, the ranges around its two boundaries and a short patch that ends where each chunk ends (ties), in
    // order of their last site (ties as they came); with the group's min_take, which holds the first sub-batch back long after its items are
    // resident, and with min_take 1 and 700, where residency is what binds
    long n_items = 0, n_subs = 0;
    if (kept.size() == 3 && kept[1].chunks) {
        const wgshare::Span& s = kept[1];
        std::vector<wgshare::Range> items;
        for (auto& c : kept_chunks) if (s.own_lo <= c.lo && c.hi <= s.own_hi) { items.push_back(c); items.push_back({c.hi - 60, c.hi}); }
        for (int64_t b : {s.own_lo, s.own_hi}) for (int64_t reach : {(int64_t)50, (int64_t)5000}) items.push_back({b - reach, b + reach});
        std::stable_sort(items.begin(), items.end(), [](const wgshare::Range& a, const wgshare::Range& b) { return a.hi < b.hi; });
        const int64_t mt = wgshare::min_take(5000, s);
        bad += mt != std::max<int64_t>(20000, (s.win_hi - s.win_lo) / 5);
        for (int64_t m : {mt, (int64_t)1, (int64_t)700}) bad += walk_take_rule(items, s, m, n_subs, h);
        n_items = (long)items.size();
    } else bad++;
    printf("share_plan: %ld plans, %ld idle shares, %ld chunks routed to their owners, %ld junction ranges routed, %ld unroutable, %ld routes by hand, %ld refusals, "
           "take rule: %ld items in %ld sub-batches of 3 walks, %ld mismatches, checksum %016llx\n",
           n_plans, n_idle, n_chunks_routed, n_routed, n_unroutable, n_hand, n_refused, n_items, n_subs, bad, (unsigned long long)h);
}

// The plans of the pat engines and of sample_stats (bimodal_plan.h, homog_plan.h, stats_plan.h) over the fixed tables of tests/test_patplan_cpu.py
// (blocks that share an endCpG, nested ones, a startCpG within 150 sites of site 1, one block alone; ranges on every residue of a 16-byte vector, empty
// ones, none, one tile of vectors and one more) and over seeded random ones; bimodal: the feed's walk - retire, drop, append one read per chunk - with
// every table read where the engine reads it, and the scratch layout of each retired group; the refusals.  One line each: counts and a checksum.
static void pat_plan_lines()
{
    uint64_t h = 1469598103934665603ULL;
    auto fold = [&](uint64_t v) { h = (h ^ v) * 1099511628211ULL; };
    auto fold_msg = [&](int rc, const std::string& m) { fold((uint64_t)(int64_t)rc); for (char ch : m) fold((uint64_t)(unsigned char)ch); };
    typedef std::vector<int64_t> V;
    std::vector<std::pair<V, V>> tables{{{400}, {420}}, {{300, 10, 250, 500}, {320, 320, 320, 501}}, {{100, 200, 210, 205, 900}, {1000, 300, 220, 206, 901}},
                                        {{1, 150, 151, 152, 700}, {5, 160, 400, 153, 800}}, {{5, 2147483646}, {9, 2147483647}}};
    for (uint64_t k = 0; k < 200; k++) {
        const int64_t n_sites = 30 + (int64_t)(mix(k * 3 + 1) % 3000), nb = 1 + (int64_t)(mix(k * 3 + 2) % 40);
        V s((size_t)nb), e((size_t)nb);
        for (int64_t j = 0; j < nb; j++) { s[(size_t)j] = 1 + (int64_t)(mix(k * 1000 + (uint64_t)j) % (uint64_t)n_sites); e[(size_t)j] = s[(size_t)j] + 1 + (int64_t)(mix(k * 2000 + (uint64_t)j) % (k % 3 ? 30 : 1500)); }
        if (nb > 2) e[1] = e[0] > s[1] ? e[0] : e[1];
        tables.push_back({s, e});
    }
    // ---- bimodal
    long n_ok = 0, n_refused = 0, n_retired = 0, bad = 0;
    for (auto& t : tables) {
        BimodalPlan p;
        std::string msg;
        const int64_t nb = (int64_t)t.first.size();
        if (plan_bimodal(t.first.data(), t.second.data(), nb, 1, n_ok % 3 == 0 ? -1 : 16, p, msg) != WGBSSEG_OK) { bad++; continue; }
        n_ok++;
        for (int64_t j = 0; j < nb; j++) { fold((uint64_t)p.by_end[(size_t)j]); fold((uint64_t)p.lo_after[(size_t)j]); }
        int64_t pending = 0;
        long long last = WG_BIM_NONE;
        const long long hi = t.second[(size_t)p.by_end[(size_t)nb - 1]] + 2, step = hi > 100000 ? hi / 997 : 1 + (long long)(mix((uint64_t)nb) % 7);
        for (long long start = 1;; start += step) {                                  // one read per chunk, starts ascending past the last endCpG
            const int64_t p1 = start > hi ? nb : p.retire_upto(pending, last);
            bad += p1 < pending || p1 > nb;
            if (p1 > pending) {
                std::vector<wg_bim_meta> meta((size_t)(p1 - pending));
                std::vector<long long> off(meta.size());
                for (size_t g = 0; g < meta.size(); g++) meta[g] = {0, 0, 0, (long long)(mix((uint64_t)(pending + (int64_t)g)) % 600), (long long)(g % 3), 0};
                size_t used = 0;
                bad += wg_bim_scratch_layout(meta.data(), p.by_end.data() + pending, p1 - pending, p.lds_cols, off.data(), used, msg) != WGBSSEG_OK;
                for (long long o : off) fold((uint64_t)o);
                fold((uint64_t)used);
                n_retired += (long)(p1 - pending);
            }
            pending = p1;
            fold((uint64_t)p.drop_below(pending));
            if (start > hi) break;
            last = start;
        }
        bad += pending != nb;
    }
    {
        const int64_t s[2] = {5, 0}, e[2] = {9, 4};
        BimodalPlan p;
        std::string msg;
        for (int k = 0; k < 4; k++) {
            const int rc = k == 0 ? plan_bimodal(s, e, 0, 1, -1, p, msg) : k == 1 ? plan_bimodal(nullptr, e, 2, 1, -1, p, msg) : k == 2 ? plan_bimodal(s, e, 2, 0, -1, p, msg) : plan_bimodal(s, e, 2, 1, -1, p, msg);
            n_refused += rc == WGBSSEG_E_ARG && !msg.empty();
            fold_msg(rc, msg);
        }
        const wg_bim_meta m[2] = {{0, 0, 0, 300, 5, 0}, {0, 0, 0, 300, 1ll << 31, 0}};
        const int32_t ids[2] = {3, 8};
        long long off[2];
        size_t used = 0;
        const int rc = wg_bim_scratch_layout(m, ids, 2, 16, off, used, msg);
        n_refused += rc == WGBSSEG_E_CAPACITY;
        fold_msg(rc, msg);
        for (int64_t n : {(int64_t)1, (int64_t)5, (int64_t)6, (int64_t)4096, (int64_t)1 << 40}) { const BimodalChunkBound ub(n); fold(ub.lines); fold(ub.words); }
    }
    printf("bimodal_plan: %ld plans, %ld blocks retired, %ld refusals, %ld mismatches, checksum %016llx\n", n_ok, n_retired, n_refused, bad, (unsigned long long)h);
    // ---- homog: the same tables in (startCpG, endCpG) order
    h = 1469598103934665603ULL; n_ok = n_refused = bad = 0;
    const float edges[4] = {0.0f, 0.25f, 0.75f, 1.0f}, flat[4] = {0.0f, 0.5f, 0.5f, 1.0f};
    for (auto& t : tables) {
        std::vector<std::pair<int64_t, int64_t>> rows;
        for (size_t j = 0; j < t.first.size(); j++) rows.push_back({t.first[j], t.second[j]});
        std::sort(rows.begin(), rows.end());
        V s, e;
        for (auto& r : rows) { s.push_back(r.first); e.push_back(r.second); }
        HomogPlan p;
        std::string msg;
        if (plan_homog(s.data(), e.data(), (int64_t)s.size(), edges, 3, 1, p, msg) != WGBSSEG_OK) { bad++; continue; }
        n_ok++;
        for (size_t j = 0; j < s.size(); j++) { fold((uint64_t)p.s32[j]); fold((uint64_t)p.e32[j]); fold((uint64_t)p.pmax[j]); bad += p.pmax[j] < p.e32[j] || (j && p.pmax[j] < p.pmax[j - 1]); }
        fold((uint64_t)p.last_end);
    }
    {
        const int64_t s[2] = {5, 3}, e[2] = {9, 4}, z[2] = {0, 3}, r[2] = {5, 6}, re[2] = {5, 1ll << 31};
        HomogPlan p;
        std::string msg;
        for (int k = 0; k < 8; k++) {
            const int rc = k == 0 ? plan_homog(s, e, 0, edges, 3, 1, p, msg) : k == 1 ? plan_homog(s, e, 1, nullptr, 3, 1, p, msg) : k == 2 ? plan_homog(s, e, 1, edges, 9, 1, p, msg)
                         : k == 3 ? plan_homog(s, e, 1, flat, 3, 1, p, msg) : k == 4 ? plan_homog(s, e, 1, edges, 3, 0, p, msg) : k == 5 ? plan_homog(z, e, 2, edges, 3, 1, p, msg)
                         : k == 6 ? plan_homog(r, re, 2, edges, 3, 1, p, msg) : plan_homog(s, e, 2, edges, 3, 1, p, msg);
            n_refused += rc == WGBSSEG_E_ARG && !msg.empty();
            fold_msg(rc, msg);
        }
    }
    printf("homog_plan: %ld plans, %ld refusals, %ld mismatches, checksum %016llx\n", n_ok, n_refused, bad, (unsigned long long)h);
    // ---- sample_stats: both row widths
    h = 1469598103934665603ULL; n_ok = n_refused = bad = 0;
    std::vector<std::pair<V, V>> ranges{{{}, {}}, {{0, 5, 5, 1000}, {0, 5, 5, 1000}}, {{0, 4}, {4, 8}}, {{0}, {WG_ST_TILE * 8}}, {{0}, {WG_ST_TILE * 8 + 1}}, {{3, 90000}, {3 + WG_ST_TILE * 4 - 4, 90001}}};
    for (int64_t a = 0; a < 16; a++) for (int64_t b = a; b <= 33; b++) ranges.push_back({{a, b, b}, {b, b, 34}});
    for (uint64_t k = 0; k < 200; k++) {
        V cuts;
        for (uint64_t j = 0; j < 2 * (mix(k + 77) % 25); j++) cuts.push_back((int64_t)(mix(k * 100 + j) % 40001));
        std::sort(cuts.begin(), cuts.end());
        V a, b;
        for (size_t j = 0; j + 1 < cuts.size(); j += 2) { a.push_back(cuts[j]); b.push_back(cuts[j + 1]); }
        ranges.push_back({a, b});
    }
    for (auto& t : ranges)
        for (int elem = 1; elem <= 2; elem++) {
            StatsPlan p;
            std::string msg;
            if (plan_sample_stats(t.first.data(), t.second.data(), (int64_t)t.first.size(), 1 << 20, elem, 3, p, msg) != WGBSSEG_OK) { bad++; continue; }
            n_ok++;
            const StatsPlan::View<const int64_t> v = p.view((const int64_t*)p.upload.data());
            for (int64_t i = 0; i < p.n_ranges; i++) { fold((uint64_t)v.x0[i]); fold((uint64_t)v.x1[i]); fold((uint64_t)v.cumv[i]); bad += v.cumv[i + 1] < v.cumv[i]; }
            bad += v.cumv[p.n_ranges] != p.n_vec || p.upload.size() != (size_t)p.n_ranges * 3 + 1;
            fold((uint64_t)p.n_sites); fold((uint64_t)p.n_vec); fold((uint64_t)p.n_tiles);
        }
    {
        const int64_t a[2] = {0, 3}, b[2] = {4, 9}, neg[1] = {-1}, big[1] = {(1ll << 20) + 1};
        StatsPlan p;
        std::string msg;
        for (int k = 0; k < 6; k++) {
            const int rc = k == 0 ? plan_sample_stats(a, b, -1, 1 << 20, 1, 3, p, msg) : k == 1 ? plan_sample_stats(nullptr, b, 2, 1 << 20, 1, 3, p, msg)
                         : k == 2 ? plan_sample_stats(neg, b, 1, 1 << 20, 1, 3, p, msg) : k == 3 ? plan_sample_stats(a, big, 1, 1 << 20, 2, 3, p, msg)
                         : k == 4 ? plan_sample_stats(a, b, 2, 1 << 20, 1, 3, p, msg) : plan_sample_stats(a, b, 1, 1 << 20, 1, 65536, p, msg);
            n_refused += rc == WGBSSEG_E_ARG && !msg.empty();
            fold_msg(rc, msg);
        }
    }
    printf("stats_plan: %ld plans, %ld refusals, %ld mismatches, checksum %016llx\n", n_ok, n_refused, bad, (unsigned long long)h);
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: san_host <threads> <out.bed>\n"); return 2; }
    setenv("WGBSSEG_STITCH_THREADS", argv[1], 1);
    block_plan_line();
    share_plan_line();
    pat_plan_lines();
    std::vector<int64_t> s, e;
    for (int rep = 0; rep < 3; rep++) {                                      // the pool is reused across calls
        std::vector<int64_t> s1, e1;
        run_world(7, 40000, 5000, 0, true, s1, e1);                          // every first attempt agrees
        run_world(5, 30000, 3000, 40, true, s1, e1);                         // left edges disagree: doubling, follow-up batches
        run_world(5, 30000, 3000, 40, false, s1, e1);                        // the same without speculation
        run_world(1, 9000, 700, 200, true, s1, e1);                          // one region, patches that grow past a chunk
        run_world(3, 500, 60000, 0, true, s, e);                             // single-chunk regions (s, e: the blocks written below)
    }
    {   // the stitcher's open-addressing table (round 5) against std::map: inserts that force it to grow, updates, hits and misses, then concurrent readers
        wgstitch::SiteTable<int64_t> tab(4);
        std::map<wgstitch::Sites, int64_t> ref;
        uint64_t x = 12345;
        long bad = 0;
        for (int i = 0; i < 60000; i++) {
            x = mix(x + (uint64_t)i);
            const wgstitch::Sites k((int64_t)(x % 5000) + 1, (int64_t)(x % 5000) + 1 + (int64_t)((x >> 20) % 300));
            if ((x >> 40) % 3 == 0) { tab[k] = (int64_t)i; ref[k] = (int64_t)i; }
            else {
                const int64_t* f = tab.find(k);
                auto it = ref.find(k);
                bad += (f == nullptr) != (it == ref.end()) || (f && *f != it->second) || tab.count(k) != (ref.count(k) != 0);
            }
        }
        std::vector<std::thread> th;
        std::vector<long> miss((size_t)4, 0);
        for (int t = 0; t < 4; t++) th.emplace_back([&, t] { for (auto& kv : ref) { const int64_t* f = tab.find(kv.first); miss[(size_t)t] += !f || *f != kv.second; } });
        for (auto& t : th) t.join();
        printf("sitetable: %zu keys, mismatches %ld, concurrent misses %ld\n", ref.size(), bad, miss[0] + miss[1] + miss[2] + miss[3]);
    }
    // BED rows of the last world's blocks on a toy genome of 3 chromosomes
    const int64_t n_sites = 2000;
    std::vector<uint32_t> loci((size_t)n_sites);
    for (int64_t i = 0; i < n_sites; i++) loci[(size_t)i] = (uint32_t)(100 + 13 * i + (mix((uint64_t)i) % 7));
    const int64_t cum[3] = {700, 1500, 2000};
    const char* names[3] = {"chr1", "chr2", "chrX"};
    wgadd::Genome g = {loci.data(), n_sites, cum, names, 3};
    std::vector<int64_t> bs, be;
    for (size_t i = 0; i < s.size(); i++) if (e[i] <= n_sites + 1 && wgadd::loc2chrom(g, s[i]) == wgadd::loc2chrom(g, e[i] - 1)) { bs.push_back(s[i]); be.push_back(e[i]); }
    FILE* fp = fopen(argv[2], "wb");
    if (!fp) return 3;
    std::string err;
    const int rc = wgadd::add_loci(g, bs.data(), be.data(), (int64_t)bs.size(), fp, atoi(argv[1]), err);
    fclose(fp);
    printf("add_loci: %zu rows, rc %d %s\n", bs.size(), rc, err.c_str());
    {   // the same genome's rows straight from border lists (three regions = the chromosomes, one of them without a block), min_cpg 1 and 3
        std::vector<int32_t> flat;
        std::vector<int64_t> off{0};
        const int64_t lo[3] = {1, 701, 1501}, hi[3] = {701, 1501, 2001};
        for (int r = 0; r < 3; r++) {
            if (r != 1) for (int64_t b = lo[r]; b < hi[r]; b += 1 + (int64_t)(mix((uint64_t)b) % 9)) flat.push_back((int32_t)b);
            if (r != 1) flat.push_back((int32_t)hi[r]);
            off.push_back((int64_t)flat.size());
        }
        for (int64_t mc : {(int64_t)1, (int64_t)3}) {
            wgadd::BorderRows rows{flat.data(), off.data(), 3, mc, {}};
            rows.index();
            FILE* nul = fopen("/dev/null", "wb");
            std::string m;
            int64_t written = 0;
            const int r3 = wgadd::add_loci_rows(g, rows, rows.total(), nul, atoi(argv[1]), m, &written);
            fclose(nul);
            printf("add_loci from borders, min_cpg %lld: %lld of %lld blocks written, rc %d %s\n", (long long)mc, (long long)written, (long long)rows.total(), r3, m.c_str());
        }
    }
    // and its refusals
    const int64_t bad_s[3] = {5, 0, 1999}, bad_e[3] = {3, 4, 2003};
    for (int i = 0; i < 3; i++) {
        FILE* nul = fopen("/dev/null", "wb");
        std::string m;
        const int r2 = wgadd::add_loci(g, bad_s + i, bad_e + i, 1, nul, 1, m);
        fclose(nul);
        printf("add_loci bad row %d: rc %d %s\n", i, r2, m.c_str());
    }
    // the block tools' text paths (table_io.h): a table with a header, comments, NA fields and no last newline through the parser,
    // the sharded writers (file: pwrite side by side; a pipe-like descriptor: in order) and the number formatter
    {
        std::string text = "chr\tstart\tend\tstartCpG\tendCpG\n# c\n\n";
        const int64_t n_rows = 40000;
        for (int64_t i = 0; i < n_rows; i++) {
            char row[96];
            if (i % 97 == 5) snprintf(row, sizeof row, "chr%d\t%lld\t%lld\tNA\t\n", (int)(1 + i % 22), (long long)(10 * i), (long long)(10 * i + 7));
            else snprintf(row, sizeof row, "chr%d\t%lld\t%lld\t%lld\t%lld\textra\n", (int)(1 + i % 22), (long long)(10 * i), (long long)(10 * i + 7), (long long)(1 + 2 * i), (long long)(3 + 2 * i));
            text += row;
        }
        text.pop_back();
        std::vector<int64_t> lo((size_t)n_rows + 8), sc((size_t)n_rows + 8), ec((size_t)n_rows + 8);
        std::vector<int32_t> l3((size_t)n_rows + 8);
        std::vector<uint8_t> na((size_t)n_rows + 8);
        int64_t got = 0;
        const int prc = wgtab::parse_blocks(text.data(), (int64_t)text.size(), -1, n_rows + 8, lo.data(), l3.data(), sc.data(), ec.data(), na.data(), &got);
        int64_t n_na = 0;
        for (int64_t i = 0; i < got; i++) n_na += na[(size_t)i];
        printf("parse_blocks: rc %d rows %lld na %lld, row 1 = [%lld, %lld)\n", prc, (long long)got, (long long)n_na, (long long)sc[1], (long long)ec[1]);
        const std::string bad = "chr1\t1\t2\t3.5\t4\n";
        printf("parse_blocks on a float field: rc %d\n", wgtab::parse_blocks(bad.data(), (int64_t)bad.size(), -1, 4, lo.data(), l3.data(), sc.data(), ec.data(), na.data(), &got));
        wgtab::parse_blocks(text.data(), (int64_t)text.size(), -1, n_rows + 8, lo.data(), l3.data(), sc.data(), ec.data(), na.data(), &got);
        const int64_t n_cols = 5;
        std::vector<double> vals((size_t)(got * n_cols));
        for (size_t i = 0; i < vals.size(); i++) vals[i] = (mix(i) % 13 == 0) ? std::nan("") : (mix(i) % 11 == 0 ? 1.5e300 : (double)(mix(i) % 100001) / 100000.0);
        const wgtab::Rows R = {text.data(), lo.data(), l3.data(), sc.data(), ec.data(), na.data()};
        std::string tpath = std::string(argv[2]) + ".table";
        uint64_t h = 1469598103934665603ULL;
        for (int pass = 0; pass < 2; pass++) {                                // 0: regular file, 1: in order (the way a pipe is written)
            const int fd = open(tpath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
            std::string m;
            const int wrc = wgtab::write_table(fd, pass ? -1 : 0, R, got, vals.data(), n_cols, n_cols, 3, atoi(argv[1]), m);
            close(fd);
            FILE* f = fopen(tpath.c_str(), "rb");
            uint64_t hh = 1469598103934665603ULL;
            int ch;
            long bytes = 0;
            while ((ch = fgetc(f)) != EOF) { hh = (hh ^ (uint64_t)ch) * 1099511628211ULL; bytes++; }
            fclose(f);
            printf("write_table pass %d: rc %d %s, %ld bytes, checksum %016llx%s\n", pass, wrc, m.c_str(), bytes, (unsigned long long)hh, pass && hh != h ? " DIFFERS" : "");
            h = hh;
        }
        std::vector<uint16_t> mc((size_t)got * 2);
        for (int64_t i = 0; i < got; i++) { mc[(size_t)(2 * i + 1)] = (uint16_t)(mix((uint64_t)i) % 65536); mc[(size_t)(2 * i)] = (uint16_t)(mc[(size_t)(2 * i + 1)] * (mix((uint64_t)i + 7) % 101) / 100); }
        const int fd = open(tpath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        std::string m;
        const int brc = wgtab::write_bedgraph<uint16_t>(fd, 0, R, got, mc.data(), atoi(argv[1]), m);
        close(fd);
        printf("write_bedgraph: rc %d %s\n", brc, m.c_str());
        // `convert -L`: a BED table with a text, an integer and a strand column, unknown chromosomes, blank lines
        std::string bed = "\n";
        const char* cn[3] = {"chr1", "chr2", "chrX"};
        const int64_t nb = 50000;
        for (int64_t i = 0; i < nb; i++) {
            char row[128];
            snprintf(row, sizeof row, "%s\t%lld\t%lld\t%s%lld\t%lld\t%c\n", i % 211 == 3 ? "chrUn" : cn[i % 3], (long long)(100 + 7 * i), (long long)(300 + 7 * i),
                     i % 5 ? "n" : "NA", (long long)(i % 5 ? i : 0), (long long)(i % 1000), i % 2 ? '+' : '-');
            if (i % 5 == 0) { std::string r2 = row; const size_t k = r2.find("NA0"); r2.replace(k, 3, "NA"); bed += r2; } else bed += row;
        }
        std::vector<int64_t> blo((size_t)nb + 4), bs((size_t)nb + 4), be((size_t)nb + 4);
        std::vector<int32_t> bl3((size_t)nb + 4), brl((size_t)nb + 4), bci((size_t)nb + 4);
        int64_t bn = 0;
        int32_t bw = 0;
        const int brc2 = wgtab::parse_bed(bed.data(), (int64_t)bed.size(), nb + 4, cn, 3, blo.data(), bl3.data(), brl.data(), bci.data(), bs.data(), be.data(), &bn, &bw);
        int64_t unknown = 0;
        for (int64_t i = 0; i < bn; i++) unknown += bci[(size_t)i] < 0;
        printf("parse_bed: rc %d rows %lld width %d unknown %lld\n", brc2, (long long)bn, (int)bw, (long long)unknown);
        const std::string fl = "chr1\t1\t2\t0.50\n";          // comes back as 0.5: not this path's
        printf("parse_bed on a float column: rc %d\n", wgtab::parse_bed(fl.data(), (int64_t)fl.size(), 4, cn, 3, blo.data(), bl3.data(), brl.data(), bci.data(), bs.data(), be.data(), &bn, &bw));
        wgtab::parse_bed(bed.data(), (int64_t)bed.size(), nb + 4, cn, 3, blo.data(), bl3.data(), brl.data(), bci.data(), bs.data(), be.data(), &bn, &bw);
        std::vector<int64_t> cs((size_t)bn), ce((size_t)bn);
        for (int64_t i = 0; i < bn; i++) { cs[(size_t)i] = bci[(size_t)i] < 0 ? 0 : 1 + i; ce[(size_t)i] = bci[(size_t)i] < 0 ? 0 : 4 + i; }
        const int fd2 = open(tpath.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0666);
        const int arc = wgtab::write_annotated_bed(fd2, 0, bed.data(), blo.data(), bl3.data(), brl.data(), cs.data(), ce.data(), bn, atoi(argv[1]), m);
        close(fd2);
        FILE* f2 = fopen(tpath.c_str(), "rb");
        uint64_t h2 = 1469598103934665603ULL;
        int ch2;
        long bytes2 = 0;
        while ((ch2 = fgetc(f2)) != EOF) { h2 = (h2 ^ (uint64_t)ch2) * 1099511628211ULL; bytes2++; }
        fclose(f2);
        printf("write_annotated_bed: rc %d %s, %ld bytes, checksum %016llx\n", arc, m.c_str(), bytes2, (unsigned long long)h2);
        unlink(tpath.c_str());
    }
    return 0;
}
