// row_engines.h — the calls that work on the context's resident rows (wgbsseg_block_sums, _marker_stats, _sample_stats, _merge_rows, _pair_ranges,
// _pair_hist, _beta2bed, _beta2bed_bgzf, _convert_regions, _site_counts, _site_table), the stand-alone wgbsseg_bgzf_deflate, the helpers they share and their extern "C" entry points.  Part of wgbsseg.hip, which includes
// it once set_err, HIP_TRY, the owners and the context are in scope; what a call decides on the host is in block_plan.h, stats_plan.h, merge_plan.h,
// pair_plan.h, bed_plan.h and array_plan.h, this file stages, launches and fetches.
#pragma once

namespace {

// what a call on the resident rows begins with; -> WGBSSEG_OK (0) or the refusal
int need_rows(const wgbsseg_ctx* c, char* err, size_t errlen)
{
    if (!c) { set_err(err, errlen, "ctx is NULL"); return WGBSSEG_E_ARG; }
    if (!c->betas) { set_err(err, errlen, "betas not set"); return WGBSSEG_E_STATE; }
    return WGBSSEG_OK;
}

// f(std::integral_constant<int, ELEM>) for the bytes per count of the resident rows: the one place that turns `elem` into a template argument
template <class F>
void by_elem(int32_t elem, F&& f)
{
    if (elem == 1) f(std::integral_constant<int, 1>()); else f(std::integral_constant<int, 2>());
}

// The timed tail of an auxiliary call (block_sums, marker_stats, sample_stats, convert_regions): begin() in front of its launches on stream A;
// end() behind them brings the results home, waits, and leaves the launches' device time where wgbsseg_last_block_sums_ms reads it.
struct AuxClock {
    wgbsseg_ctx* c;
    struct Fetch { void* dst; const void* src; size_t bytes; };
    hipError_t begin() const { return hipEventRecord(c->ev[0], c->sA); }
    hipError_t end(std::initializer_list<Fetch> home) const
    {
        hipError_t e = hipEventRecord(c->ev[1], c->sA);
        for (const Fetch& f : home) if (e == hipSuccess) e = hipMemcpyAsync(f.dst, f.src, f.bytes, hipMemcpyDeviceToHost, c->sA);
        if (e == hipSuccess) e = hipStreamSynchronize(c->sA);
        float ms = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev[0], c->ev[1]);
        if (e == hipSuccess) c->last_block_sums_ms = ms;
        return e;
    }
};

using BlockSumTables = BlockSumPlan::View<const int32_t>;      // a plan's tables on the device (bs_plan)

// uint8 rows, a table ordered by first and last site: the descriptors of every block once (prep), the streamed pass, and a wavefront
// per (block, sample) for the blocks the ring cannot serve
int launch_block_sums_streaming(wgbsseg_ctx* c, const BlockSumPlan& p, const BlockSumTables& d, int mode, uint32_t min_cov, char* err, size_t errlen)
{
    const int64_t n_blocks = p.n_blocks;
    int32_t* dd1 = c->bs_desc.as<int32_t>();
    int32_t* dd0 = dd1 + n_blocks;
    int32_t* drr = dd0 + n_blocks;
    hipLaunchKernelGGL(k_block_sums_prep, dim3((unsigned)((n_blocks + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, c->sA, d.x0, d.x1, d.perm, n_blocks, p.n_tiles, dd1, dd0, drr);
    HIP_TRY(hipGetLastError());
    const unsigned gy = (unsigned)((c->n_samples + 3) / 4);
    const dim3 grid((unsigned)((p.n_tiles + WG_BSR_RUN - 1) / WG_BSR_RUN), gy);
#define WG_LAUNCH_BSR(M) hipLaunchKernelGGL(k_block_sums_run<M>, grid, dim3(WG_BLOCK), 0, c->sA, c->betas, c->pitch, c->n_total, dd1, dd0, drr, d.tile_first, \
                                            p.n_tiles, n_blocks, (int)c->n_samples, min_cov, c->bs_out.p)
    if (mode == 0) WG_LAUNCH_BSR(0); else if (mode == 1) WG_LAUNCH_BSR(1); else if (mode == 2) WG_LAUNCH_BSR(2); else WG_LAUNCH_BSR(3);
#undef WG_LAUNCH_BSR
    HIP_TRY(hipGetLastError());
    if (p.n_direct)
        hipLaunchKernelGGL(k_block_sums_direct, dim3((unsigned)p.n_direct, gy), dim3(WG_BLOCK), 0, c->sA, c->betas, c->pitch, c->n_total, d.x0, d.x1, d.perm,
                           d.direct, p.n_direct, n_blocks, (int)c->n_samples, mode, min_cov, c->bs_out.p);
    HIP_TRY(hipGetLastError());
    return WGBSSEG_OK;
}

// every other table and uint16 rows: tiles of WG_BS_TILE sites, 4 x spw samples per workgroup
int launch_block_sums_general(wgbsseg_ctx* c, const BlockSumPlan& p, const BlockSumTables& d, int spw, unsigned gy, int mode, uint32_t min_cov, char* err, size_t errlen)
{
    const int64_t gx = (p.n_tiles + WG_BS_RUN - 1) / WG_BS_RUN;
    by_elem(c->elem, [&](auto E) {
        hipLaunchKernelGGL(k_block_sums<decltype(E)::value>, dim3((unsigned)gx, gy), dim3(WG_BLOCK), 0, c->sA, c->betas, c->pitch, c->n_total,
                           d.x0, d.x1, d.perm, d.tile_first, p.n_tiles, p.n_blocks, (int)c->n_samples, spw, mode, min_cov, c->bs_out.p);
    });
    HIP_TRY(hipGetLastError());
    return WGBSSEG_OK;
}

// what both pair calls begin with: the checks of pair_plan.h, then the pair list on the device (a | b)
int pair_list_up(wgbsseg_ctx* c, const char* who, const int32_t* a, const int32_t* b, int64_t n_pairs, int32_t min_cov, char* err, size_t errlen)
{
    std::string msg;
    if (!wg_pair_check_list(who, a, b, n_pairs, min_cov, c->n_samples, c->n_total, msg)) { set_err(err, errlen, "%s", msg.c_str()); return WGBSSEG_E_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->ph_pairs.ensure((size_t)n_pairs * 8));
    HIP_TRY(hipMemcpyAsync(c->ph_pairs.p, a, (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->sA));
    HIP_TRY(hipMemcpyAsync(c->ph_pairs.as<int32_t>() + n_pairs, b, (size_t)n_pairs * 4, hipMemcpyHostToDevice, c->sA));
    return WGBSSEG_OK;
}

}  // namespace

extern "C" {

// plan (block_plan.h) -> upload -> launches -> fetch
int wgbsseg_block_sums(wgbsseg_ctx* c, const int64_t* start0, const int64_t* end0, int64_t n_blocks, int32_t mode,
                       uint32_t min_cov, void* out, char* err, size_t errlen)
{
    if (const int rc = need_rows(c, err, errlen)) return rc;
    if (n_blocks > 0 && !out) { set_err(err, errlen, "bad arguments to block_sums"); return WGBSSEG_E_ARG; }
    BlockSumPlan p;
    std::string msg;
    int rc = plan_block_sums(start0, end0, n_blocks, c->n_total, c->elem, mode, c->bs_general, p, msg);      // (bs_general: WGBSSEG_BLOCK_SUMS_GENERAL=1, tests)
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    if (n_blocks == 0) return WGBSSEG_OK;
    // samples per wavefront of the general kernel (it keeps two tiles of each in registers, one being reduced, one in flight)
    const int spw = (c->elem == 1 && c->n_samples > 4) ? 2 : 1;
    const unsigned gy = (unsigned)((c->n_samples + 4 * spw - 1) / (4 * spw));
    if (gy > 65535) { set_err(err, errlen, "too many samples for one block_sums call"); return WGBSSEG_E_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    const size_t esz = mode == 0 ? 8 : (mode == 1 ? 2 : (mode == 2 ? 4 : 8));
    const size_t obytes = (size_t)c->n_samples * (size_t)n_blocks * esz;
    c->table_blocks = 0;                                         // bs_out is about to change
    HIP_TRY(c->bs_plan.ensure(p.upload.size() * 4));
    HIP_TRY(c->bs_out.ensure(obytes));
    if (p.monotone) HIP_TRY(c->bs_desc.ensure((size_t)n_blocks * 12));
    HIP_TRY(hipMemcpyAsync(c->bs_plan.p, p.upload.data(), p.upload.size() * 4, hipMemcpyHostToDevice, c->sA));
    const BlockSumTables d = p.view(c->bs_plan.as<const int32_t>());
    const AuxClock clock{c};
    HIP_TRY(clock.begin());
    if (p.monotone) rc = launch_block_sums_streaming(c, p, d, mode, min_cov, err, errlen);
    else rc = launch_block_sums_general(c, p, d, spw, gy, mode, min_cov, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    HIP_TRY(clock.end({{out, c->bs_out.p, obytes}}));
    c->last_valid = false;
    c->table_blocks = mode == 3 ? n_blocks : 0;
    return WGBSSEG_OK;
}

int wgbsseg_marker_stats(wgbsseg_ctx* c, const int32_t* tg, int32_t n_tg, const int32_t* bg, int32_t n_bg, int64_t n_blocks, double* out,
                         char* err, size_t errlen)
{
    if (!c || !tg || !bg || n_tg < 1 || n_bg < 1 || !out || n_blocks < 1) { set_err(err, errlen, "bad arguments to marker_stats"); return WGBSSEG_E_ARG; }
    if (c->table_blocks != n_blocks) { set_err(err, errlen, "marker_stats: the last wgbsseg_block_sums call was not a mode-3 reduction over these %lld blocks", (long long)n_blocks); return WGBSSEG_E_STATE; }
    for (int i = 0; i < n_tg; i++) if (tg[i] < 0 || tg[i] >= c->n_samples) { set_err(err, errlen, "marker_stats: no sample %d", (int)tg[i]); return WGBSSEG_E_ARG; }
    for (int i = 0; i < n_bg; i++) if (bg[i] < 0 || bg[i] >= c->n_samples) { set_err(err, errlen, "marker_stats: no sample %d", (int)bg[i]); return WGBSSEG_E_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->mk_out.ensure((size_t)n_blocks * 64 + (size_t)(n_tg + n_bg) * 4));
    double* dout = c->mk_out.as<double>();
    int32_t* dtg = reinterpret_cast<int32_t*>(dout + n_blocks * 8);
    int32_t* dbg = dtg + n_tg;
    HIP_TRY(hipMemcpyAsync(dtg, tg, (size_t)n_tg * 4, hipMemcpyHostToDevice, c->sA));
    HIP_TRY(hipMemcpyAsync(dbg, bg, (size_t)n_bg * 4, hipMemcpyHostToDevice, c->sA));
    const AuxClock clock{c};
    HIP_TRY(clock.begin());
    hipLaunchKernelGGL(k_marker_stats, dim3((unsigned)(((n_blocks + 1) / 2 + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, c->sA, c->bs_out.as<double>(), n_blocks,      // (two blocks per thread)
                       dtg, (int)n_tg, dbg, (int)n_bg, dout);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.end({{out, dout, (size_t)n_blocks * 64}}));
    return WGBSSEG_OK;
}

double wgbsseg_last_block_sums_ms(const wgbsseg_ctx* c) { return c ? c->last_block_sums_ms : 0.0; }

static_assert(sizeof(wgbsseg_sample_stat) == sizeof(wg_sample_stat) && sizeof(wg_sample_stat) == 72, "wgbsseg_sample_stat is the kernels' wg_sample_stat");

// plan (stats_plan.h) -> upload -> two launches -> fetch
int wgbsseg_sample_stats(wgbsseg_ctx* c, const int64_t* start0, const int64_t* end0, int64_t n_ranges, int32_t depth_at,
                         wgbsseg_sample_stat* out, char* err, size_t errlen)
{
    if (const int rc = need_rows(c, err, errlen)) return rc;
    if (!out) { set_err(err, errlen, "bad arguments to sample_stats"); return WGBSSEG_E_ARG; }
    StatsPlan p;
    std::string msg;
    const int rc = plan_sample_stats(start0, end0, n_ranges, c->n_total, c->elem, c->n_samples, p, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    if (p.n_vec == 0) {                                          // nothing to read: no ranges, or empty ones only
        memset(out, 0, sizeof(*out) * (size_t)c->n_samples);
        c->last_block_sums_ms = 0.0;
        return WGBSSEG_OK;
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t part_bytes = (size_t)p.n_tiles * (size_t)c->n_samples * sizeof(wg_stat_part);
    HIP_TRY(c->st_ranges.ensure(p.upload.size() * 8));
    HIP_TRY(c->st_parts.ensure(part_bytes + (size_t)c->n_samples * sizeof(wg_sample_stat)));
    HIP_TRY(hipMemcpyAsync(c->st_ranges.p, p.upload.data(), p.upload.size() * 8, hipMemcpyHostToDevice, c->sA));
    const StatsPlan::View<const int64_t> d = p.view(c->st_ranges.as<const int64_t>());
    wg_stat_part* dparts = c->st_parts.as<wg_stat_part>();
    wg_sample_stat* dout = reinterpret_cast<wg_sample_stat*>(c->st_parts.as<uint8_t>() + part_bytes);
    const dim3 grid((unsigned)p.n_tiles, (unsigned)c->n_samples);
    const AuxClock clock{c};
    HIP_TRY(clock.begin());
    by_elem(c->elem, [&](auto E) {
        hipLaunchKernelGGL(k_sample_stats<decltype(E)::value>, grid, dim3(WG_ST_BLOCK), 0, c->sA, c->betas, c->pitch, d.x0, d.x1, d.cumv, n_ranges, p.n_vec, depth_at, dparts, p.n_tiles);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sample_stats_fold, dim3((unsigned)c->n_samples), dim3(WG_ST_BLOCK), 0, c->sA, dparts, p.n_tiles, (uint64_t)p.n_sites, dout);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.end({{out, dout, sizeof(*out) * (size_t)c->n_samples}}));
    return WGBSSEG_OK;
}

// plan (merge_plan.h) -> the row list up -> one launch -> the summed row home in slabs through the two page-locked text buffers of beta2bed:
// while the host copies slab k out of one, slab k+1 arrives in the other
int wgbsseg_merge_rows(wgbsseg_ctx* c, const int32_t* samples, int32_t n_samples, int32_t lbeta_out, void* out, char* err, size_t errlen)
{
    if (const int rc = need_rows(c, err, errlen)) return rc;
    MergePlan p;
    std::string msg;
    const int rc = plan_merge_rows(samples, n_samples, c->n_samples, c->n_total, c->elem, lbeta_out, out, p, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->mg_samples.ensure((size_t)n_samples * 4));
    HIP_TRY(c->mg_out.ensure((size_t)p.out_bytes));
    const size_t slab = (size_t)wg_merge_slab_len(p.out_bytes, 0);
    for (auto& h : c->bed.home) if (!h.ensure(slab)) { set_err(err, errlen, "merge_rows: out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    HIP_TRY(hipMemcpyAsync(c->mg_samples.p, samples, (size_t)n_samples * 4, hipMemcpyHostToDevice, c->sA));
    HIP_TRY(hipEventRecord(c->ev[0], c->sA));
    const dim3 grid((unsigned)p.groups), block(WG_MG_BLOCK);
    by_elem(c->elem, [&](auto E) {
        constexpr int ELEM = decltype(E)::value;
        const auto k = lbeta_out ? k_beta_merge<ELEM, 2> : k_beta_merge<ELEM, 1>;
        hipLaunchKernelGGL(k, grid, block, 0, c->sA, c->betas, c->pitch, c->n_total, c->mg_samples.as<const int32_t>(), n_samples, p.n_vec, c->mg_out.as<uint8_t>());
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[1], c->sA));
    const int64_t n_slabs = wg_merge_slabs(p.out_bytes);
    const auto fetch = [&](int64_t k) {
        return hipMemcpyAsync(c->bed.home[k & 1].p, c->mg_out.as<uint8_t>() + k * WG_MG_SLAB, (size_t)wg_merge_slab_len(p.out_bytes, k), hipMemcpyDeviceToHost, c->sA);
    };
    HIP_TRY(fetch(0));
    for (int64_t k = 0; k < n_slabs; k++) {
        HIP_TRY(hipStreamSynchronize(c->sA));
        if (k + 1 < n_slabs) HIP_TRY(fetch(k + 1));
        memcpy(static_cast<uint8_t*>(out) + k * WG_MG_SLAB, c->bed.home[k & 1].p, (size_t)wg_merge_slab_len(p.out_bytes, k));
    }
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->last_merge_rows_ms = ms;
    return WGBSSEG_OK;
}

double wgbsseg_last_merge_rows_ms(const wgbsseg_ctx* c) { return c ? c->last_merge_rows_ms : 0.0; }

static_assert(sizeof(wgbsseg_pair_range) == sizeof(wg_pair_range) && sizeof(wg_pair_range) == 40, "wgbsseg_pair_range is the kernels' wg_pair_range");

int wgbsseg_pair_ranges(wgbsseg_ctx* c, const int32_t* a, const int32_t* b, int64_t n_pairs, int32_t min_cov,
                        wgbsseg_pair_range* out, char* err, size_t errlen)
{
    if (const int rc = need_rows(c, err, errlen)) return rc;
    if (!out) { set_err(err, errlen, "pair_ranges: out is NULL"); return WGBSSEG_E_ARG; }
    const int rc = pair_list_up(c, "pair_ranges", a, b, n_pairs, min_cov, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    const wgbsseg_pair_range start = {0, 0, 0, 0, 0};
    std::vector<wg_pair_range> init((size_t)n_pairs, wg_pair_range{0, ~0ull, 0, ~0ull, 0});
    HIP_TRY(c->ph_out.ensure(init.size() * sizeof(wg_pair_range)));
    wg_pair_range* dout = c->ph_out.as<wg_pair_range>();
    HIP_TRY(hipMemcpyAsync(dout, init.data(), init.size() * sizeof(wg_pair_range), hipMemcpyHostToDevice, c->sA));
    const int32_t* dpa = c->ph_pairs.as<int32_t>();
    const dim3 grid((unsigned)((c->n_total + WG_PH_RUN - 1) / WG_PH_RUN * n_pairs));
    const AuxClock clock{c};
    HIP_TRY(clock.begin());
    by_elem(c->elem, [&](auto E) {
        hipLaunchKernelGGL(k_pair_ranges<decltype(E)::value>, grid, dim3(WG_PH_BLOCK), 0, c->sA, c->betas, c->pitch, c->n_total, dpa, dpa + n_pairs, (int32_t)n_pairs, min_cov, dout);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.end({{out, dout, sizeof(*out) * (size_t)n_pairs}}));
    for (int64_t i = 0; i < n_pairs; i++) if (out[i].n == 0) out[i] = start;      // (the bit patterns min and max began with are no doubles to hand out)
    return WGBSSEG_OK;
}

int wgbsseg_pair_hist(wgbsseg_ctx* c, const int32_t* a, const int32_t* b, int64_t n_pairs, int32_t min_cov, int32_t bins,
                      const double* edges, uint64_t* counts, char* err, size_t errlen)
{
    if (const int rc = need_rows(c, err, errlen)) return rc;
    if (!counts) { set_err(err, errlen, "pair_hist: counts is NULL"); return WGBSSEG_E_ARG; }
    std::string msg;
    if (!wg_pair_check_bins(bins, msg)) { set_err(err, errlen, "%s", msg.c_str()); return WGBSSEG_E_ARG; }
    if (n_pairs >= 1 && !wg_pair_check_edges(edges, n_pairs, bins, msg)) { set_err(err, errlen, "%s", msg.c_str()); return WGBSSEG_E_ARG; }
    const int rc = pair_list_up(c, "pair_hist", a, b, n_pairs, min_cov, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    const size_t ebytes = (size_t)n_pairs * 2 * (size_t)(bins + 1) * 8, cbytes = (size_t)n_pairs * (size_t)bins * (size_t)bins * 8;
    HIP_TRY(c->ph_edges.ensure(ebytes));
    HIP_TRY(c->ph_out.ensure(cbytes));
    HIP_TRY(hipMemcpyAsync(c->ph_edges.p, edges, ebytes, hipMemcpyHostToDevice, c->sA));
    unsigned long long* dcounts = c->ph_out.as<unsigned long long>();
    const int32_t* dpa = c->ph_pairs.as<int32_t>();
    const dim3 grid((unsigned)((c->n_total + WG_PH_RUN - 1) / WG_PH_RUN * n_pairs));
    const size_t lds = (size_t)wg_ph_lds_bytes(bins);
    const bool corners = env_flag("WGBSSEG_PAIR_CORNERS", false);     // (read per call: env.h; off: measured 5 % slower on the benchmark rows)
    const AuxClock clock{c};
    HIP_TRY(clock.begin());
    HIP_TRY(hipMemsetAsync(dcounts, 0, cbytes, c->sA));
    by_elem(c->elem, [&](auto E) {
        const auto k = corners ? k_pair_hist<decltype(E)::value, true> : k_pair_hist<decltype(E)::value, false>;
        hipLaunchKernelGGL(k, grid, dim3(WG_PH_BLOCK), lds, c->sA, c->betas, c->pitch, c->n_total, dpa, dpa + n_pairs, (int32_t)n_pairs, min_cov, bins,
                           c->ph_edges.as<const double>(), dcounts);
    });
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.end({{counts, dcounts, cbytes}}));
    return WGBSSEG_OK;
}

void wgbsseg_pair_hist_limits(int32_t* max_bins, int64_t* run_sites)
{
    if (max_bins) *max_bins = WG_PH_MAX_BINS;
    if (run_sites) *run_sites = WG_PH_RUN;
}

}  // extern "C"

namespace {

// everything of `n` bytes to fd, whatever write(2) takes at a time; -> 0 or errno
int write_all(int fd, const char* p, size_t n)
{
    while (n) {
        const ssize_t w = write(fd, p, n);
        if (w < 0) { if (errno == EINTR) continue; return errno; }
        p += w; n -= (size_t)w;
    }
    return 0;
}

// One beta2bed call in flight: its plan (bed_plan.h), what its launches share, what it has counted and written.  Two slabs are in flight,
// each in the buffers and between the events of its parity (BedScratch); wgbsseg_beta2bed runs the steps in the order of its loop.
struct BedRun {
    wgbsseg_ctx* c = nullptr;
    BedPlan plan;
    const uint16_t* mult = nullptr;      // the caller's multiplicities, from site plan.start0 on, or nullptr
    int fd = -1;                         // where the text goes
    char* err = nullptr; size_t errlen = 0;
    wg_bed_args base = {};               // the launch arguments every slab shares
    BedWgTable wg = {};                  // where the workgroup table keeps what (bed_plan.h)
    int64_t lines = 0, bytes = 0;        // lines counted | bytes written so far
    uint64_t home_bytes[2] = {0, 0};     // per parity: the text of the slab that last took it, in bytes
    bool bgzf = false;                   // the text stays on the device: its BGZF members come home and are written
    int64_t text_bytes = 0;              //   the text deflated so far, in bytes

    wg_bed_args slab_args(int64_t k) const { wg_bed_args s = base; s.first = plan.slab_first(k); s.n = (int32_t)plan.slab_count(k); return s; }
    uint64_t* wg_at(int64_t word) const { return c->bed.wg.as<uint64_t>() + word; }
    hipError_t add_ms(double& sum, const Event& e0, const Event& e1) const
    {
        float ms = 0;
        const hipError_t e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess) sum += ms;
        return e;
    }

    int tables_up(int32_t sample, const int64_t* chrom_cum, const char* const* chrom_names, int32_t n_chroms, const wgbsseg_bed_opts* o);   // events and buffers are there, the chromosome table is queued, `base` is filled
    hipError_t queue_lengths(int64_t k);   // queues slab k's multiplicities, its length pass and scan (len0 .. len1) and its totals' way home
    int wait_home(int64_t k);              // waits for the stream: slab k's totals and slab k-1's text are home; reads slab k-1's emit time
    int take_totals(int64_t k);            // reads slab k's length time and its totals: lines counted, bytes checked and kept for its parity
    int queue_emit(int64_t k);             // queues slab k's emit pass (emit0 .. emit1) and its text's way home; nothing for a slab without text
    int queue_deflate(int64_t k);          // bgzf: behind slab k's emit pass its text becomes members (def0 .. def1), packed densely (.. pack1); the packed size's way home
    int fetch_packed(int64_t k);           // bgzf: slab k's packed members, whose size is home, come home on a stream of their own; waits for them
    int write_home(int64_t k);             // writes slab k's text, which is home, to fd; -> 0 or errno
    int finish(int io, int64_t* lines_written, int64_t* bytes_written);   // the call's time and counts; after a failed write, waits for what is still queued
};

int BedRun::tables_up(int32_t sample, const int64_t* chrom_cum, const char* const* chrom_names, int32_t n_chroms, const wgbsseg_bed_opts* o)
{
    BedScratch& s = c->bed;
    for (auto& ev : s.ev) for (Event* e : {&ev.len0, &ev.len1, &ev.emit0, &ev.emit1}) if (!e->h) HIP_TRY(e->create());
    if (bgzf) for (auto& ev : s.ev) for (Event* e : {&ev.def0, &ev.def1, &ev.pack1}) if (!e->h) HIP_TRY(e->create());
    const std::vector<char> tab = wg_bed_pack_chroms(chrom_cum, chrom_names, n_chroms);
    const BedChromTable at = wg_bed_chrom_table(n_chroms);
    wg = wg_bed_wg_table(BedPlan::workgroups(plan.slab_count(0)));
    HIP_TRY(s.tab.ensure(tab.size()));
    HIP_TRY(s.wg.ensure(wg.size()));
    if (mult) HIP_TRY(s.mult.ensure((size_t)plan.slab_count(0) * 2));
    if (!s.tot.ensure(2 * 2 * 8)) { set_err(err, errlen, "beta2bed: out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    HIP_TRY(hipMemcpyAsync(s.tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice, c->sA));
    base.row = c->betas + (size_t)sample * (size_t)c->pitch;
    base.loci = c->loci;
    base.mult = mult ? s.mult.as<uint16_t>() : nullptr;
    base.cum = reinterpret_cast<const int64_t*>(s.tab.as<char>() + at.cum);
    base.names = s.tab.as<char>() + at.names;
    base.n_chroms = n_chroms; base.min_cov = o->min_cov; base.mean = o->mean ? 1 : 0; base.keep_na = o->keep_na ? 1 : 0;
    base.stage_bytes = (uint32_t)plan.stage_bytes;
    return WGBSSEG_OK;
}

hipError_t BedRun::queue_lengths(int64_t k)
{
    BedScratch& s = c->bed;
    const int par = wg_bed_parity(k);
    const wg_bed_args a = slab_args(k);
    const dim3 grid((unsigned)BedPlan::workgroups(a.n));
    hipError_t e = hipSuccess;
    if (mult) e = hipMemcpyAsync(s.mult.p, mult + (a.first - plan.start0), (size_t)a.n * 2, hipMemcpyHostToDevice, c->sA);
    if (e == hipSuccess) e = hipEventRecord(s.ev[par].len0, c->sA);
    if (e != hipSuccess) return e;
    by_elem(c->elem, [&](auto E) { hipLaunchKernelGGL(k_bed_len<decltype(E)::value>, grid, dim3(WG_BED_BLOCK), 0, c->sA, a, wg_at(wg.bytes), wg_at(wg.lines)); });
    hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, c->sA, wg_at(wg.bytes), wg_at(wg.lines), (int64_t)grid.x, wg_at(wg.base), wg_at(wg.tot_bytes));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(s.ev[par].len1, c->sA);
    if (e == hipSuccess) e = hipMemcpyAsync(static_cast<uint64_t*>(s.tot.p) + 2 * par, wg_at(wg.tot_bytes), 16, hipMemcpyDeviceToHost, c->sA);
    return e;
}

int BedRun::wait_home(int64_t k)
{
    HIP_TRY(hipStreamSynchronize(c->sA));
    if (k == 0) return WGBSSEG_OK;
    const int before = wg_bed_parity(k - 1);
    if (home_bytes[before]) HIP_TRY(add_ms(c->bed.emit_ms, c->bed.ev[before].emit0, c->bed.ev[before].emit1));
    if (home_bytes[before] && bgzf) {
        HIP_TRY(add_ms(c->bed.deflate_ms, c->bed.ev[before].def0, c->bed.ev[before].def1));
        HIP_TRY(add_ms(c->bed.pack_ms, c->bed.ev[before].def1, c->bed.ev[before].pack1));
    }
    return WGBSSEG_OK;
}

int BedRun::take_totals(int64_t k)
{
    const int par = wg_bed_parity(k);
    HIP_TRY(add_ms(c->bed.len_ms, c->bed.ev[par].len0, c->bed.ev[par].len1));
    volatile const uint64_t* tot = static_cast<volatile const uint64_t*>(c->bed.tot.p) + 2 * par;      // (bytes, lines)
    lines += (int64_t)tot[1];
    home_bytes[par] = tot[0];
    std::string msg;
    const int rc = wg_bed_check_slab_bytes(home_bytes[par], k, plan.slab_sites, msg);
    if (rc != WGBSSEG_OK) set_err(err, errlen, "%s", msg.c_str());
    return rc;
}

int BedRun::queue_emit(int64_t k)
{
    BedScratch& s = c->bed;
    const int par = wg_bed_parity(k);
    const uint64_t tot = home_bytes[par];
    if (!tot) return WGBSSEG_OK;
    const BedTextCap cap = wg_bed_text_capacity(tot, plan.slab_bytes_bound(0));
    HIP_TRY(s.out[par].ensure(cap.device));
    if (!bgzf && !s.home[par].ensure(cap.home)) { set_err(err, errlen, "beta2bed: out of page-locked host memory (%llu bytes)", (unsigned long long)tot); return WGBSSEG_E_NOMEM; }
    const wg_bed_args a = slab_args(k);
    const dim3 grid((unsigned)BedPlan::workgroups(a.n));
    HIP_TRY(hipEventRecord(s.ev[par].emit0, c->sA));
    by_elem(c->elem, [&](auto E) { hipLaunchKernelGGL(k_bed_emit<decltype(E)::value>, grid, dim3(WG_BED_BLOCK), 0, c->sA, a, wg_at(wg.base), s.out[par].as<char>()); });
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.ev[par].emit1, c->sA));
    if (bgzf) return queue_deflate(k);
    HIP_TRY(hipMemcpyAsync(s.home[par].p, s.out[par].p, (size_t)tot, hipMemcpyDeviceToHost, c->sA));
    return WGBSSEG_OK;
}

// The members of a slab are cut from the slab's own text (65280 bytes each, the last one shorter), so the compressed bytes depend on the
// slab size; the text they inflate to does not.
int BedRun::queue_deflate(int64_t k)
{
    BedScratch& s = c->bed;
    const int par = wg_bed_parity(k);
    const int64_t tot = (int64_t)home_bytes[par], members = wg_deflate_members(tot);
    HIP_TRY(s.slots.ensure((size_t)members * WG_DEF_PITCH));
    HIP_TRY(s.zmeta.ensure((size_t)(2 * members + 2) * 8));
    HIP_TRY(s.packed[par].ensure((size_t)wg_deflate_bound(tot)));
    if (!s.ztot.ensure(2 * 2 * 8)) { set_err(err, errlen, "beta2bed: out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    uint64_t* sizes = s.zmeta.as<uint64_t>(), *first = sizes + members, *totals = first + members;
    HIP_TRY(hipEventRecord(s.ev[par].def0, c->sA));
    hipLaunchKernelGGL(k_bgzf_deflate, dim3((unsigned)((members + WG_DEF_WAVES - 1) / WG_DEF_WAVES)), dim3(64 * WG_DEF_WAVES), 0, c->sA,
                       s.out[par].as<const uint8_t>(), tot, members, s.slots.as<uint8_t>(), sizes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.ev[par].def1, c->sA));
    hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, c->sA, sizes, sizes, members, first, totals);
    hipLaunchKernelGGL(k_bgzf_pack, dim3((unsigned)members), dim3(WG_PACK_BLOCK), 0, c->sA, s.slots.as<const uint8_t>(), sizes, first, s.packed[par].as<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.ev[par].pack1, c->sA));
    HIP_TRY(hipMemcpyAsync(static_cast<uint64_t*>(s.ztot.p) + 2 * par, totals, 16, hipMemcpyDeviceToHost, c->sA));
    return WGBSSEG_OK;
}

int BedRun::fetch_packed(int64_t k)
{
    BedScratch& s = c->bed;
    const int par = wg_bed_parity(k);
    if (!home_bytes[par]) return WGBSSEG_OK;
    const uint64_t packed = static_cast<volatile const uint64_t*>(s.ztot.p)[2 * par];
    if (packed > (uint64_t)wg_deflate_bound((int64_t)home_bytes[par])) { set_err(err, errlen, "beta2bed: slab %lld packed to %llu bytes, more than its bound", (long long)k, (unsigned long long)packed); return WGBSSEG_E_HIP; }
    if (!s.home[par].ensure((size_t)packed)) { set_err(err, errlen, "beta2bed: out of page-locked host memory (%llu bytes)", (unsigned long long)packed); return WGBSSEG_E_NOMEM; }
    HIP_TRY(hipMemcpyAsync(s.home[par].p, s.packed[par].p, (size_t)packed, hipMemcpyDeviceToHost, c->sB));
    HIP_TRY(hipStreamSynchronize(c->sB));
    text_bytes += (int64_t)home_bytes[par];
    home_bytes[par] = packed;                                    // what write_home writes
    return WGBSSEG_OK;
}

int BedRun::write_home(int64_t k)
{
    const int par = wg_bed_parity(k);
    if (!home_bytes[par]) return 0;
    const int io = write_all(fd, static_cast<const char*>(c->bed.home[par].p), (size_t)home_bytes[par]);
    if (!io) bytes += (int64_t)home_bytes[par];
    return io;
}

int BedRun::finish(int io, int64_t* lines_written, int64_t* bytes_written)
{
    c->last_block_sums_ms = c->bed.len_ms + c->bed.emit_ms;
    if (bgzf && !io) {
        io = write_all(fd, reinterpret_cast<const char*>(WG_BGZF_EOF), sizeof(WG_BGZF_EOF));
        if (!io) bytes += (int64_t)sizeof(WG_BGZF_EOF);
    }
    if (bytes_written) *bytes_written = bytes;
    if (io) {
        (void)hipStreamSynchronize(c->sA);                       // (what is still in flight lands in buffers the context keeps)
        set_err(err, errlen, "beta2bed: write failed (errno %d): %s", io, strerror(io));
        return WGBSSEG_E_IO;
    }
    if (lines_written) *lines_written = lines;
    return WGBSSEG_OK;
}

// state checks -> plan (bed_plan.h) -> the slab pipeline: while the device emits slab k and measures slab k+1, the host writes slab k-1.
// bgzf: slab k's text is deflated and packed on the device behind its emit pass; what comes home and is written are its BGZF members,
// and the end-of-file member follows the last slab.
int beta2bed_run(wgbsseg_ctx* c, int32_t sample, int64_t start0, int64_t end0, const uint16_t* mult,
                 const int64_t* chrom_cum, const char* const* chrom_names, int32_t n_chroms,
                 const wgbsseg_bed_opts* o, int fd, bool bgzf, int64_t* lines_written, int64_t* bytes_written, int64_t* text_bytes,
                 char* err, size_t errlen)
{
    if (c && lines_written) *lines_written = 0;
    if (c && bytes_written) *bytes_written = 0;
    if (c && text_bytes) *text_bytes = 0;
    if (const int rc = need_rows(c, err, errlen)) return rc;
    if (!c->loci || c->n_loci != c->n_total) { set_err(err, errlen, "loci not set or length differs from the betas (%lld vs %lld)", (long long)c->n_loci, (long long)c->n_total); return WGBSSEG_E_STATE; }
    BedRun run;
    run.c = c; run.mult = mult; run.fd = fd; run.err = err; run.errlen = errlen; run.bgzf = bgzf;
    std::string msg;
    int rc = wg_bed_plan(sample, c->n_samples, start0, end0, c->n_total, chrom_cum, chrom_names, n_chroms, o, run.plan, msg);
    if (rc == WGBSSEG_OK) rc = wg_bed_check_mult(mult, end0 - start0, start0, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    c->bed.len_ms = c->bed.emit_ms = c->bed.deflate_ms = c->bed.pack_ms = c->last_block_sums_ms = 0.0;
    const int64_t n = run.plan.n_slabs;
    if (n == 0) return bgzf ? run.finish(0, lines_written, bytes_written) : WGBSSEG_OK;
    HIP_TRY(hipSetDevice(c->device));
    rc = run.tables_up(sample, chrom_cum, chrom_names, n_chroms, o);
    if (rc != WGBSSEG_OK) return rc;
    HIP_TRY(run.queue_lengths(0));
    int io = 0;
    for (int64_t k = 0; k <= n && !io; k++) {
        rc = run.wait_home(k);                                   // slab k's totals and slab k-1's text (bgzf: its packed size) arrive
        if (rc == WGBSSEG_OK && k < n) rc = run.take_totals(k);
        if (rc == WGBSSEG_OK && k < n) rc = run.queue_emit(k);   // slab k is emitted (bgzf: and deflated and packed) ...
        if (rc != WGBSSEG_OK) return rc;
        if (k + 1 < n) HIP_TRY(run.queue_lengths(k + 1));        // ... and the lengths of slab k+1 queued
        if (k > 0 && bgzf) { rc = run.fetch_packed(k - 1); if (rc != WGBSSEG_OK) return rc; }      // slab k-1's members come home beside that
        if (k > 0) io = run.write_home(k - 1);                   // slab k-1 is written while the device works
    }
    if (text_bytes) *text_bytes = run.text_bytes;
    return run.finish(io, lines_written, bytes_written);
}

}  // namespace

extern "C" {

int wgbsseg_beta2bed(wgbsseg_ctx* c, int32_t sample, int64_t start0, int64_t end0, const uint16_t* mult,
                     const int64_t* chrom_cum, const char* const* chrom_names, int32_t n_chroms,
                     const wgbsseg_bed_opts* o, int fd, int64_t* lines_written, int64_t* bytes_written,
                     char* err, size_t errlen)
{
    return beta2bed_run(c, sample, start0, end0, mult, chrom_cum, chrom_names, n_chroms, o, fd, false, lines_written, bytes_written, nullptr, err, errlen);
}

int wgbsseg_beta2bed_bgzf(wgbsseg_ctx* c, int32_t sample, int64_t start0, int64_t end0, const uint16_t* mult,
                          const int64_t* chrom_cum, const char* const* chrom_names, int32_t n_chroms,
                          const wgbsseg_bed_opts* o, int fd, int64_t* lines_written, int64_t* bytes_written, int64_t* text_bytes,
                          char* err, size_t errlen)
{
    return beta2bed_run(c, sample, start0, end0, mult, chrom_cum, chrom_names, n_chroms, o, fd, true, lines_written, bytes_written, text_bytes, err, errlen);
}

double wgbsseg_bgzf_deflate_ms(const wgbsseg_ctx* c) { return c ? c->bed.deflate_ms + c->bed.pack_ms : -1.0; }

void wgbsseg_bgzf_deflate_pass_ms(const wgbsseg_ctx* c, double* deflate_ms, double* pack_ms)
{
    if (deflate_ms) *deflate_ms = c ? c->bed.deflate_ms : 0.0;
    if (pack_ms) *pack_ms = c ? c->bed.pack_ms : 0.0;
}

int64_t wgbsseg_bgzf_deflate_bound(int64_t n) { return n < 0 ? -1 : wg_deflate_bound(n); }

// host text -> BGZF bytes: every member by k_bgzf_deflate, packed by k_bgzf_pack (the counterpart of wgbsseg_bgzf_inflate)
int wgbsseg_bgzf_deflate(int device, const void* text, int64_t n, void* out, int64_t cap, int64_t* out_len, int eof, char* err, size_t errlen)
{
    if (!out_len) { set_err(err, errlen, "bad arguments to bgzf_deflate"); return WGBSSEG_E_ARG; }
    *out_len = 0;
    DeflatePlan p;
    std::string msg;
    int rc = plan_deflate(text, n, out, cap, WG_DEF_WAVES, p, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    rc = check_device(device, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    uint64_t totals[2] = {0, 0};
    if (p.members) {
        HIP_TRY(hipSetDevice(device));
        DevBuf dtext, slots, meta, dense;
        HIP_TRY(dtext.ensure((size_t)n)); HIP_TRY(slots.ensure((size_t)p.slot_bytes)); HIP_TRY(meta.ensure((size_t)(2 * p.members + 2) * 8)); HIP_TRY(dense.ensure((size_t)p.bound));
        uint64_t* sizes = meta.as<uint64_t>(), *first = sizes + p.members, *dtot = first + p.members;
        HIP_TRY(hipMemcpy(dtext.p, text, (size_t)n, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_bgzf_deflate, dim3((unsigned)p.grid), dim3(64 * WG_DEF_WAVES), 0, 0, dtext.as<const uint8_t>(), n, p.members, slots.as<uint8_t>(), sizes);
        hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, 0, sizes, sizes, p.members, first, dtot);
        hipLaunchKernelGGL(k_bgzf_pack, dim3((unsigned)p.members), dim3(WG_PACK_BLOCK), 0, 0, slots.as<const uint8_t>(), sizes, first, dense.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(totals, dtot, 16, hipMemcpyDeviceToHost));
        if ((int64_t)totals[0] > p.bound - (int64_t)sizeof(WG_BGZF_EOF)) { set_err(err, errlen, "bgzf_deflate: %llu bytes came out, more than the bound", (unsigned long long)totals[0]); return WGBSSEG_E_HIP; }
        HIP_TRY(hipMemcpy(out, dense.p, (size_t)totals[0], hipMemcpyDeviceToHost));
    }
    if (eof) memcpy(static_cast<char*>(out) + totals[0], WG_BGZF_EOF, sizeof(WG_BGZF_EOF));
    *out_len = (int64_t)totals[0] + (eof ? (int64_t)sizeof(WG_BGZF_EOF) : 0);
    return WGBSSEG_OK;
}

void wgbsseg_beta2bed_pass_ms(const wgbsseg_ctx* c, double* length_ms, double* emit_ms)
{
    if (length_ms) *length_ms = c ? c->bed.len_ms : 0.0;
    if (emit_ms) *emit_ms = c ? c->bed.emit_ms : 0.0;
}

void wgbsseg_beta2bed_limits(int64_t* default_slab, int64_t* max_slab, int32_t* max_stage_bytes, int32_t* max_name)
{
    if (default_slab) *default_slab = WG_BED_DEFAULT_SLAB;
    if (max_slab) *max_slab = WG_BED_MAX_SLAB;
    if (max_stage_bytes) *max_stage_bytes = WG_BED_STAGE_BYTES;
    if (max_name) *max_name = WG_BED_MAX_NAME;
}

int wgbsseg_convert_regions(wgbsseg_ctx* c, const int64_t* chrom_lo, const int64_t* chrom_hi, const int64_t* chrom_bp, const int64_t* start,
                            const int64_t* end, const uint8_t* slow, int64_t n, int64_t* start_cpg, int64_t* end_cpg, char* err, size_t errlen)
{
    if (!c) { set_err(err, errlen, "ctx is NULL"); return WGBSSEG_E_ARG; }
    if (!c->loci) { set_err(err, errlen, "loci not set"); return WGBSSEG_E_STATE; }
    if (n < 0 || (n && (!chrom_lo || !chrom_hi || !chrom_bp || !start || !end || !slow || !start_cpg || !end_cpg))) { set_err(err, errlen, "bad arguments to convert_regions"); return WGBSSEG_E_ARG; }
    if (n == 0) return WGBSSEG_OK;
    for (int64_t i = 0; i < n; i++)
        if (chrom_lo[i] < 0 || chrom_hi[i] < chrom_lo[i] || chrom_hi[i] > c->n_loci) {
            set_err(err, errlen, "region %lld: chromosome slice [%lld, %lld) is outside the %lld resident loci", (long long)i, (long long)chrom_lo[i], (long long)chrom_hi[i], (long long)c->n_loci);
            return WGBSSEG_E_ARG;
        }
    HIP_TRY(hipSetDevice(c->device));
    const size_t nb = (size_t)n * 8;
    HIP_TRY(c->cv_in.ensure(5 * nb + (size_t)n));
    HIP_TRY(c->cv_out.ensure(2 * nb));
    char* d = c->cv_in.as<char>();
    const int64_t* srcs[5] = {chrom_lo, chrom_hi, chrom_bp, start, end};
    for (int k = 0; k < 5; k++) HIP_TRY(hipMemcpyAsync(d + k * nb, srcs[k], nb, hipMemcpyHostToDevice, c->sA));
    HIP_TRY(hipMemcpyAsync(d + 5 * nb, slow, (size_t)n, hipMemcpyHostToDevice, c->sA));
    int64_t* o = c->cv_out.as<int64_t>();
    const int64_t gx = (n + WG_BLOCK - 1) / WG_BLOCK;
    if (gx > 0x7fffffff) { set_err(err, errlen, "too many regions for one convert call"); return WGBSSEG_E_ARG; }
    const AuxClock clock{c};
    HIP_TRY(clock.begin());
    hipLaunchKernelGGL(k_convert, dim3((unsigned)gx), dim3(WG_BLOCK), 0, c->sA, c->loci, reinterpret_cast<const int64_t*>(d),
                       reinterpret_cast<const int64_t*>(d + nb), reinterpret_cast<const int64_t*>(d + 2 * nb), reinterpret_cast<const int64_t*>(d + 3 * nb),
                       reinterpret_cast<const int64_t*>(d + 4 * nb), reinterpret_cast<const uint8_t*>(d + 5 * nb), n, o, o + n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.end({{start_cpg, o, nb}, {end_cpg, o + n, nb}}));
    return WGBSSEG_OK;
}

}  // extern "C"

namespace {

// the gather pass of `rows` rows from row `first` of the call's sites on: queued on stream A (array_kernels.h)
void launch_site_gather(wgbsseg_ctx* c, int64_t first, int64_t rows, int32_t n_cols, uint32_t* cells)
{
    wg_gather_args g;
    g.betas = c->betas; g.pitch = c->pitch;
    g.site0 = c->site.site0.as<int64_t>() + first;
    g.samples = c->site.samples.as<int32_t>();
    g.n_cells = rows * (int64_t)n_cols; g.n_cols = n_cols;
    const dim3 grid((unsigned)SitePlan::workgroups(g.n_cells));
    by_elem(c->elem, [&](auto E) { hipLaunchKernelGGL(k_site_gather<decltype(E)::value>, grid, dim3(WG_SITE_BLOCK), 0, c->sA, g, cells); });
}

// what both probe-table calls begin with: the checks of array_plan.h, then the sites and the samples on the device
int site_lists_up(wgbsseg_ctx* c, const char* who, const int64_t* site0, int64_t n_rows, const int32_t* samples, int32_t n_cols, char* err, size_t errlen)
{
    std::string msg;
    const int rc = wg_site_check_gather(who, site0, n_rows, samples, n_cols, c->n_samples, c->n_total, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    if (n_rows == 0) return WGBSSEG_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->site.site0.ensure((size_t)n_rows * 8));
    HIP_TRY(c->site.samples.ensure((size_t)n_cols * 4));
    HIP_TRY(hipMemcpyAsync(c->site.site0.p, site0, (size_t)n_rows * 8, hipMemcpyHostToDevice, c->sA));
    HIP_TRY(hipMemcpyAsync(c->site.samples.p, samples, (size_t)n_cols * 4, hipMemcpyHostToDevice, c->sA));
    return WGBSSEG_OK;
}

// One site_table call in flight: its plan (array_plan.h), what its launches share, what it has counted and written.  Two slabs are in
// flight as in BedRun, in BedScratch's buffers and between its events and SiteScratch's; wgbsseg_site_table runs the steps in the order of its loop.
struct SiteRun {
    wgbsseg_ctx* c = nullptr;
    SitePlan plan;
    int fd = -1;                         // where the text goes
    char* err = nullptr; size_t errlen = 0;
    wg_site_args base = {};              // the launch arguments every slab shares
    BedWgTable wg = {};                  // where the workgroup table keeps what (bed_plan.h)
    int64_t lines = 0, bytes = 0;        // lines counted | bytes written so far
    uint64_t home_bytes[2] = {0, 0};     // per parity: the text of the slab that last took it, in bytes

    wg_site_args slab_args(int64_t k) const { wg_site_args s = base; s.first_row = plan.slab_first(k); s.n_fields = (int32_t)plan.fields(plan.slab_count(k)); return s; }
    uint64_t* wg_at(int64_t word) const { return c->bed.wg.as<uint64_t>() + word; }
    hipError_t add_ms(double& sum, const Event& e0, const Event& e1) const
    {
        float ms = 0;
        const hipError_t e = hipEventElapsedTime(&ms, e0, e1);
        if (e == hipSuccess) sum += ms;
        return e;
    }

    int tables_up(const char* labels, const int64_t* label_off);   // events and buffers are there, the labels are queued, `base` is filled
    hipError_t queue_lengths(int64_t k);   // queues slab k's gather pass (g0 .. g1), its length pass and scan (len0 .. len1) and its totals' way home
    int wait_home(int64_t k);              // waits for the stream: slab k's totals and slab k-1's text are home; reads slab k-1's emit time
    int take_totals(int64_t k);            // reads slab k's gather and length times and its totals: lines counted, bytes kept for its parity
    int queue_emit(int64_t k);             // queues slab k's emit pass (emit0 .. emit1) and its text's way home
    int write_home(int64_t k);             // writes slab k's text, which is home, to fd; -> 0 or errno
    int finish(int io, int64_t* lines_written, int64_t* bytes_written);   // the call's time and counts; after a failed write, waits for what is still queued
};

int SiteRun::tables_up(const char* labels, const int64_t* label_off)
{
    BedScratch& s = c->bed;
    SiteScratch& t = c->site;
    for (auto& ev : s.ev) for (Event* e : {&ev.len0, &ev.len1, &ev.emit0, &ev.emit1}) if (!e->h) HIP_TRY(e->create());
    for (auto& ev : t.ev) for (Event* e : {&ev.g0, &ev.g1}) if (!e->h) HIP_TRY(e->create());
    wg = wg_bed_wg_table(SitePlan::workgroups(plan.fields(plan.slab_count(0))));
    const size_t label_bytes = (size_t)(label_off[plan.n_rows] - label_off[0]);
    HIP_TRY(s.wg.ensure(wg.size()));
    HIP_TRY(t.cells.ensure((size_t)plan.cells(plan.slab_count(0)) * 4));
    HIP_TRY(t.labels.ensure(label_bytes ? label_bytes : 1));
    HIP_TRY(t.label_off.ensure((size_t)(plan.n_rows + 1) * 8));
    if (!s.tot.ensure(2 * 2 * 8)) { set_err(err, errlen, "site_table: out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    if (label_bytes) HIP_TRY(hipMemcpyAsync(t.labels.p, labels + label_off[0], label_bytes, hipMemcpyHostToDevice, c->sA));
    HIP_TRY(hipMemcpyAsync(t.label_off.p, label_off, (size_t)(plan.n_rows + 1) * 8, hipMemcpyHostToDevice, c->sA));
    base.cells = t.cells.as<uint32_t>();
    base.labels = t.labels.as<char>();
    base.label_off = t.label_off.as<int64_t>();
    base.label_base = label_off[0];
    base.n_cols = plan.n_cols; base.min_cov = (uint32_t)plan.min_cov;
    return WGBSSEG_OK;
}

hipError_t SiteRun::queue_lengths(int64_t k)
{
    BedScratch& s = c->bed;
    const int par = wg_bed_parity(k);
    const wg_site_args a = slab_args(k);
    const dim3 grid((unsigned)SitePlan::workgroups(a.n_fields));
    hipError_t e = hipEventRecord(c->site.ev[par].g0, c->sA);
    if (e != hipSuccess) return e;
    launch_site_gather(c, a.first_row, plan.slab_count(k), plan.n_cols, c->site.cells.as<uint32_t>());
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(c->site.ev[par].g1, c->sA);
    if (e == hipSuccess) e = hipEventRecord(s.ev[par].len0, c->sA);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_site_len, grid, dim3(WG_SITE_BLOCK), 0, c->sA, a, wg_at(wg.bytes), wg_at(wg.lines));
    hipLaunchKernelGGL(k_bed_scan, dim3(1), dim3(WG_BED_BLOCK), 0, c->sA, wg_at(wg.bytes), wg_at(wg.lines), (int64_t)grid.x, wg_at(wg.base), wg_at(wg.tot_bytes));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(s.ev[par].len1, c->sA);
    if (e == hipSuccess) e = hipMemcpyAsync(static_cast<uint64_t*>(s.tot.p) + 2 * par, wg_at(wg.tot_bytes), 16, hipMemcpyDeviceToHost, c->sA);
    return e;
}

int SiteRun::wait_home(int64_t k)
{
    HIP_TRY(hipStreamSynchronize(c->sA));
    if (k == 0) return WGBSSEG_OK;
    const int before = wg_bed_parity(k - 1);
    if (home_bytes[before]) HIP_TRY(add_ms(c->site.emit_ms, c->bed.ev[before].emit0, c->bed.ev[before].emit1));
    return WGBSSEG_OK;
}

int SiteRun::take_totals(int64_t k)
{
    const int par = wg_bed_parity(k);
    HIP_TRY(add_ms(c->site.gather_ms, c->site.ev[par].g0, c->site.ev[par].g1));
    HIP_TRY(add_ms(c->site.len_ms, c->bed.ev[par].len0, c->bed.ev[par].len1));
    volatile const uint64_t* tot = static_cast<volatile const uint64_t*>(c->bed.tot.p) + 2 * par;      // (bytes, lines)
    lines += (int64_t)tot[1];
    home_bytes[par] = tot[0];
    return WGBSSEG_OK;
}

int SiteRun::queue_emit(int64_t k)
{
    BedScratch& s = c->bed;
    const int par = wg_bed_parity(k);
    const uint64_t tot = home_bytes[par];
    if (!tot) return WGBSSEG_OK;
    const BedTextCap cap = wg_bed_text_capacity(tot, plan.slab_bytes_bound(0));
    HIP_TRY(s.out[par].ensure(cap.device));
    if (!s.home[par].ensure(cap.home)) { set_err(err, errlen, "site_table: out of page-locked host memory (%llu bytes)", (unsigned long long)tot); return WGBSSEG_E_NOMEM; }
    const wg_site_args a = slab_args(k);
    const dim3 grid((unsigned)SitePlan::workgroups(a.n_fields));
    HIP_TRY(hipEventRecord(s.ev[par].emit0, c->sA));
    hipLaunchKernelGGL(k_site_emit, grid, dim3(WG_SITE_BLOCK), 0, c->sA, a, wg_at(wg.base), s.out[par].as<char>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s.ev[par].emit1, c->sA));
    HIP_TRY(hipMemcpyAsync(s.home[par].p, s.out[par].p, (size_t)tot, hipMemcpyDeviceToHost, c->sA));
    return WGBSSEG_OK;
}

int SiteRun::write_home(int64_t k)
{
    const int par = wg_bed_parity(k);
    if (!home_bytes[par]) return 0;
    const int io = write_all(fd, static_cast<const char*>(c->bed.home[par].p), (size_t)home_bytes[par]);
    if (!io) bytes += (int64_t)home_bytes[par];
    return io;
}

int SiteRun::finish(int io, int64_t* lines_written, int64_t* bytes_written)
{
    c->last_block_sums_ms = c->site.gather_ms + c->site.len_ms + c->site.emit_ms;
    if (bytes_written) *bytes_written = bytes;
    if (io) {
        (void)hipStreamSynchronize(c->sA);                       // (what is still in flight lands in buffers the context keeps)
        set_err(err, errlen, "site_table: write failed (errno %d): %s", io, strerror(io));
        return WGBSSEG_E_IO;
    }
    if (lines_written) *lines_written = lines;
    return WGBSSEG_OK;
}

}  // namespace

extern "C" {

// checks (array_plan.h) -> the lists up -> one gather launch over every row -> fetch
int wgbsseg_site_counts(wgbsseg_ctx* c, const int64_t* site0, int64_t n_rows, const int32_t* samples, int32_t n_cols, uint16_t* out, char* err, size_t errlen)
{
    if (const int rc = need_rows(c, err, errlen)) return rc;
    if (n_rows > 0 && !out) { set_err(err, errlen, "site_counts: out is NULL"); return WGBSSEG_E_ARG; }
    const int rc = site_lists_up(c, "site_counts", site0, n_rows, samples, n_cols, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    c->last_block_sums_ms = 0.0;
    if (n_rows == 0) return WGBSSEG_OK;
    const size_t obytes = (size_t)n_rows * (size_t)n_cols * 4;
    if (SitePlan::workgroups((int64_t)(obytes / 4)) > 0x7fffffff) { set_err(err, errlen, "site_counts: %lld rows x %d columns are too many cells for one call", (long long)n_rows, (int)n_cols); return WGBSSEG_E_ARG; }
    HIP_TRY(c->site.cells.ensure(obytes));
    const AuxClock clock{c};
    HIP_TRY(clock.begin());
    launch_site_gather(c, 0, n_rows, n_cols, c->site.cells.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(clock.end({{out, c->site.cells.p, obytes}}));      // (a cell is its {meth, cov} as two uint16)
    return WGBSSEG_OK;
}

// state checks -> plan (array_plan.h) -> the slab pipeline: while the device emits slab k and gathers and measures slab k+1, the host writes slab k-1
int wgbsseg_site_table(wgbsseg_ctx* c, const int64_t* site0, int64_t n_rows, const int32_t* samples, int32_t n_cols, const char* labels,
                       const int64_t* label_off, const wgbsseg_site_table_opts* o, int fd, int64_t* lines_written, int64_t* bytes_written,
                       char* err, size_t errlen)
{
    if (c && lines_written) *lines_written = 0;
    if (c && bytes_written) *bytes_written = 0;
    if (const int rc = need_rows(c, err, errlen)) return rc;
    SiteRun run;
    run.c = c; run.fd = fd; run.err = err; run.errlen = errlen;
    std::string msg;
    int rc = wg_site_check_gather("site_table", site0, n_rows, samples, n_cols, c->n_samples, c->n_total, msg);
    if (rc == WGBSSEG_OK) rc = wg_site_plan(n_rows, n_cols, labels, label_off, o, run.plan, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    c->site.gather_ms = c->site.len_ms = c->site.emit_ms = c->last_block_sums_ms = 0.0;
    const int64_t n = run.plan.n_slabs;
    if (n == 0) return WGBSSEG_OK;
    rc = site_lists_up(c, "site_table", site0, n_rows, samples, n_cols, err, errlen);
    if (rc == WGBSSEG_OK) rc = run.tables_up(labels, label_off);
    if (rc != WGBSSEG_OK) return rc;
    HIP_TRY(run.queue_lengths(0));
    int io = 0;
    for (int64_t k = 0; k <= n && !io; k++) {
        rc = run.wait_home(k);                                   // slab k's totals and slab k-1's text arrive
        if (rc == WGBSSEG_OK && k < n) rc = run.take_totals(k);
        if (rc == WGBSSEG_OK && k < n) rc = run.queue_emit(k);   // slab k is emitted ...
        if (rc != WGBSSEG_OK) return rc;
        if (k + 1 < n) HIP_TRY(run.queue_lengths(k + 1));        // ... and slab k+1 gathered and measured behind it: one cell table serves both
        if (k > 0) io = run.write_home(k - 1);                   // slab k-1 is written while the device works
    }
    return run.finish(io, lines_written, bytes_written);
}

void wgbsseg_site_table_pass_ms(const wgbsseg_ctx* c, double* gather_ms, double* length_ms, double* emit_ms)
{
    if (gather_ms) *gather_ms = c ? c->site.gather_ms : 0.0;
    if (length_ms) *length_ms = c ? c->site.len_ms : 0.0;
    if (emit_ms) *emit_ms = c ? c->site.emit_ms : 0.0;
}

void wgbsseg_site_table_limits(int64_t* default_slab_rows, int64_t* max_slab_rows, int32_t* max_label, int32_t* max_cols)
{
    if (default_slab_rows) *default_slab_rows = WG_SITE_DEFAULT_SLAB_ROWS;
    if (max_slab_rows) *max_slab_rows = WG_SITE_MAX_SLAB_ROWS;
    if (max_label) *max_label = WG_SITE_MAX_LABEL;
    if (max_cols) *max_cols = WG_SITE_MAX_COLS;
}

}  // extern "C"
