// wgbsseg.hip — host side of libwgbsseg.so: the C ABI of include/wgbsseg.h over the gfx950 kernels of
// seg_kernels.h and the other *_kernels.h.  One context = one GPU (own streams, grow-only scratch in HBM).  No CPU compute path exists
// here: without a HIP device every entry point fails.
//
// Build (see wgbs_tools_amd/build.py):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -shared wgbsseg.hip -o libwgbsseg.so
// -ffp-contract=off is REQUIRED: the likelihood term must round exactly like the reference's x86-64 build
// (no fused multiply-add anywhere; SURVEY.md 7 hard part 2).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <initializer_list>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>
#include <pthread.h>
#include <sched.h>
#include <sys/mman.h>
#include <unistd.h>
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
#include <emmintrin.h>
#endif

#include "../../include/wgbsseg.h"
#include "owners.h"
#include "seg_kernels.h"
#include "block_plan.h"
#include "share_plan.h"
#include "block_kernels.h"
#include "pat_kernels.h"
#include "homog_kernels.h"
#include "frag_kernels.h"
#include "view_kernels.h"
#include "sam_kernels.h"
#include "fasta_kernels.h"
#include "bimodal_kernels.h"
#include "inflate_plan.h"
#include "inflate_kernels.h"
#include "deflate_plan.h"
#include "deflate_kernels.h"
#include "stats_kernels.h"
#include "merge_kernels.h"
#include "pair_kernels.h"
#include "bed_kernels.h"
#include "array_kernels.h"
#include "bed2beta_plan.h"
#include "bed2beta_kernels.h"
#include "plain_dp.h"
#include "stitch.h"
#include "add_loci.h"
#include "table_io.h"

namespace {

void set_err(char* err, size_t errlen, const char* fmt, ...)
{
    if (!err || !errlen) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, errlen, fmt, ap);
    va_end(ap);
}

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e__ = (expr);                                                                   \
        if (e__ != hipSuccess) {                                                                   \
            set_err(err, errlen, "HIP error %d (%s) at %s:%d: %s", (int)e__, hipGetErrorString(e__), \
                    __FILE__, __LINE__, #expr);                                                    \
            return WGBSSEG_E_HIP;                                                                  \
        }                                                                                          \
    } while (0)

hipError_t set_kernel_attributes();      // defined below, next to the kernel launchers
inline int ceil_pow2(int v) { int r = 1; while (r < v) r <<= 1; return r; }
inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

}  // namespace

#define WG_MAX_CPUS 8192
struct NearCpus { std::vector<unsigned long> bits; bool valid = false; };      // affinity mask of the CPUs next to a device

// The events of a batch: stream A: it begins, its tables are up, windows done, statistics copied, tile plan done; the scan stream: k_validate, k_scan
// (jobs with wide tiles only), the pass is done (its verdict may be copied); stream B: traceback + border lists, results on the host.
enum BatchEvent { EV_BEGIN, EV_WINDOWS, EV_SCAN_END, EV_PLAN, EV_TRACE0, EV_TRACE1, EV_HOME, EV_STATS, EV_VALIDATE0, EV_VALIDATE1, EV_SCAN0, EV_SCAN1, EV_UPLOADED, EV_COUNT };

// What wgbsseg_beta2bed keeps between calls (row_engines.h, BedRun): the chromosome table (bed_plan.h: wg_bed_pack_chroms) | a slab's
// multiplicities | its workgroup table (bed_plan.h: BedWgTable) | the text of two slabs, on the device and at home | the totals of two slabs
// at home | per slab parity the events around the length pass and scan and around the emit pass | the two passes' times of the last call.
// Members go in reverse order of declaration: events, then page-locked memory, then device memory, as when they were the context's own.
// The context's destructor has synchronised the device by then, so nothing here needs a teardown rule of its own.
// wgbsseg_beta2bed_bgzf adds: the member slots of one slab | its sizes, first bytes and total (deflate_plan.h) | the packed members of two
// slabs | their totals at home | per slab parity the events around the deflate launch and behind the pack launch | the two launches' times.
struct BedScratch {
    DevBuf tab, mult, wg, out[2];
    DevBuf slots, zmeta, packed[2];
    PinnedBuf home[2], tot, ztot;
    struct PassEvents { Event len0, len1, emit0, emit1, def0, def1, pack1; } ev[2];
    double len_ms = 0.0, emit_ms = 0.0, deflate_ms = 0.0, pack_ms = 0.0;
};

// What wgbsseg_site_counts and wgbsseg_site_table keep between calls (row_engines.h, SiteRun) beyond BedScratch's workgroup table, text buffers,
// totals and pass events, which the probe table shares with beta2bed: the rows' sites | the columns' samples | the label bytes | their
// offsets | the compact cell table of one slab (site_counts: of the whole call) | per slab parity the events around the gather pass |
// the three passes' times of the last call.
struct SiteScratch {
    DevBuf site0, samples, labels, label_off, cells;
    struct GatherEvents { Event g0, g1; } ev[2];
    double gather_ms = 0.0, len_ms = 0.0, emit_ms = 0.0;
};

struct wgbsseg_ctx {
    int device = 0;
    NearCpus near_cpus;          // the upload threads run there (worked out once, at create)
    Stream sA, sB, sC;     // scoring (+ everything else) | recurrence, traceback | the scan pass
    Stream sA2;                                // second scoring stream: medium / wide tiles beside the narrow ones (stage loop)
    // inputs
    DevBuf betas_own, loci_own;
    const uint8_t* betas = nullptr;
    int64_t pitch = 0, n_total = 0;
    int32_t elem = 1;        // bytes per count of the resident rows: 1 = .beta / .bin (uint8 pairs), 2 = .lbeta (uint16 pairs; block sums only)
    int64_t site_base = 0;   // absolute 0-based index of resident site 0 (messages only; all call coordinates are resident-relative)
    int32_t n_samples = 0;
    const uint32_t* loci = nullptr;
    int64_t n_loci = 0;
    // scratch
    DevBuf chunks, wtile, carry, W16, cum32, back16, chunk_pairs, status, tile_tot, tile_base, tile_chunk;
    DevBuf plan_cbase, plan_cum0, plan_tbase, plan_pairs, plan_tiles, plan_cnt, umax16;
    std::vector<PinnedBuf> pinned;
    std::vector<PinnedBuf> up_stage;   // the page-locked staging pieces of the uploads, `depth` per upload thread (run_upload); kept until destroy
    DevBuf tiles[3], cost[3], stage_ctr, dpstate, tmp_borders, nb, boff, out_borders[2], edges, lookup;
    DevBuf dbg_a, dbg_b, dbg_c;   // the wgbsseg_debug_* calls and wgbsseg_prefix_sums only
    int out_par = 0;              // which of the two result buffers the batch in flight writes: the lists of the previous batch may still be on their way home (below)
    // early delivery (segment_regions' first batch): k_copy_out (on the scan stream) writes the chunks' border lists into the page-locked result ...
    Event evS;     // the scan stream's last command of the batch in flight (the copy of its verdict)
    Event evD;     // ... while the host already rehearses the junctions on the lists' edges and runs the follow-up batch; evD: the lists are home
    bool out_pending = false;
    bool batch_open = false;      // a batch is between its first launch and its clean end (an error return leaves it set: the next batch drains the device first)
    std::vector<wg_d2> h_lookup;   // host copy of the k-scaled log tables of the call in flight (source of an async upload)
    float lookup_pc = -1.0f;       // what the device copy `lookup` was built for: pseudo count and exponent rows of the narrow / wide / medium class
    int lookup_rows[3] = {-1, -1, -1};
    Event ev[EV_COUNT];   // a batch's events (BatchEvent); the context's other calls time themselves between ev[0] and ev[1]
    PinnedBuf h_status;      // page-locked landing area of the status words: D2H copies that really are asynchronous
    PinnedBuf h_job, h_pieces, h_sb;   // ... the staging areas of a job's tables on their way up (chunk table, window tiles, cleared status | k_validate's pieces)
    PinnedBuf h_out;         // ... and of a batch's CSR offsets (a small batch: of its border lists too)
    std::vector<Event> ev_cost0, ev_cost1, ev_dp0, ev_dp1, ev_fork, ev_join;     // per stage
    // last-call info
    wgbsseg_timings tim = {};
    int64_t last_sites = 0, last_pairs = 0;
    int32_t last_stages = 0;
    bool last_valid = false;
    // the last batch's chunk table, for wgbsseg_debug_fetch: where each chunk lies in the job-site arrays (every chunk from a multiple of 8 entries on) and,
    // for a one-stage job, in the cost buffer (first row and blocks: read back from the stage plan at the first fetch of "cost")
    struct LastChunk { int64_t site_off; int32_t len; int64_t cost_row0, cost_rows; };
    std::vector<LastChunk> last_chunks;
    bool last_cost_rows_known = false;
    // the last batch's plan, for wgbsseg_debug_last_plan: the form plan_stages chose and Batch::stages launched, copied when the batch ends (like last_chunks)
    struct LastPlan {
        int32_t n_stages = 0, gated = 0, nbuf = 0, last_pct = 0, dp_mode = 0, all_narrow = 0, live_ctx = 0, n_chunks = 0;
        std::vector<int32_t> sb;             // [n_stages + 1] stage bounds
        std::vector<int32_t> dp16;           // [n_stages] 1: the stage's recurrence was k_dp16
        std::vector<int64_t> stage_tiles;    // [3 * n_stages] tiles per stage and class
    } last_plan;
    long long cost_budget_bytes = 0;
    int force_stages = 0;
    bool counted_live = false;
    // staging and tiling as the environment asks (env.h: WGBSSEG_STAGE_GATE_WIDE_EVALS, _STAGE_MIN_EVALS, _STAGE_GATE_SHARED, _STAGE_GATE, _LAST_STAGE_PCT, _DP_MODE, _NS, _TI).
    // stage_gate > 0: the stages of a staged job alternate between the two scoring streams behind k_stage_gate; last_stage_pct -1: chosen per job
    double stage_gate_wide_evals = 100000.0, stage_min_evals_per_step = 21000.0;
    bool stage_gate_shared = false;
    int stage_gate = 768, last_stage_pct = -1, force_dp_mode = 0, force_ns = 0, force_ti = 0;
    double last_block_sums_ms = 0.0;
    int64_t table_blocks = 0;  // > 0: bs_out holds the [n_samples][table_blocks] ratio table of a mode-3 block reduction (what wgbsseg_marker_stats reads)
    bool accumulate = false;   // add to `tim` instead of resetting it (region-level calls span several batches)
    // site ranges whose `meth <= cov` check has run in the API call in flight (sorted, disjoint): the follow-up batches of a
    // region-level call hold junction patches only, all inside chunks its first batch has validated.  Never kept across
    // API calls: device-resident betas handed over by pointer may change between them.
    std::vector<std::pair<int64_t, int64_t>> validated;
    DevBuf scan_pieces, divcheck, plan_sb;
    DevBuf bs_plan, bs_desc, bs_out;   // wgbsseg_block_sums: the plan's tables (block_plan.h) | the streaming kernel's block descriptors | the result
    DevBuf mk_out, cv_in, cv_out;      // wgbsseg_marker_stats: the statistics and the two sample lists; wgbsseg_convert_regions: the regions' columns | their CpG ranges
    DevBuf st_ranges, st_parts;     // wgbsseg_sample_stats: the range table | the tiles' partial results and the per-sample results
    DevBuf mg_samples, mg_out;      // wgbsseg_merge_rows: the rows named | the summed row
    double last_merge_rows_ms = 0.0;
    DevBuf ph_pairs, ph_edges, ph_out;   // wgbsseg_pair_ranges / _pair_hist: the pair list (a | b) | the edges | the ranges or the counts
    BedScratch bed;                      // wgbsseg_beta2bed
    SiteScratch site;                    // wgbsseg_site_counts, wgbsseg_site_table
    std::vector<int32_t> h_stage_bounds;
    // the short division core of the narrow scoring tiles: verified on the device per pseudo count (k_check_div)
    float divs_pc = -1.0f;     // pseudo count the verdict below is for
    bool divs_ok = false;
    int64_t last_dp_chunks = 0, last_dp_stride = 0;
    float divs_m_pc = -1.0f;   // the same for the operand pairs of a medium tile (ntotal <= 255 * WG_MEDIUM_WMAX)
    bool divs_m_ok = false;
    // the switches of the environment as create_ctx read them (env.h has the table): WGBSSEG_DIV_SHORT, _BLOCK_SUMS_GENERAL, _SCAN_PIECE_SITES,
    // _MEDIUM_WMAX (0: no medium class), _DP_WLEAN, not _NO_EARLY, not _NO_SPECULATION, _PROFILE >= 2
    bool divs_enabled = true, bs_general = false;
    int64_t scan_piece_sites = 4096;
    int medium_wmax = WG_MEDIUM_WMAX;
    bool dp_wlean = true, early = true, speculate = true, batch_marks = false;
    // Everything above frees itself, in reverse order of declaration — the streams last; by then nothing runs on the device any more.
    ~wgbsseg_ctx() { (void)hipSetDevice(device); (void)hipDeviceSynchronize(); }
};

namespace {

// The CPUs next to a device: /sys/bus/pci/devices/<bus id>/local_cpulist (e.g. "0-63,128-191"), cut to the CPUs this process may run on, as an
// affinity mask of up to WG_MAX_CPUS CPUs (a fixed cpu_set_t stops at 1024 and sched_getaffinity then FAILS on a larger host: ADVICE r05).  Worked out
// once per context (create).  An upload thread that runs on the OTHER socket of a two-socket host fills page-locked pieces over there and the DMA then crosses the
// socket link: measured on an MI355X box (round 5, x200 = 11.3 GB): the same upload at 9 .. 35 GB/s from run to run with free-running
// threads.  false: unknown (no sysfs, every CPU listed, WGBSSEG_UPLOAD_PIN=0) — the threads then run where the scheduler puts them.
bool device_local_cpus(int device, NearCpus* out)
{
    out->valid = false;
    if (!env_flag("WGBSSEG_UPLOAD_PIN", true)) return false;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, device) != hipSuccess) { (void)hipGetLastError(); return false; }
    for (char* q = bus; *q; q++) if (*q >= 'A' && *q <= 'F') *q = (char)(*q - 'A' + 'a');       // sysfs names are lower case
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", bus);
    FILE* f = fopen(path, "r");
    if (!f) return false;
    char line[8192] = {0};
    const bool got = fgets(line, (int)sizeof line, f) != nullptr;
    fclose(f);
    if (!got) return false;
    const size_t bytes = CPU_ALLOC_SIZE(WG_MAX_CPUS);
    std::vector<unsigned long> allowed(bytes / sizeof(unsigned long), 0ul);
    out->bits.assign(bytes / sizeof(unsigned long), 0ul);
    cpu_set_t* A = reinterpret_cast<cpu_set_t*>(allowed.data());
    cpu_set_t* L = reinterpret_cast<cpu_set_t*>(out->bits.data());
    if (sched_getaffinity(0, bytes, A) != 0) return false;
    int n_local = 0;
    for (const char* q = line; *q;) {
        while (*q == ',' || *q == ' ' || *q == '\n') q++;
        if (*q < '0' || *q > '9') break;
        char* end = nullptr;
        long a = strtol(q, &end, 10), b = a;
        if (*end == '-') b = strtol(end + 1, &end, 10);
        for (long x = a; x <= b && x < WG_MAX_CPUS; x++) if (CPU_ISSET_S((int)x, bytes, A)) { CPU_SET_S((int)x, bytes, L); n_local++; }
        q = end;
    }
    if (n_local == 0 || n_local == CPU_COUNT_S(bytes, A)) return false;      // nothing to choose from
    out->valid = true;
    return true;
}
inline void pin_to(const NearCpus& n)
{
    if (n.valid) (void)pthread_setaffinity_np(pthread_self(), n.bits.size() * sizeof(unsigned long), reinterpret_cast<const cpu_set_t*>(n.bits.data()));
}
// Page-cached file bytes -> a page-locked staging piece (round 6, profiles/r06_upload_ab.txt):
//   * the piece's pages are mapped in ONE call (madvise MADV_POPULATE_READ, Linux >= 5.14) instead of a minor fault per 4 KB page as the copy touches them;
//   * non-temporal stores: the staging piece is written once and read by the DMA engine — no read-for-ownership, no cache pollution.
// WGBSSEG_UPLOAD_POPULATE=0 / WGBSSEG_UPLOAD_NT=0 switch either off (A/B).  x200 (11.3 GB) end to end on one box: 0.38-0.45 s -> 0.32 s with both and
// 8 x 2 MB pieces; x32 0.107-0.114 -> 0.098-0.110.  The rate of ONE setting still swings between 30 and 47 GB/s from run to run on the same box.
struct FillMode { bool populate = true, nt = true; };
inline void fill_piece(void* dst, const uint8_t* src, size_t n, const FillMode& m)
{
#ifdef MADV_POPULATE_READ
    if (m.populate) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(src) & ~(uintptr_t)4095, b = (reinterpret_cast<uintptr_t>(src) + n + 4095) & ~(uintptr_t)4095;
        (void)madvise(reinterpret_cast<void*>(a), b - a, MADV_POPULATE_READ);      // (an error — an old kernel, not a mapping — just leaves the faults to the copy)
    }
#endif
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)
    if (m.nt && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        __m128i* d = reinterpret_cast<__m128i*>(dst);
        const __m128i* s = reinterpret_cast<const __m128i*>(src);
        size_t v = n >> 6;
        for (; v > 0; v--, s += 4, d += 4) {
            const __m128i x0 = _mm_loadu_si128(s), x1 = _mm_loadu_si128(s + 1), x2 = _mm_loadu_si128(s + 2), x3 = _mm_loadu_si128(s + 3);
            _mm_stream_si128(d, x0); _mm_stream_si128(d + 1, x1); _mm_stream_si128(d + 2, x2); _mm_stream_si128(d + 3, x3);
        }
        _mm_sfence();
        const size_t done = n & ~(size_t)63;
        if (n > done) memcpy(static_cast<char*>(dst) + done, src + done, n - done);
        return;
    }
#endif
    memcpy(dst, src, n);
}
// What one upload call does: the five WGBSSEG_UPLOAD_* switches are read here and nowhere else, per call.  The two forms:
//   blocking (set_betas_host, set_lbetas_host, set_loci_host, group_load_host): 4 MB pieces, 4 threads (small inputs fewer: below two, the plain copy of
//     upload_rows), two pieces per thread, filled by memcpy, rows one after the other.  One thread drives ~33 GB/s (page faults + the copy into page-locked
//     staging); a few threads, each with its own stream, fill the link (measured 46 GB/s with 4; more threads only contend).
//   streaming (group_load_host_async): 4 threads x 1 MB, from 4 GB up 8 x 2 MB, WGBSSEG_UPLOAD_DEPTH pieces per thread, filled by fill_piece, piece-major:
//     piece p of EVERY row before piece p + 1 of any, which is what makes a prefix of the sites ready for the segmenter while the rest is on its way.
//     (Measured, free-running threads: 4 threads x 1 MB 33.5 GB/s, x 2 MB 26-29, 8-16 threads 17-30: profiles/r02_upload_sweep.txt.  Round 5, threads on the
//     device's CPUs: 8 threads x 4 MB 37-42 GB/s on 11.3 GB (x200: 0.35-0.38 s end to end against 0.43-0.50 with 4 x 1 MB); x32's 1.8 GB the same either
//     way: profiles/r05_upload_pinned_ab.txt.  Round 6: 8 x 2 MB with the pieces' pages mapped per call and a non-temporal fill: x200 0.32 s end to end on
//     both runs of the A/B against 0.33-0.45 for 8 x 4 MB, profiles/r06_upload_ab.txt.)
struct UploadPlan {
    int64_t piece = 0, ppr = 0, n_tasks = 0;     // bytes of a staging piece; pieces per row; pieces in all
    int T = 1, depth = 2;                        // upload threads; staging pieces (copies in flight) per thread
    bool piece_major = false;                    // task it = p * n_rows + r, not r * ppr + p
    FillMode fill = {false, false};
};
UploadPlan plan_upload(bool streaming, int64_t n_rows, int64_t row_bytes)
{
    UploadPlan u;
    const int64_t bytes = row_bytes * n_rows;
    const bool big = streaming && bytes >= (4LL << 30);
    const long long kb = env_int("WGBSSEG_UPLOAD_PIECE_KB", 0), threads = env_int("WGBSSEG_UPLOAD_THREADS", 0);
    u.piece = kb >= 64 ? (int64_t)kb << 10 : streaming ? (big ? 2 << 20 : 1 << 20) : 4 << 20;
    u.ppr = (row_bytes + u.piece - 1) / u.piece;
    u.n_tasks = u.ppr * n_rows;
    const int64_t T = std::min<int64_t>(threads > 0 ? threads : big ? 8 : 4, 64);
    u.T = (int)std::max<int64_t>(1, std::min<int64_t>(T, streaming ? u.n_tasks : std::min<int64_t>(u.n_tasks / 2, bytes >> 24)));
    u.piece_major = streaming;
    if (streaming) {
        const long long depth = env_int("WGBSSEG_UPLOAD_DEPTH", 2);
        if (depth >= 2 && depth <= 8) u.depth = (int)depth;
        u.fill.populate = env_flag("WGBSSEG_UPLOAD_POPULATE", true);
        u.fill.nt = env_flag("WGBSSEG_UPLOAD_NT", true);
    }
    return u;
}

// The upload loop: pageable host rows (typically memory-mapped .beta files) -> HBM, dst + r * dst_pitch <- rows[r][0 .. row_bytes), in pieces that
// u.T threads claim one after the other.  A thread runs on the device's CPUs with a stream of its own and u.depth staging pieces of the context
// (c->up_stage; allocated — and so first touched — by the thread itself, after pin_to: they sit on that socket), and calls landed(it) when piece `it`
// is on the device.  Returns every thread's verdict.
template <class Landed>
std::vector<hipError_t> run_upload(wgbsseg_ctx* c, const UploadPlan& u, uint8_t* dst, int64_t dst_pitch, const uint8_t* const* rows, int64_t n_rows,
                                   int64_t row_bytes, Landed landed)
{
    const int depth = u.depth;
    if (c->up_stage.size() < (size_t)(depth * u.T)) c->up_stage.resize((size_t)(depth * u.T));
    std::atomic<int64_t> next(0);
    std::vector<hipError_t> terr((size_t)u.T, hipSuccess);
    auto worker = [&](int t) {
        pin_to(c->near_cpus);
        hipError_t e = hipSetDevice(c->device);
        PinnedBuf* const stg = &c->up_stage[(size_t)(depth * t)];
        for (int k = 0; k < depth && e == hipSuccess; k++) if (!stg[k].ensure_exact((size_t)u.piece)) e = hipErrorOutOfMemory;
        Stream st;
        Event ev[8];
        int64_t task_of[8] = {-1, -1, -1, -1, -1, -1, -1, -1};      // the piece whose copy was queued last from slot k (-1: none in flight)
        if (e == hipSuccess) e = st.create();
        for (int k = 0; k < depth && e == hipSuccess; k++) e = ev[k].create(false);
        auto settle = [&](int k) {                                  // slot k's previous copy has left the piece
            if (task_of[k] < 0) return;
            e = hipEventSynchronize(ev[k]);
            if (e == hipSuccess) landed(task_of[k]);
            task_of[k] = -1;
        };
        int k = 0;
        while (e == hipSuccess) {
            const int64_t it = next.fetch_add(1);
            if (it >= u.n_tasks) break;
            const int64_t p = u.piece_major ? it / n_rows : it % u.ppr, r = u.piece_major ? it % n_rows : it / u.ppr;
            const int64_t o = p * u.piece, b = std::min<int64_t>(u.piece, row_bytes - o);
            settle(k);
            if (e != hipSuccess) break;
            fill_piece(stg[k].p, rows[r] + o, (size_t)b, u.fill);
            e = hipMemcpyAsync(dst + r * dst_pitch + o, stg[k].p, (size_t)b, hipMemcpyHostToDevice, st);
            if (e == hipSuccess) e = hipEventRecord(ev[k], st);
            task_of[k] = it;
            k = (k + 1) % depth;
        }
        for (int q = 0; q < depth && e == hipSuccess; q++, k = (k + 1) % depth) settle(k);
        if (st) { const hipError_t e2 = hipStreamSynchronize(st); if (e == hipSuccess) e = e2; }      // (after an error too: no copy may outlive the call, the pieces stay)
        terr[(size_t)t] = e;
    };
    std::vector<std::thread> th;
    for (int t = 0; t < u.T; t++) th.emplace_back(worker, t);
    for (auto& x : th) x.join();
    return terr;
}

int upload_rows(wgbsseg_ctx* c, uint8_t* dst, int64_t dst_pitch, const uint8_t* const* rows, int64_t n_rows, int64_t row_bytes,
                const char* what, char* err, size_t errlen)
{
    const double t0 = wall_s();
    const UploadPlan u = plan_upload(false, n_rows, row_bytes);
    if (u.T <= 1) {      // small inputs: the plain copy
        for (int64_t r = 0; r < n_rows; r++)
            HIP_TRY(hipMemcpyAsync(dst + r * dst_pitch, rows[r], (size_t)row_bytes, hipMemcpyHostToDevice, c->sA));
        HIP_TRY(hipStreamSynchronize(c->sA));
    } else {
        const std::vector<hipError_t> terr = run_upload(c, u, dst, dst_pitch, rows, n_rows, row_bytes, [](int64_t) {});
        for (int t = 0; t < u.T; t++) HIP_TRY(terr[(size_t)t]);
    }
    if (profiling()) fprintf(stderr, "[wgbsseg] %s to the device: %.1f ms, %.1f GB/s (%d upload threads)\n", what, (wall_s() - t0) * 1e3,
                             (double)row_bytes * n_rows / (wall_s() - t0) * 1e-9, u.T);
    return WGBSSEG_OK;
}

// ready_sites: the sites that are resident for EVERY row, counted from the front (what the streaming segmenter waits on)
int upload_rows_streaming(wgbsseg_ctx* c, uint8_t* dst, int64_t dst_pitch, const uint8_t* const* rows, int64_t n_rows, int64_t row_bytes,
                          std::atomic<int64_t>& ready_sites, std::string& msg)
{
    const double t0 = wall_s();
    const UploadPlan u = plan_upload(true, n_rows, row_bytes);
    std::vector<std::atomic<int>> rows_done((size_t)u.ppr);
    for (auto& x : rows_done) x.store(0);
    std::atomic<int64_t> pieces_done(0);
    std::mutex mu;
    auto complete = [&](int64_t task) {                          // task = p * n_rows + r: row r's piece p is on the device
        const int64_t p = task / n_rows;
        if (rows_done[(size_t)p].fetch_add(1) + 1 == (int)n_rows) {
            std::lock_guard<std::mutex> lk(mu);
            int64_t d = pieces_done.load();
            while (d < u.ppr && rows_done[(size_t)d].load() == (int)n_rows) d++;
            pieces_done.store(d);
            ready_sites.store(std::min<int64_t>(d * u.piece, row_bytes) / 2);
        }
    };
    const std::vector<hipError_t> terr = run_upload(c, u, dst, dst_pitch, rows, n_rows, row_bytes, complete);
    for (int t = 0; t < u.T; t++)
        if (terr[(size_t)t] != hipSuccess) { msg = std::string("HIP error during the upload: ") + hipGetErrorString(terr[(size_t)t]); return WGBSSEG_E_HIP; }
    ready_sites.store(row_bytes / 2);
    if (profiling()) fprintf(stderr, "[wgbsseg] betas to the device (streaming): %.1f ms, %.1f GB/s (%d upload threads x %d pieces of %lld KB%s%s%s)\n", (wall_s() - t0) * 1e3,
                             (double)row_bytes * n_rows / (wall_s() - t0) * 1e-9, u.T, u.depth, (long long)(u.piece >> 10), c->near_cpus.valid ? ", on the device's CPUs" : "",
                             u.fill.populate ? ", pages mapped per piece" : "", u.fill.nt ? ", non-temporal fill" : "");
    return WGBSSEG_OK;
}

}  // namespace

extern "C" {

int wgbsseg_version(void) { return WGBSSEG_VERSION; }

int wgbsseg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"
namespace {
std::atomic<int> g_live_ctx[64];      // contexts alive per device (gated stages want theirs alone on its device)

// what every context and engine asks of its device: it exists and is a gfx950 (it is made the current device)
int check_device(int device, char* err, size_t errlen)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_err(err, errlen, "no HIP device available (%s); libwgbsseg has no CPU fallback", hipGetErrorString(e));
        return WGBSSEG_E_HIP;
    }
    if (device < 0 || device >= n) { set_err(err, errlen, "device %d out of range (0..%d)", device, n - 1); return WGBSSEG_E_ARG; }
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (!strstr(prop.gcnArchName, "gfx950")) {
        set_err(err, errlen, "device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
        return WGBSSEG_E_HIP;
    }
    return WGBSSEG_OK;
}

// scan_low_priority: the scan stream below the scoring streams (right where k_validate competes with the kernels of its OWN batch only; the shares of a group that
// double up on a device get it at the scoring streams' priority: wgbsseg_group_create)
int create_ctx(int device, bool scan_low_priority, wgbsseg_ctx** out, char* err, size_t errlen)
{
    if (!out) { set_err(err, errlen, "out is NULL"); return WGBSSEG_E_ARG; }
    *out = nullptr;
    const int rc = check_device(device, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    HIP_TRY(set_kernel_attributes());        // per device, checked: k_dp / k_cost ask for more than 64 KB of dynamic LDS
    std::unique_ptr<wgbsseg_ctx> c(new (std::nothrow) wgbsseg_ctx());      // (a failing call below frees what has been made)
    if (!c) { set_err(err, errlen, "out of host memory"); return WGBSSEG_E_NOMEM; }
    c->device = device;
    (void)device_local_cpus(device, &c->near_cpus);
    HIP_TRY(c->sA.create());
    {   // the recurrence stream outranks the scoring stream: its 483 latency-bound workgroups should never queue behind
        // the hundreds of thousands of throughput-bound scoring tiles
        int lo_p = 0, hi_p = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
        HIP_TRY(c->sB.create(hi_p));
        // ... and the scan stream ranks below it: k_validate starts with the batch, beside the windows pass, and must not take the wavefront
        // slots of the kernels that are on the way to the first scoring tile (measured, hg19 x 32: scoring begins 0.36 ms into the batch
        // instead of 0.46, profiles/r06_front_ab.txt)
        HIP_TRY(scan_low_priority ? c->sC.create(lo_p) : c->sC.create());
    }
    HIP_TRY(c->sA2.create());
    HIP_TRY(c->evD.create(false));
    HIP_TRY(c->evS.create(false));
    for (auto& v : c->ev) HIP_TRY(v.create());
    const long long budget_mb = env_int("WGBSSEG_COST_BUDGET_MB", 0);
    c->cost_budget_bytes = (budget_mb > 0 ? budget_mb : 6144LL) << 20;
    c->force_stages = (int)env_int("WGBSSEG_FORCE_STAGES", 0);
    c->stage_gate = (int)env_int("WGBSSEG_STAGE_GATE", c->stage_gate, 0);
    c->stage_gate_shared = env_flag("WGBSSEG_STAGE_GATE_SHARED", false);
    c->stage_gate_wide_evals = env_double("WGBSSEG_STAGE_GATE_WIDE_EVALS", c->stage_gate_wide_evals);
    c->stage_min_evals_per_step = env_double("WGBSSEG_STAGE_MIN_EVALS", c->stage_min_evals_per_step);
    if (env_int("WGBSSEG_LAST_STAGE_PCT", -1) != -1) c->last_stage_pct = (int)env_int("WGBSSEG_LAST_STAGE_PCT", -1, 5, 800);      // (unset: chosen per job)
    c->force_dp_mode = (int)env_int("WGBSSEG_DP_MODE", 0, 0, 2);
    c->force_ns = (int)env_int("WGBSSEG_NS", 0);
    c->force_ti = (int)env_int("WGBSSEG_TI", 0);
    c->bs_general = env_flag("WGBSSEG_BLOCK_SUMS_GENERAL", false);
    c->divs_enabled = env_flag("WGBSSEG_DIV_SHORT", true);
    { const long long sp = env_int("WGBSSEG_SCAN_PIECE_SITES", 0); if (sp >= 1024) c->scan_piece_sites = sp & ~1023LL; }
    const int wm = (int)env_int("WGBSSEG_MEDIUM_WMAX", WG_MEDIUM_WMAX, 0, WG_MEDIUM_WMAX);
    c->medium_wmax = wm > WG_NARROW_WMAX ? wm : 0;
    c->dp_wlean = env_flag("WGBSSEG_DP_WLEAN", true);
    c->early = !env_flag("WGBSSEG_NO_EARLY", false);
    c->speculate = !env_flag("WGBSSEG_NO_SPECULATION", false);
    c->batch_marks = env_int("WGBSSEG_PROFILE", 0) >= 2;
    g_live_ctx[device & 63].fetch_add(1, std::memory_order_relaxed);
    c->counted_live = true;
    *out = c.release();
    return WGBSSEG_OK;
}
}  // namespace
extern "C" {

int wgbsseg_create(int device, wgbsseg_ctx** out, char* err, size_t errlen) { return create_ctx(device, true, out, err, errlen); }

void wgbsseg_destroy(wgbsseg_ctx* c)
{
    if (!c) return;
    if (c->counted_live) g_live_ctx[c->device & 63].fetch_sub(1, std::memory_order_relaxed);
    const double t0 = wall_s();
    delete c;
    if (profiling()) fprintf(stderr, "[wgbsseg] destroy: %.1f ms\n", (wall_s() - t0) * 1e3);
}

// The context's own device rows for n_samples x n_sites count pairs of `elem` bytes: they exist, the context points at them (the device is current),
// and what the last call left behind is no longer valid.  The bytes are still to come.
static hipError_t own_rows(wgbsseg_ctx* c, int64_t n_samples, int64_t n_sites, int elem)
{
    const int64_t pitch = round_up(2 * elem * n_sites, 256) + 256;      // slack: vector loads may run past the last site
    const hipError_t e = c->betas_own.ensure((size_t)pitch * (size_t)n_samples);
    if (e != hipSuccess) return e;
    c->betas = c->betas_own.as<uint8_t>();
    c->pitch = pitch; c->n_total = n_sites; c->n_samples = (int32_t)n_samples; c->elem = elem;
    c->last_valid = false;
    return hipSuccess;
}

static int set_rows_host(wgbsseg_ctx* c, const uint8_t* const* samples, int64_t n_samples, int64_t n_sites, int elem, char* err, size_t errlen)
{
    if (!c || !samples || n_samples < 1 || n_sites < 1) { set_err(err, errlen, "bad arguments to set_betas_host"); return WGBSSEG_E_ARG; }
    for (int64_t s = 0; s < n_samples; s++)
        if (!samples[s]) { set_err(err, errlen, "samples[%lld] is NULL", (long long)s); return WGBSSEG_E_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(own_rows(c, n_samples, n_sites, elem));
    return upload_rows(c, c->betas_own.as<uint8_t>(), c->pitch, samples, n_samples, 2 * elem * n_sites, "betas", err, errlen);
}

int wgbsseg_set_betas_host(wgbsseg_ctx* c, const uint8_t* const* samples, int64_t n_samples, int64_t n_sites,
                           char* err, size_t errlen)
{
    return set_rows_host(c, samples, n_samples, n_sites, 1, err, errlen);
}

int wgbsseg_set_lbetas_host(wgbsseg_ctx* c, const uint16_t* const* samples, int64_t n_samples, int64_t n_sites,
                            char* err, size_t errlen)
{
    return set_rows_host(c, reinterpret_cast<const uint8_t* const*>(samples), n_samples, n_sites, 2, err, errlen);
}

int wgbsseg_set_betas_device(wgbsseg_ctx* c, const void* base, int64_t n_samples, int64_t pitch_bytes, int64_t n_sites,
                             char* err, size_t errlen)
{
    if (!c || !base || n_samples < 1 || n_sites < 1 || pitch_bytes < 2 * n_sites) { set_err(err, errlen, "bad arguments to set_betas_device"); return WGBSSEG_E_ARG; }
    if (((uintptr_t)base & 15) || (pitch_bytes & 15)) { set_err(err, errlen, "device betas base and pitch must be multiples of 16 bytes"); return WGBSSEG_E_ARG; }
    c->betas = reinterpret_cast<const uint8_t*>(base);
    c->pitch = pitch_bytes; c->n_total = n_sites; c->n_samples = (int32_t)n_samples; c->elem = 1;
    c->last_valid = false;
    return WGBSSEG_OK;
}

int wgbsseg_set_loci_host(wgbsseg_ctx* c, const uint32_t* loci, int64_t n_sites, char* err, size_t errlen)
{
    if (!c || !loci || n_sites < 1) { set_err(err, errlen, "bad arguments to set_loci_host"); return WGBSSEG_E_ARG; }
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->loci_own.ensure((size_t)n_sites * 4));
    const uint8_t* row = reinterpret_cast<const uint8_t*>(loci);
    const int rc = upload_rows(c, c->loci_own.as<uint8_t>(), 0, &row, 1, n_sites * 4, "loci", err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    c->loci = c->loci_own.as<uint32_t>();
    c->n_loci = n_sites;
    c->last_valid = false;
    return WGBSSEG_OK;
}

int wgbsseg_set_loci_device(wgbsseg_ctx* c, const void* loci, int64_t n_sites, char* err, size_t errlen)
{
    if (!c || !loci || n_sites < 1) { set_err(err, errlen, "bad arguments to set_loci_device"); return WGBSSEG_E_ARG; }
    // every kernel reads the loci as uint32; k_window's 16-byte loads start at the 16-byte boundary at or below a locus, which it works
    // out from the address itself, and never leave [loci, loci + n_sites): whole entries is all the alignment they need
    if ((uintptr_t)loci & 3) { set_err(err, errlen, "device loci must be a multiple of 4 bytes"); return WGBSSEG_E_ARG; }
    c->loci = reinterpret_cast<const uint32_t*>(loci);
    c->n_loci = n_sites;
    c->last_valid = false;
    return WGBSSEG_OK;
}

}  // extern "C"

namespace {

// Host copy of the chunk table + job-wide offsets; uploads it and builds the JobView.
struct Job {
    std::vector<ChunkDesc> h;
    std::vector<ScanPiece> pieces;      // what k_validate reads: the batch's sites not yet validated in this API call, cut into wave tasks
    int64_t val_sites = 0;
    std::vector<int64_t> wtile_off;     // exclusive prefix of 256-site tiles per chunk (+ total), then (as int32 pairs) the chunk of every 256th tile
    int64_t sites = 0, carry_entries = 0, units = 0, n_hint = 0;
    int64_t sites_padded = 0;           // the job-site arrays (W16, cum32, back16) hold every chunk from a multiple of 8 entries on: 16-byte vectors of them are aligned
    int32_t max_len = 0;
    JobStatus st0;          // source of an async H2D copy: must outlive the call's stream work
    JobView v = {};
};

int build_job(wgbsseg_ctx* c, const int64_t* start0, const int32_t* len, int64_t n_chunks, Job& job, bool need_loci,
              char* err, size_t errlen)
{
    if (!c) { set_err(err, errlen, "ctx is NULL"); return WGBSSEG_E_ARG; }
    if (!c->betas) { set_err(err, errlen, "betas not set"); return WGBSSEG_E_STATE; }
    if (c->elem != 1) { set_err(err, errlen, "the resident rows are uint16 (.lbeta): segment, scan and prefix sums read uint8 .beta data only (as the reference's segmentor, segmentor.cpp:166-176)"); return WGBSSEG_E_STATE; }
    if (need_loci && (!c->loci || c->n_loci != c->n_total)) { set_err(err, errlen, "loci not set or length differs from the betas (%lld vs %lld)", (long long)c->n_loci, (long long)c->n_total); return WGBSSEG_E_STATE; }
    if (!start0 || !len || n_chunks < 1 || n_chunks > 0x7fffffff) { set_err(err, errlen, "bad chunk list"); return WGBSSEG_E_ARG; }
    job.h.resize((size_t)n_chunks);
    job.wtile_off.resize((size_t)n_chunks + 1);
    int64_t so = 0, co = 0, wt = 0, uo = 0, total = 0;
    for (int64_t i = 0; i < n_chunks; i++) {
        if (len[i] < 1 || len[i] > (1 << 30) || start0[i] < 0 || start0[i] + len[i] > c->n_total) {
            set_err(err, errlen, "chunk %lld = [%lld, +%d) is empty or outside the %lld sites of the beta files",
                    (long long)i, (long long)start0[i], (int)len[i], (long long)c->n_total);
            return WGBSSEG_E_ARG;
        }
        ChunkDesc& d = job.h[(size_t)i];
        d.start0 = start0[i]; d.len = len[i]; d.site_off = so; d.carry_off = co; d.unit_off = uo; d.nG = (int32_t)(((start0[i] + len[i] - 1) >> WG_CARRY_SHIFT) - (start0[i] >> WG_CARRY_SHIFT) + 1);
        job.wtile_off[(size_t)i] = wt;
        wt += (len[i] + WG_WIN_TILE - 1) / WG_WIN_TILE;
        so += round_up((int64_t)len[i], 8);
        total += len[i];
        uo += (len[i] + 15) / 16;
        co += (int64_t)d.nG * c->n_samples;
        job.max_len = std::max(job.max_len, len[i]);
    }
    job.wtile_off[(size_t)n_chunks] = wt;
    {   // hint table for k_window: chunk of tile 256*h, for h = 0 .. tiles/256 + 1 (int32, packed behind the prefix)
        const int64_t nh = (wt >> 8) + 2;
        job.n_hint = nh;
        job.wtile_off.resize((size_t)n_chunks + 1 + (size_t)((nh + 1) / 2));
        int32_t* hint = reinterpret_cast<int32_t*>(job.wtile_off.data() + n_chunks + 1);
        int64_t cix = 0;
        for (int64_t h = 0; h < nh; h++) {
            const int64_t tile = h << 8;
            while (cix + 1 < n_chunks && job.wtile_off[(size_t)cix + 1] <= tile) cix++;
            hint[h] = (int32_t)cix;
        }
    }
    job.sites = total; job.sites_padded = so; job.carry_entries = co; job.units = uo;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->chunks.ensure(sizeof(ChunkDesc) * (size_t)n_chunks));
    HIP_TRY(c->carry.ensure(sizeof(uint2) * (size_t)co));
    HIP_TRY(c->status.ensure(sizeof(JobStatus)));
    HIP_TRY(c->wtile.ensure(8 * job.wtile_off.size()));
    memset(&job.st0, 0, sizeof(job.st0));
    job.st0.first_bad = ~0ULL;
    // the job's tables go up through ONE page-locked staging area (round 6): a copy out of pageable memory is staged by the runtime and
    // blocks the caller for ~15 us — four of them in front of every batch, the follow-up batches of junction patches included
    const size_t b_chunks = sizeof(ChunkDesc) * (size_t)n_chunks, b_wtile = 8 * job.wtile_off.size();
    const size_t o_wtile = (size_t)round_up((int64_t)b_chunks, 64), o_status = o_wtile + (size_t)round_up((int64_t)b_wtile, 64), o_end = o_status + 64;
    if (c->h_job.ensure(o_end)) {
        char* h = reinterpret_cast<char*>(c->h_job.p);
        memcpy(h, job.h.data(), b_chunks);
        memcpy(h + o_wtile, job.wtile_off.data(), b_wtile);
        memcpy(h + o_status, &job.st0, sizeof(job.st0));
        HIP_TRY(hipMemcpyAsync(c->chunks.p, h, b_chunks, hipMemcpyHostToDevice, c->sA));
        HIP_TRY(hipMemcpyAsync(c->wtile.p, h + o_wtile, b_wtile, hipMemcpyHostToDevice, c->sA));
        HIP_TRY(hipMemcpyAsync(c->status.p, h + o_status, sizeof(job.st0), hipMemcpyHostToDevice, c->sA));
    } else {
        HIP_TRY(hipMemcpyAsync(c->chunks.p, job.h.data(), b_chunks, hipMemcpyHostToDevice, c->sA));
        HIP_TRY(hipMemcpyAsync(c->wtile.p, job.wtile_off.data(), b_wtile, hipMemcpyHostToDevice, c->sA));
        HIP_TRY(hipMemcpyAsync(c->status.p, &job.st0, sizeof(job.st0), hipMemcpyHostToDevice, c->sA));
    }
    JobView& v = job.v;
    v.betas = c->betas; v.pitch = c->pitch; v.n_total = c->n_total; v.loci = c->loci;
    v.chunks = c->chunks.as<ChunkDesc>(); v.carry = c->carry.as<uint2>();
    v.n_samples = c->n_samples; v.n_chunks = (int32_t)n_chunks;
    return WGBSSEG_OK;
}

bool interval_covered(const std::vector<std::pair<int64_t, int64_t>>& v, int64_t lo, int64_t hi)
{
    // v sorted by first site: the last interval that begins at or before lo (false negatives only when intervals overlap)
    auto it = std::upper_bound(v.begin(), v.end(), lo, [](int64_t x, const std::pair<int64_t, int64_t>& iv) { return x < iv.first; });
    return it != v.begin() && (--it)->second >= hi;
}

// The sites of a batch that still need the `meth <= cov` pass in this API call, as wave tasks of k_validate.  Chunks of a
// genome arrive in order and tile their regions: they fuse into one run per region; junction patches (same batch or a
// follow-up batch) fall inside runs and drop out.  Arbitrary chunk lists work too (overlaps are validated twice).
int plan_validation(wgbsseg_ctx* c, Job& job, bool fresh_call, char* err, size_t errlen)
{
    if (fresh_call) c->validated.clear();
    std::vector<std::pair<int64_t, int64_t>> runs;
    bool sorted = true;
    for (const ChunkDesc& d : job.h) {
        const int64_t lo = d.start0, hi = d.start0 + d.len;
        if (!runs.empty() && lo == runs.back().second) { runs.back().second = hi; continue; }
        if (interval_covered(c->validated, lo, hi) || (sorted && interval_covered(runs, lo, hi))) continue;
        if (!runs.empty() && lo < runs.back().first) sorted = false;
        runs.emplace_back(lo, hi);
    }
    const int64_t P = c->scan_piece_sites;
    job.pieces.clear(); job.val_sites = 0;
    for (const auto& r : runs) {
        job.val_sites += r.second - r.first;
        for (int64_t a = r.first; a < r.second; ) {
            const int64_t b = std::min(r.second, (a / P + 1) * P);          // cut on absolute multiples of P: aligned streams
            job.pieces.push_back(ScanPiece{a, (int32_t)(b - a), 0});
            a = b;
        }
    }
    if (!runs.empty()) {
        std::vector<std::pair<int64_t, int64_t>>& V = c->validated;
        V.insert(V.end(), runs.begin(), runs.end());
        std::sort(V.begin(), V.end());
        size_t w = 0;
        for (size_t i = 1; i < V.size(); i++) {
            if (V[i].first <= V[w].second) V[w].second = std::max(V[w].second, V[i].second);
            else V[++w] = V[i];
        }
        V.resize(w + 1);
        HIP_TRY(c->scan_pieces.ensure(sizeof(ScanPiece) * job.pieces.size()));
        const size_t b_pieces = sizeof(ScanPiece) * job.pieces.size();
        const void* src = job.pieces.data();
        if (c->h_pieces.ensure(b_pieces)) { memcpy(c->h_pieces.p, src, b_pieces); src = c->h_pieces.p; }      // (page-locked: the copy does not block, see build_job)
        HIP_TRY(hipMemcpyAsync(c->scan_pieces.p, src, b_pieces, hipMemcpyHostToDevice, c->sA));
    }
    return WGBSSEG_OK;
}

// The scan pass.  k_validate (per piece, read-only): the `meth <= cov` check of read_beta_file (segmentor.cpp:179-188) over the sites of the
// batch this API call has not checked yet; it needs nothing but the beta bytes, so a batch launches it first of all, beside the windows pass
// (round 6).  k_scan (per chunk, with carries + the same check): only for a job with wide scoring tiles — the one consumer of the carries —
// or a caller that wants them.
int launch_validate(wgbsseg_ctx* c, const Job& job, hipStream_t s, char* err, size_t errlen)
{
    if (job.pieces.empty()) return WGBSSEG_OK;
    const int64_t tasks = (int64_t)job.pieces.size() * job.v.n_samples;
    const int64_t vb = (tasks + (WG_BLOCK / 64) - 1) / (WG_BLOCK / 64);
    if (vb > 0x7fffffff) { set_err(err, errlen, "too many (piece, sample) rows"); return WGBSSEG_E_ARG; }
    hipLaunchKernelGGL(k_validate, dim3((unsigned)vb), dim3(WG_BLOCK), 0, s, job.v, c->status.as<JobStatus>(),
                       c->scan_pieces.as<ScanPiece>(), (int64_t)job.pieces.size());
    HIP_TRY(hipGetLastError());
    return WGBSSEG_OK;
}

int launch_scan(wgbsseg_ctx* c, const Job& job, hipStream_t s, char* err, size_t errlen)
{
    const int64_t rows = (int64_t)job.v.n_chunks * job.v.n_samples;      // wave tasks
    const int64_t blocks = (rows + (WG_BLOCK / 64) - 1) / (WG_BLOCK / 64);
    if (blocks > 0x7fffffff) { set_err(err, errlen, "too many (chunk, sample) rows"); return WGBSSEG_E_ARG; }
    hipLaunchKernelGGL(k_scan, dim3((unsigned)blocks), dim3(WG_BLOCK), 0, s, job.v, c->status.as<JobStatus>());
    HIP_TRY(hipGetLastError());
    return WGBSSEG_OK;
}

int report_bad_site(const wgbsseg_ctx* c, const JobStatus& st, char* err, size_t errlen)
{
    const long long s = (long long)(st.first_bad >> 40), site = (long long)(st.first_bad & ((1ULL << 40) - 1));
    uint8_t mc[2] = {0, 0};
    (void)hipMemcpy(mc, c->betas + s * c->pitch + 2 * site, 2, hipMemcpyDeviceToHost);
    set_err(err, errlen, "invalid data: sample %lld (0-based, argument order), site %lld (0-based): meth %d > cov %d",
            s, site + (long long)c->site_base, (int)mc[0], (int)mc[1]);
    return WGBSSEG_E_METH_GT_COV;
}

template <int TI, int FAST, int SPLIT>
hipError_t launch_cost(const JobView& v, const StageView& sv, const CostArgs& a, const TileDesc* td, int64_t tiles, double* cost, size_t lds, hipStream_t s)
{
    const int64_t padded = round_up(tiles, 8 * (int64_t)a.xcd_group);      // whole groups for every XCD; workgroups behind the last tile leave at once
    if (TI > 64 || a.NS >= v.n_samples)      // every sample in LDS at once: the form without partial sums across sample groups
        hipLaunchKernelGGL((k_cost<TI, FAST, SPLIT, true>), dim3((unsigned)padded), dim3(WG_BLOCK), lds, s, v, sv, a, td, tiles, cost, padded);
    else
        hipLaunchKernelGGL((k_cost<(TI > 64 ? 64 : TI), FAST, SPLIT, false>), dim3((unsigned)padded), dim3(WG_BLOCK), lds, s, v, sv, a, td, tiles, cost, padded);
    return hipGetLastError();
}

// k_cost of a tile class: 0 narrow tiles, TI start sites (128 / 64 / 32 / 16); 1 wide tiles, WG_WIDE_TS start sites x WG_WIDE_TK end sites;
// 2 medium tiles, WG_MEDIUM_TS start sites.  FAST = wg_term_mode of the pseudo count, or 3: mode 2 with the short division core
template <int FAST>
hipError_t launch_cost_fast(int cls, int TI, const JobView& v, const StageView& sv, const CostArgs& a, const TileDesc* td, int64_t tiles, double* cost, size_t lds, hipStream_t s)
{
    if (cls == 2) return launch_cost<WG_MEDIUM_TS, FAST, 2>(v, sv, a, td, tiles, cost, lds, s);
    if (cls == 1) return launch_cost<WG_WIDE_TS, FAST == 3 ? 2 : FAST, 1>(v, sv, a, td, tiles, cost, lds, s);      // (the short division is a form of the tiles with few operand pairs)
    if (TI == 128) return launch_cost<128, FAST, 0>(v, sv, a, td, tiles, cost, lds, s);
    if (TI == 64) return launch_cost<64, FAST, 0>(v, sv, a, td, tiles, cost, lds, s);
    if (TI == 32) return launch_cost<32, FAST, 0>(v, sv, a, td, tiles, cost, lds, s);
    return launch_cost<16, FAST, 0>(v, sv, a, td, tiles, cost, lds, s);
}
hipError_t launch_cost_class(int cls, int fast, int TI, const JobView& v, const StageView& sv, const CostArgs& a, const TileDesc* td, int64_t tiles, double* cost, size_t lds, hipStream_t s)
{
    return fast == 3 ? launch_cost_fast<3>(cls, TI, v, sv, a, td, tiles, cost, lds, s) : fast == 2 ? launch_cost_fast<2>(cls, TI, v, sv, a, td, tiles, cost, lds, s)
         : fast == 1 ? launch_cost_fast<1>(cls, TI, v, sv, a, td, tiles, cost, lds, s) : launch_cost_fast<0>(cls, TI, v, sv, a, td, tiles, cost, lds, s);
}

// Kernels that ask for more than 64 KB of dynamic LDS need the attribute on EVERY device they run on: set once per
// context, right after hipSetDevice (wgbsseg_create), and checked.
template <int FAST>
hipError_t set_cost_attrs()
{
    const void* fns[] = {reinterpret_cast<const void*>(&k_cost<128, FAST, 0, true>),
                         reinterpret_cast<const void*>(&k_cost<64, FAST, 0, true>), reinterpret_cast<const void*>(&k_cost<32, FAST, 0, true>),
                         reinterpret_cast<const void*>(&k_cost<16, FAST, 0, true>), reinterpret_cast<const void*>(&k_cost<WG_WIDE_TS, FAST == 3 ? 2 : FAST, 1, true>),
                         reinterpret_cast<const void*>(&k_cost<WG_MEDIUM_TS, FAST, 2, true>),
                         reinterpret_cast<const void*>(&k_cost<64, FAST, 0, false>), reinterpret_cast<const void*>(&k_cost<32, FAST, 0, false>),
                         reinterpret_cast<const void*>(&k_cost<16, FAST, 0, false>), reinterpret_cast<const void*>(&k_cost<WG_WIDE_TS, FAST == 3 ? 2 : FAST, 1, false>),
                         reinterpret_cast<const void*>(&k_cost<WG_MEDIUM_TS, FAST, 2, false>)};
    for (const void* f : fns) {
        const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
hipError_t set_kernel_attributes()
{
    hipError_t e = set_cost_attrs<0>();
    if (e == hipSuccess) e = set_cost_attrs<1>();
    if (e == hipSuccess) e = set_cost_attrs<2>();
    if (e == hipSuccess) e = set_cost_attrs<3>();
    const void* dps[] = {reinterpret_cast<const void*>(&k_dp<7, 64>), reinterpret_cast<const void*>(&k_dp<7, 64, true>),
                         reinterpret_cast<const void*>(&k_dp<7, 32>),
                         reinterpret_cast<const void*>(&k_dp<15, 32>)};
    for (const void* f : dps)
        if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    return e;
}

void grow_events(std::vector<Event>& v, size_t n)
{
    while (v.size() < n) { v.emplace_back(); (void)v.back().create(); }
}

typedef std::function<int32_t*(int64_t)> BorderAlloc;       // total border count -> destination (NULL: too small)

// Early delivery of a batch's result (the first batch of a region-level call; the destination must be page-locked, i.e. device-visible):
// the call returns when the CSR offsets, the lists of the items from `n_lead` on (junction patches) and the EDGES of the leading items'
// lists (the chunks: first / last WG_EDGE borders each) are on the host; the leading items' lists are still being written by k_copy_out
// and are complete after wait_pending_output().
struct EarlyOut {
    int64_t n_lead = 0;              // in: leading items whose lists may come late (0: no early delivery)
    bool dest_device_visible = false;   // in (set by the caller's BorderAlloc): the destination it handed out is page-locked memory the device can write
    const int32_t* edges = nullptr;  // out: [n_lead][front | back][WG_EDGE], the back right-aligned (valid until the context's next batch)
    bool pending = false;            // out: the leading lists are still on their way
};
int wait_pending_output(wgbsseg_ctx* c, char* err, size_t errlen)
{
    if (!c->out_pending) return WGBSSEG_OK;
    c->out_pending = false;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->evD));
    return WGBSSEG_OK;
}

// One chunk whose loci are not ascending, the reference's loops as written (csrc/plain_dp.h): ascending borders incl. 0 and len.
int plain_segment_chunk(wgbsseg_ctx* c, int64_t start0, int32_t n, const wgbsseg_params* P, std::vector<int32_t>& borders, char* err, size_t errlen)
{
    const int32_t W = (int32_t)std::min<int64_t>(P->max_cpg, n);
    // Ring of R rows of W doubles: the rows of the band in flight + the W - 1 rows before it that its steps still read.  ~1 GB of
    // ring while that holds at least W + 255 rows (W <= ~11,400); deeper windows take the floor W + 255 rows, i.e. up to W * n * 8
    // bytes (28.8 GB for max_cpg >= chunk = 60,000 — within an MI355X's 288 GB; E_NOMEM below when the device cannot give it).
    // WGBSSEG_PLAIN_RING_ROWS caps the rows (tests: the banded ring with R < n on chunks small enough for the suite).
    int64_t budget_rows = std::max<int64_t>((int64_t)W + 255, (1LL << 30) / ((int64_t)W * 8));
    const long long cap_rows = env_int("WGBSSEG_PLAIN_RING_ROWS", 0);      // (read per batch: a test sets it on a live context)
    if (cap_rows > 0) budget_rows = std::max<int64_t>((int64_t)W, (int64_t)cap_rows);     // R >= W keeps the band >= 1 row
    const int32_t R = (int32_t)std::min<int64_t>(n, budget_rows);
    const int32_t band = R >= n ? n : R - (W - 1);
    DevBuf buf, M, T, bad;      // (this call's alone: they go when it returns)
    if (buf.ensure((size_t)W * (size_t)R * 8) != hipSuccess || M.ensure((size_t)(n + 1) * 8) != hipSuccess || T.ensure((size_t)(n + 1) * 4) != hipSuccess ||
        bad.ensure(8) != hipSuccess) {
        (void)hipGetLastError();
        set_err(err, errlen, "out of device memory for the plain recurrence of a chunk with non-ascending loci (%d sites, max_cpg %d)", (int)n, (int)W);
        return WGBSSEG_E_NOMEM;
    }
    JobStatus st = {};
    st.first_bad = ~0ULL;
    HIP_TRY(hipMemcpyAsync(bad.p, &st.first_bad, 8, hipMemcpyHostToDevice, c->sA));
    PlainArgs A = {c->betas, c->pitch, c->n_total, c->n_samples, c->loci, start0, n, W, P->max_bp, P->pseudo_count, P->pseudo_count + P->pseudo_count,
                   R, buf.as<double>(), M.as<double>(), T.as<int32_t>(), bad.as<unsigned long long>()};
    for (int32_t b0 = 0; b0 < n; b0 += band) {
        const int32_t b1 = (int32_t)std::min<int64_t>(n, (int64_t)b0 + band);
        hipLaunchKernelGGL(k_plain_rows, dim3((unsigned)((b1 - b0 + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0, c->sA, A, b0, b1);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_plain_dp, dim3(1), dim3(WG_BLOCK), 0, c->sA, A, b0, b1);
        HIP_TRY(hipGetLastError());
    }
    std::vector<int32_t> hT((size_t)n + 1);
    HIP_TRY(hipMemcpyAsync(hT.data(), T.p, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipMemcpyAsync(&st.first_bad, bad.p, 8, hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    if (st.first_bad != ~0ULL) return report_bad_site(c, st, err, errlen);
    borders.clear();                                          // segmentor.cpp:50-58: i = n; push; while i > 0: i = max(0, T[i]); push — printed in reverse
    int32_t i = n;
    borders.push_back(i);
    while (i > 0) {
        const int32_t t = hT[(size_t)i];
        const int32_t nx = t > 0 ? t : 0;
        if (nx >= i) { set_err(err, errlen, "internal: back-pointer %d at step %d of a plain recurrence", (int)t, (int)i); return WGBSSEG_E_STATE; }
        i = nx;
        borders.push_back(i);
    }
    std::reverse(borders.begin(), borders.end());
    return WGBSSEG_OK;
}

// ---- one batch: a plan decided on the host, then the phases that launch it ------------------------------------------------

// How a batch is tiled, staged and recurred, decided on the host from the window statistics (plan_tiles, plan_stages: no HIP call).  Tile classes: 0 narrow, 1 wide, 2 medium.
struct BatchPlan {
    int Wmax = 0;                  // the job's widest window
    int WA = 0;                    // widest window of a narrow tile: min(Wmax, WG_NARROW_WMAX)
    int WMED = 0;                  // widest window of a medium tile (0: no medium class)
    int term_mode[3] = {};         // per class: the form of the likelihood term (wg_term_mode)
    int rows[3] = {};              // per class: exponent rows of the k-scaled lookup tables (term mode 2 only)
    int TI = 64;                   // start sites of a narrow tile
    int NS[3] = {1, 1, 1};         // per class: samples per LDS group
    size_t lds[3] = {};            // per class: dynamic LDS of k_cost
    int n_stages = 1;
    bool gated = false;            // the stages alternate between the two scoring streams behind k_stage_gate
    int last_pct = 100;            // length of the last stage in percent of the others'
    const int32_t* sb = nullptr;   // [n_stages + 1] stage bounds (held by the context: the source of an async upload)
    bool all_narrow = false;       // no window beyond the narrow tiles': the tile and pair counts below are the host's own
    std::vector<int64_t> stage_pairs, stage_tiles;   // per stage: scored blocks; tiles per class at [3 * stage + class] (read back from k_stage_plan unless all narrow)
    int dp_mode = 0;               // k_dp: 0 64-step batches, 1 32-step batches, 2 the same with 15 worker waves (deep windows)
    int ringN = 0; int64_t state_stride = 0;   // k_dp's ring of pending maxima (0: none) and its state per chunk, in doubles
    int nbuf = 1;                  // scored-block buffers
    int live_ctx = 0;              // contexts alive on the device when the plan was made (what `gated` saw)
};

// dynamic LDS of a k_cost tile of class cls with ti start sites and ns samples per LDS group
size_t cost_lds(const BatchPlan& p, int ti, int cls, int ns)
{
    const int wm = cls == 2 ? WG_MEDIUM_WMAX : WG_NARROW_WMAX;
    const size_t rows = cls == 1 ? ((((size_t)ns * (WG_WIDE_TK + 1 + WG_WIDE_TS + 1) + 1) & ~(size_t)1) * 8)    // P of the ends + P of the starts, (meth, cov) as two dwords
                                 : ((((size_t)ns * (ti + wm + 1) + 3) & ~(size_t)3) * 4);             // tile-local prefixes, packed in one dword
    // guard-free kernels: just the two lookup tables, sized to the pseudo count and the tile class; otherwise the general fast tables
    const size_t tabs = p.term_mode[cls] == 2 ? (size_t)p.rows[cls] * (16 + 64) * sizeof(wg_d2) : sizeof(wg_fast_tables);
    // one 16-byte record per start (+ the closing one), 8 ints, and for narrow / medium tiles the block -> start map: a byte per eight blocks + forward steps
    // (CostArgs::cmap = 3; a byte per block was measured for small cohorts, x8 scoring 6.73 ms against 6.59, x16 12.50 / 12.07: profiles/r04_cost_rec_ab.txt)
    return tabs + rows + (size_t)(ti + 1) * 16 + 32 + (cls == 1 ? 0 : ((size_t)ti * wm >> 3) + 8);
}

// Tiling of the scoring kernel.
// Narrow tiles (class 0): TI aligned start sites whose windows are all <= WA = min(widest window, WG_NARROW_WMAX);
// LDS per workgroup: fast log tables + NS sample rows of TI+61 tile-local prefixes (one packed dword each) + small
// per-tile arrays.  The kernel is a long dependent chain per evaluation, so resident wavefronts matter: pick the
// shape that maximises (workgroups per CU) x (lane occupancy of the block rounds).
// Wide tiles (class 1): 16 start sites x 128 end sites, for every 16-site unit that shares an aligned TI-group with
// a window > WA (CpG islands; everything in deep mode); prefixes of starts and ends as (meth, cov) dword pairs.
// Medium tiles (class 2, round 3): units of a non-narrow group whose windows stay <= WG_MEDIUM_WMAX = 252 sites (block counts < 2^16): CpG islands.
int plan_tiles(const wgbsseg_ctx* c, const Job& job, const JobStatus& st, float pc, BatchPlan& p, char* err, size_t errlen)
{
    p.Wmax = (int)st.max_window;
    p.WA = std::min(p.Wmax, WG_NARROW_WMAX);
    p.WMED = c->medium_wmax;
    // exponent rows of the k-scaled log tables (pseudo count >= 1): narrow tiles score blocks of <= WG_NARROW_WMAX sites,
    // wide tiles blocks up to the job's widest window
    // The guard-free form of the term (pseudo count >= 1) rests on block totals below 2^21 (csrc/exact_log2.h: p < 1 after the
    // three float roundings, table rows down to 2^-23): the narrow tiles (blocks of <= 60 sites) always have them, the wide
    // tiles only while 255 * (the job's widest window) < 2^21 — windows beyond 8224 sites (max_cpg > 8000: round 3) score with
    // the general guarded form, which assumes nothing about the totals.
    const int tmA = wg_term_mode(pc);
    const int tmB = (tmA == 2 && 255.0 * std::max(p.Wmax, 1) >= 0x1p21) ? 1 : tmA;
    p.term_mode[0] = p.term_mode[2] = tmA;
    p.term_mode[1] = tmB;
    p.rows[0] = tmA == 2 ? wg_lookup_rows(pc, 255.0 * WG_NARROW_WMAX) : 0;
    p.rows[1] = tmB == 2 ? wg_lookup_rows(pc, 255.0 * std::max(p.Wmax, 1)) : 0;
    p.rows[2] = tmA == 2 ? wg_lookup_rows(pc, 255.0 * WG_MEDIUM_WMAX) : 0;
    if (p.rows[0] > WG_KY_KMIN + 1 || p.rows[1] > WG_KY_KMIN + 1 || p.rows[2] > WG_KY_KMIN + 1) {
        set_err(err, errlen, "internal: %d / %d / %d lookup rows", p.rows[0], p.rows[1], p.rows[2]);
        return WGBSSEG_E_ARG;
    }
    const int Nsmp = (int)c->n_samples;
    const double Favg = (double)(int64_t)st.total_pairs / (double)std::max<int64_t>(1, job.sites);
    const int ti128_max_n = 16;
    double best = -1;
    for (int ti = 128; ti >= 16; ti >>= 1) {
        if (c->force_ti > 0 && ti != c->force_ti) continue;
        for (int ns : {Nsmp, 32, 16, 8, 4}) {
            if (ns > Nsmp) continue;
            // 128-start tiles: half the per-tile overhead for small cohorts; only with every sample in LDS at once (one group),
            // and not by default above 16 samples, where their larger rows cost a workgroup per CU
            if (ti == 128 && (ns != Nsmp || (c->force_ti != 128 && Nsmp > ti128_max_n))) continue;
            if (c->force_ns > 0 && ns != std::min(c->force_ns, Nsmp)) continue;
            const size_t l = cost_lds(p, ti, 0, ns);
            if (l > 64 * 1024) continue;
            // workgroups per CU the score counts on: LDS is handed out in granules of 1280 bytes; 5 for the 64-start tiles and below (the form
            // with partial sums across sample groups has 95 VGPRs = 5 per CU; the one-group form has 63, but letting it count 7 makes small
            // cohorts pick 64-start tiles, measured slower than 128-start ones: x8 scoring 6.92 vs 6.59 ms, profiles/r04_cost_rec_ab.txt)
            const int wgs = (int)std::min<size_t>(ti == 128 ? 8 : 5, (160 * 1024) / (size_t)round_up((int64_t)l, 1280));
            const double q = ti * std::min<double>(Favg, p.WA), eff = q / (256.0 * std::ceil(q / 256.0));
            const double groups = std::ceil((double)Nsmp / ns);
            const double score = wgs * eff / (1.0 + 0.02 * (groups - 1)) * (1.0 + 0.04 * (ti / 16));   // bias to big tiles (less staging)
            if (score > best) { best = score; p.TI = ti; p.NS[0] = ns; }
        }
    }
    if (best < 0) { p.TI = 16; p.NS[0] = 1; }
    // wide and medium tiles: the samples per group that fit the most workgroups per CU (wide: 103 VGPRs, 4 at most; medium: rows of 269 dwords per sample, 5)
    auto pick_ns = [&](int cls, int ti, int max_wgs, bool forced) {
        int pick = 1;
        double top = -1;
        for (int ns : {Nsmp, 32, 16, 8, 4, 1}) {
            if (ns > Nsmp) continue;
            if (forced && c->force_ns > 0 && ns != std::min(c->force_ns, Nsmp)) continue;
            const size_t l = cost_lds(p, ti, cls, ns);
            if (l > 64 * 1024) continue;
            const int wgs = (int)std::min<size_t>(max_wgs, (160 * 1024) / (size_t)round_up((int64_t)l, 1280));
            const double score = wgs / (1.0 + 0.02 * (std::ceil((double)Nsmp / ns) - 1));
            if (score > top) { top = score; pick = ns; }
        }
        return pick;
    };
    p.NS[1] = pick_ns(1, WG_WIDE_TS, 4, true);
    p.NS[2] = pick_ns(2, WG_MEDIUM_TS, 5, false);
    const int tile_ti[3] = {p.TI, WG_WIDE_TS, WG_MEDIUM_TS};
    for (int k = 0; k < 3; k++) p.lds[k] = (size_t)round_up((int64_t)cost_lds(p, tile_ti[k], k, p.NS[k]), 16);
    return WGBSSEG_OK;
}

// Stages: bound the scored-block buffer and overlap scoring (stream A) with the recurrence (stream B); the recurrence kernel's form.
void plan_stages(wgbsseg_ctx* c, const Job& job, const JobStatus& st, BatchPlan& p)
{
    const int64_t total_pairs = (int64_t)st.total_pairs;
    const long long bytes = total_pairs * 8;
    int n_stages = (int)std::max<long long>(1, (bytes + c->cost_budget_bytes - 1) / c->cost_budget_bytes);
    // Few chunks (one rank's share of a sharded genome): the recurrence occupies a fraction of the CUs, so let it
    // chase the scoring kernel stage by stage (measured: 71 chunks 10.1 -> 8.7 ms, 132 chunks 16.2 -> 15.0 ms).  With
    // hundreds of chunks k_dp alone (3.9 ms per 60k-site chunk, all chunks at once) beats k_dp competing for CUs.
    // (the junction patches that ride along in the batch are a few hundred sites each: they do not count)
    int n_long = 0;
    for (const ChunkDesc& d : job.h) n_long += d.len >= 8192;
    // ... unless the recurrence is the longer of the two anyway (a share of a SMALL cohort): beside the scoring kernel a step of the recurrence
    // takes ~50 ns against ~21 alone, so staging pays only when the scoring lasts longer than the ~30 ns per step it costs: at 7e11
    // evaluations/s, from ~21,000 evaluations per step of the longest chunk on (round 6, one GPU's share of 8, 71 chunks: x 8 3.69 ms in eight
    // stages, 2.63 in one; x 32 4.09 against 5.08; profiles/r06_stage_gate_ab.txt)
    const bool worth = (double)total_pairs * c->n_samples >= (double)job.max_len * c->stage_min_evals_per_step;
    if (job.max_len >= 8192) n_stages = std::max(n_stages, n_long <= 160 && worth ? 8 : 1);
    // Many chunks, all windows <= 64: one stage scores and k_dp<7,64> follows alone (1.7 ms exposed).  (Two uneven stages — the
    // recurrence of the first part of every chunk beside the scoring of the rest — were measured in round 2: 27.1-27.3 ms against 27.0
    // whatever the split, profiles/r02_tail_split_sweep.txt: the scoring kernel loses what the recurrence no longer shows.)
    if (c->force_stages > 0) n_stages = c->force_stages;
    n_stages = std::min<int>(n_stages, std::max(1, (job.max_len + 63) / 64));
    // Gated stages (k_stage_gate): the two scoring streams swap roles from stage to stage — the narrow tiles of an even stage on A with its medium / wide tiles
    // beside them on A2, an odd stage the other way round (a second PAIR of streams was measured: six streams of one priority share hardware queues, every
    // share lost 10-15 %)
    p.all_narrow = p.Wmax <= WG_NARROW_WMAX;
    // (one context per device: the streams of several contexts share hardware queues, where a gate could sit ahead of the very launch another context's gate waits for —
    // the waits are bounded, but nothing would be gained)
    // A job with medium / wide tiles (its recurrences are the 32-step kernels with the full LDS footprint, which lived on the drains: a share of 8, x 32 with islands,
    // 5.95 -> 6.4 ms under the gate) is gated only when it is clearly scoring-bound (x 100 with islands: 14.0 -> 13.3 ms): from 100,000 evaluations per step on.
    const double evals_per_step = (double)total_pairs * c->n_samples / std::max<double>(1.0, (double)job.max_len);
    p.live_ctx = g_live_ctx[c->device & 63].load(std::memory_order_relaxed);
    p.gated = c->stage_gate > 0 && n_stages > 1 && (p.all_narrow || evals_per_step >= c->stage_gate_wide_evals || c->stage_gate_shared) &&
              (c->stage_gate_shared || p.live_ctx == 1);
    // equal stages but the last (gated jobs only): its recurrence is the only one that runs with the chip to itself, at twice the pace of the others.
    // Which length: the recurrences of the other stages take ~50 ns per step beside the scoring, so while the scoring of a stage lasts no longer than 1.5 x its
    // recurrence (at 7e11 evaluations/s: up to ~52,000 evaluations per step of the longest chunk) the chain of recurrences is what the step waits for, and a last
    // stage three times the others' shortens it (a share of 8, x 32: 4.08 -> 3.79 ms with the gate; equal stages + gate alone: 4.2); a scoring-bound job keeps equal
    // stages (x 200: 20.4 -> 18.35 ms with the gate, 18.7 with a last stage twice the others').  profiles/r06_stage_gate_ab.txt
    p.last_pct = !p.gated ? 100 : (c->last_stage_pct > 0 ? c->last_stage_pct : (evals_per_step <= 52500.0 ? 300 : 100));
    const double parts = n_stages > 1 ? (double)(n_stages - 1) + p.last_pct / 100.0 : 1.0;
    const int S = (int)round_up((int64_t)std::ceil((double)job.max_len / parts), 64);
    n_stages = std::min<int>(n_stages, (job.max_len + S - 1) / S);
    std::vector<int32_t>& sb = c->h_stage_bounds;
    sb.resize((size_t)n_stages + 1);
    for (int q = 0; q < n_stages; q++) sb[(size_t)q] = (int32_t)std::min<int64_t>((int64_t)q * S, job.max_len);
    sb[(size_t)n_stages] = (int32_t)job.max_len;
    p.sb = sb.data();
    p.n_stages = n_stages;
    p.stage_pairs.assign((size_t)n_stages, 0);
    p.stage_tiles.assign((size_t)n_stages * 3, 0);
    // No window beyond the narrow tiles' (every default-parameter genome outside CpG islands): every aligned group of TI starts is ONE narrow
    // tile, so the host knows the tile counts without asking the device (round 6: one host round trip less in front of the scoring of every
    // batch); the scored blocks per stage — what sizes the cost buffer — from the windows' statistics: all of them in one stage, at most
    // (sites of the stage) x (widest window) otherwise.
    if (p.all_narrow) {
        for (int stg = 0; stg < n_stages; stg++) {
            int64_t nt = 0, sites_in = 0;
            for (const ChunkDesc& d : job.h) {
                const int64_t s0 = sb[(size_t)stg], s1 = std::min<int64_t>(sb[(size_t)stg + 1], d.len);
                if (s1 > s0) { nt += (s1 - s0 + p.TI - 1) / p.TI; sites_in += s1 - s0; }
            }
            p.stage_tiles[3 * (size_t)stg] = nt;
            p.stage_pairs[(size_t)stg] = n_stages == 1 ? total_pairs : std::min<int64_t>(total_pairs, sites_in * std::max(p.Wmax, 1));
        }
    }
    p.nbuf = n_stages > 1 ? (p.gated && n_stages > 2 ? 3 : 2) : 1;      // (gated: a stage's scoring must not wait for the recurrence two stages back when its gate opens)
    // k_dp: 64-step batches when no window of the job exceeds 64 sites; otherwise 32-step batches with a second pending
    // register per lane and, for blocks longer than 128 sites, a ring of pending maxima per chunk in global memory
    p.dp_mode = std::max(p.Wmax > 512 ? 2 : (p.Wmax > 64 ? 1 : 0), c->force_dp_mode);
    p.ringN = p.dp_mode ? ceil_pow2(p.Wmax + 128) : 0;
    p.state_stride = round_up(WG_DP_STATE_HDR + (int64_t)p.ringN + (p.ringN + 1) / 2, 2);
}

// k_check_div on stream A: is the short division core exact on every operand pair of a block of <= wmax sites?  Its verdict (0: yes) lands in dst.
int queue_div_check(wgbsseg_ctx* c, float pc, int wmax, void* dst, char* err, size_t errlen)
{
    HIP_TRY(c->divcheck.ensure(4));
    HIP_TRY(hipMemsetAsync(c->divcheck.p, 0, 4, c->sA));
    const int max_total = 255 * wmax;
    hipLaunchKernelGGL(k_check_div, dim3((unsigned)max_total + 1), dim3(WG_BLOCK), 0, c->sA, pc, pc + pc, max_total, c->divcheck.as<unsigned int>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(dst, c->divcheck.p, 4, hipMemcpyDeviceToHost, c->sA));
    return WGBSSEG_OK;
}

// One batch in flight: the call, its job, statistics and plan, where its results go.  segment_chunks_impl runs its phases in this order.
struct Batch {
    wgbsseg_ctx* c = nullptr;
    // the call as the caller made it
    const int64_t* chunk_start0 = nullptr; const int32_t* chunk_len = nullptr; int64_t n_chunks = 0;
    const BorderAlloc* alloc = nullptr; int64_t* borders_off = nullptr; EarlyOut* early = nullptr;
    bool allow_plain = true;
    wgbsseg_params P = {};               // the parameters with max_cpg cut to the longest chunk of the call
    Job job;
    int nC = 0; int64_t J = 0;           // chunks and sites of the batch
    JobStatus* hst = nullptr;            // page-locked landing area: [0] the window statistics, [1] / [3] k_check_div's verdicts (narrow / medium), [2] the scan's verdict
    JobStatus st = {};                   // the window statistics
    BatchPlan plan;
    CostArgs ca[3];                      // per tile class
    std::vector<int64_t> tile0[3];       // per tile class: first tile of every stage (+ the total)
    std::vector<int32_t> ran_dp16;       // per stage: 1 when its recurrence was launched as k_dp16 (wgbsseg_debug_last_plan)
    DevBuf* outb = nullptr; size_t out_head = 0;   // the result on the device: the CSR offsets, then from out_head the border lists
    bool marks = false;                  // (WGBSSEG_PROFILE=2) host clock: entry, tables up, windows queued, statistics here, scoring queued, everything queued, results here, return
    double hm[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    void mark(int i) { if (marks) hm[i] = wall_s(); }

    int front(char* err, size_t errlen);           // the scan pass starts with the batch on its own stream (round 6); the windows pass; the window statistics come home
    int disorder_exit(char* err, size_t errlen);   // loci not ascending inside a chunk, or a chunk of more than 2^32 blocks: the batch ends after the front
    int tile_plan(char* err, size_t errlen);       // lookup tables and stage bounds up, tiles counted (k_tile_count: not all narrow), laid out (k_stage_plan), written (k_tile_emit)
    int stages(char* err, size_t errlen);          // per stage: its scoring (stream A, A2 beside it), then its recurrence (stream B)
    int deliver(char* err, size_t errlen);         // traceback, the border lists and their CSR offsets, home (one copy, or early delivery)
    int timings(char* err, size_t errlen);         // the device time line (WGBSSEG_PROFILE=2) and the context's totals
};

// One batch: the front, the host's plan (plan_tiles, plan_stages), the tile plan, the stages, traceback and delivery, timings.
int segment_chunks_impl(wgbsseg_ctx* c, const int64_t* chunk_start0, const int32_t* chunk_len, int64_t n_chunks,
                        const wgbsseg_params* P, const BorderAlloc& alloc, int64_t* borders_off, char* err, size_t errlen, bool allow_plain = true, EarlyOut* early = nullptr)
{
    if (!P || !borders_off) { set_err(err, errlen, "NULL params/borders pointer"); return WGBSSEG_E_ARG; }
    if (P->max_bp == 0) { set_err(err, errlen, "max_bp must be >= 1 (the reference reads uninitialised loci when it is 0: segmentor.cpp:38,114)"); return WGBSSEG_E_ARG; }
    if (P->max_cpg < 1) { set_err(err, errlen, "max_cpg must be >= 1"); return WGBSSEG_E_ARG; }
    // The reference sizes its ring to any max_cpg (segmentor.cpp:92-95).  What bounds it here: a block's counts must stay exact in
    // the float sums of segmentor.cpp:122-123 (255 * max_cpg < 2^24: beyond that the REFERENCE's own sums round),
    // and a window is stored in 16 bits.  A window never exceeds its chunk (segmentor.cpp:110: j < n - i), so max_cpg counts
    // only up to the longest chunk of the call.
    int32_t longest = 1;
    if (chunk_len) for (int64_t i = 0; i < n_chunks; i++) longest = std::max(longest, chunk_len[i]);
    Batch b;
    b.c = c; b.chunk_start0 = chunk_start0; b.chunk_len = chunk_len; b.n_chunks = n_chunks;
    b.alloc = &alloc; b.borders_off = borders_off; b.early = early; b.allow_plain = allow_plain;
    b.P = *P;
    b.P.max_cpg = std::min<uint32_t>(P->max_cpg, (uint32_t)longest);
    if ((uint64_t)b.P.max_cpg * 255u >= (1u << 24) || b.P.max_cpg > WGBSSEG_MAX_CPG) {
        set_err(err, errlen, "max_cpg %u with chunks of up to %d sites unsupported: blocks of more than %d sites (255 * sites >= 2^24) do not keep their counts exact "
                "in the float sums of the reference itself (segmentor.cpp:122-123), and windows are stored in 16 bits", P->max_cpg, (int)longest, WGBSSEG_MAX_CPG);
        return WGBSSEG_E_ARG;
    }
    b.marks = c && c->batch_marks;
    b.mark(0);
    if (!(P->pseudo_count >= 0.0f)) { set_err(err, errlen, "pseudo_count must be >= 0"); return WGBSSEG_E_ARG; }
    // A batch that failed half way may have left work behind on the scoring / scan streams that reads the staging areas: such a context is drained before it is
    // used again.  (A clean one is NOT synchronised stream by stream here: the follow-up batch of an early delivery starts while k_copy_out still writes the first
    // batch's lists, and a stream synchronisation — a marker of its own in a hardware queue the streams share — waited ~0.13 ms behind that kernel.)
    if (c && c->batch_open) {
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipDeviceSynchronize());
        c->out_pending = false;
    }
    if (c) c->batch_open = true;
    int rc = build_job(c, chunk_start0, chunk_len, n_chunks, b.job, true, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    rc = plan_validation(c, b.job, !c->accumulate, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    c->last_valid = false;
    b.nC = (int)n_chunks;
    b.J = b.job.sites;

    rc = b.front(err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    if (b.st.loci_disorder || b.st.overflow) return b.disorder_exit(err, errlen);
    rc = plan_tiles(c, b.job, b.st, b.P.pseudo_count, b.plan, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    plan_stages(c, b.job, b.st, b.plan);
    rc = b.tile_plan(err, errlen);
    if (rc == WGBSSEG_OK) rc = b.stages(err, errlen);
    if (rc == WGBSSEG_OK) rc = b.deliver(err, errlen);
    if (rc == WGBSSEG_OK) rc = b.timings(err, errlen);
    return rc;
}

int Batch::front(char* err, size_t errlen)
{
    JobView& v = job.v;
    const int64_t Jp = job.sites_padded;                         // every chunk's slice of the job-site arrays begins at a multiple of 8 entries
    const int64_t nT = job.wtile_off[(size_t)nC];                // 1024-site tiles of the windows pass
    if (nT > 0x7fffffff) { set_err(err, errlen, "too many sites in one call"); return WGBSSEG_E_ARG; }
    HIP_TRY(c->W16.ensure((size_t)Jp * 2 + 16));
    HIP_TRY(c->cum32.ensure((size_t)Jp * 4 + 16));
    HIP_TRY(c->back16.ensure((size_t)Jp * 2 + 16));
    HIP_TRY(c->chunk_pairs.ensure((size_t)nC * 8));
    HIP_TRY(c->umax16.ensure((size_t)job.units * 2));
    HIP_TRY(c->tile_tot.ensure((size_t)nT * 4));
    HIP_TRY(c->tile_base.ensure((size_t)nT * 4));
    HIP_TRY(c->tile_chunk.ensure((size_t)nT * 16));          // (one int4 record per tile)
    v.W16 = c->W16.as<uint16_t>(); v.cum32 = c->cum32.as<uint32_t>(); v.back16 = c->back16.as<uint16_t>();
    v.chunk_pairs = c->chunk_pairs.as<int64_t>(); v.umax16 = c->umax16.as<uint16_t>();
    if (!c->h_status.ensure(4 * sizeof(JobStatus))) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    hst = reinterpret_cast<JobStatus*>(c->h_status.p);

    // k_validate needs the beta bytes and the list of pieces, nothing from the windows: it runs beside k_window (HBM-bound beside
    // instruction-bound) instead of behind it, and the scoring kernel of a job without wide tiles — which needs nothing from the scan
    // but its verdict, read at the end of the batch — no longer queues behind either.  (Rounds 1-5: windows 0.28 ms, then the scan
    // 0.32 ms, then the tile plan: scoring began 0.71 ms into the hg19 x 32 batch.)
    mark(1);
    HIP_TRY(hipEventRecord(c->ev[EV_BEGIN], c->sA));
    HIP_TRY(hipEventRecord(c->ev[EV_UPLOADED], c->sA));
    HIP_TRY(hipStreamWaitEvent(c->sC, c->ev[EV_UPLOADED], 0));
    HIP_TRY(hipEventRecord(c->ev[EV_VALIDATE0], c->sC));
    int rc = launch_validate(c, job, c->sC, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    HIP_TRY(hipEventRecord(c->ev[EV_VALIDATE1], c->sC));

    // a pseudo count this context has not scored with yet: may the narrow tiles use the short division core?  Every operand
    // pair they can form is tried on the device (0.1 ms, once); the verdict arrives with the window statistics.
    const bool check_div = c->divs_enabled && wg_term_mode(P.pseudo_count) == 2 && c->divs_pc != P.pseudo_count;
    if (check_div && (rc = queue_div_check(c, P.pseudo_count, WG_NARROW_WMAX, hst + 1, err, errlen)) != WGBSSEG_OK) return rc;
    // the search's first step when a wavefront has windows of 64 sites and more: 2^floor(log2(max_cpg - 1))
    int top_step = 1;
    while (2 * (int64_t)top_step <= (int64_t)P.max_cpg - 1) top_step *= 2;
    // loci of a 1024-site tile, of the site before it and of everything a PROBE of its searches can touch, in LDS (<= 48 KB; deeper windows search in L2)
    const int64_t win_want = 1 + (int64_t)WG_WIN_TILE + 2 * (int64_t)std::max(top_step, 32) + 8;
    const int win_lds = win_want <= 12288 ? (int)win_want : 0;
    const int64_t* const d_wtile = c->wtile.as<int64_t>();
    hipLaunchKernelGGL(k_window, dim3((unsigned)nT), dim3(WG_BLOCK), (size_t)win_lds * 4, c->sA, v, c->status.as<JobStatus>(),
                       d_wtile, reinterpret_cast<const int32_t*>(d_wtile + nC + 1), P.max_cpg, P.max_bp, win_lds, top_step, std::max(c->medium_wmax, WG_NARROW_WMAX),
                       c->tile_tot.as<uint32_t>(), c->tile_chunk.as<int4>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_window_scan, dim3((unsigned)nC), dim3(WG_BLOCK), 0, c->sA, v, c->status.as<JobStatus>(), d_wtile, c->tile_tot.as<uint32_t>(), c->tile_base.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[EV_WINDOWS], c->sA));
    HIP_TRY(hipMemcpyAsync(&hst[0], c->status.p, sizeof(JobStatus), hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipEventRecord(c->ev[EV_STATS], c->sA));
    // (the row offsets are not in the statistics: this pass runs while the host reads them and plans the tiles)
    hipLaunchKernelGGL(k_window_cum, dim3((unsigned)((nT + WG_CUM_TILES - 1) / WG_CUM_TILES)), dim3(WG_BLOCK), 0, c->sA, (const uint16_t*)v.W16, v.cum32, (const int4*)c->tile_chunk.as<int4>(),
                       (const uint32_t*)c->tile_base.as<uint32_t>(), nT);
    HIP_TRY(hipGetLastError());
    mark(2);
    HIP_TRY(hipEventSynchronize(c->ev[EV_STATS]));              // window statistics are here; the scan pass is still running
    mark(3);
    st = hst[0];
    if (check_div) {
        c->divs_ok = *reinterpret_cast<const unsigned int*>(&hst[1]) == 0u;
        c->divs_pc = P.pseudo_count;
        if (profiling()) fprintf(stderr, "[wgbsseg] short division core for pseudo count %g: %s\n", (double)P.pseudo_count, c->divs_ok ? "verified on every operand pair of a narrow tile" : "NOT exact, the full core stays");
    }
    // wide tiles read the carries of k_scan: behind k_validate on the scan stream, as soon as the windows are known
    if (st.wide_units && !st.loci_disorder && !st.overflow) {
        HIP_TRY(hipStreamWaitEvent(c->sC, c->ev[EV_WINDOWS], 0));
        HIP_TRY(hipEventRecord(c->ev[EV_SCAN0], c->sC));
        rc = launch_scan(c, job, c->sC, err, errlen);
        if (rc != WGBSSEG_OK) return rc;
        HIP_TRY(hipEventRecord(c->ev[EV_SCAN1], c->sC));
    }
    // the scan's verdict, read at the end of the batch
    HIP_TRY(hipEventRecord(c->ev[EV_SCAN_END], c->sC));
    HIP_TRY(hipMemcpyAsync(&hst[2], c->status.p, sizeof(JobStatus), hipMemcpyDeviceToHost, c->sC));
    HIP_TRY(hipEventRecord(c->evS, c->sC));
    return WGBSSEG_OK;
}

int Batch::disorder_exit(char* err, size_t errlen)
{
    JobStatus st2;                                        // the scan's verdict takes precedence, as it always has
    HIP_TRY(hipStreamSynchronize(c->sC));
    HIP_TRY(hipStreamSynchronize(c->sA));
    HIP_TRY(hipMemcpyAsync(&st2, c->status.p, sizeof(st2), hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    if (st2.first_bad != ~0ULL) return report_bad_site(c, st2, err, errlen);
    if (!st.loci_disorder) { set_err(err, errlen, "a chunk scores more than 2^32 blocks; use a smaller chunk_size"); return WGBSSEG_E_ARG; }
    if (!allow_plain) {
        set_err(err, errlen, "internal: loci not ascending inside chunk %u (0-based sites [%lld, +%d)) of a batch that was filtered for such chunks",
                st.loci_disorder - 1, (long long)(job.h[st.loci_disorder - 1].start0 + c->site_base), (int)job.h[st.loci_disorder - 1].len);
        return WGBSSEG_E_LOCI_ORDER;
    }
    // loci not ascending inside a chunk: the reference bars such an extension and leaves the site out of its running sums
    // (segmentor.cpp:114-117).  The batch path rests on ascending loci (windows, prefix sums); the chunks concerned (k_find_disorder) take
    // the plain path (csrc/plain_dp.h: the reference's loops as written), the rest of the batch runs again without them, and the border
    // lists are put back in the caller's order.
    DevBuf flags;
    HIP_TRY(flags.ensure((size_t)n_chunks * 4));
    HIP_TRY(hipMemsetAsync(flags.p, 0, (size_t)n_chunks * 4, c->sA));
    hipLaunchKernelGGL(k_find_disorder, dim3((unsigned)n_chunks), dim3(WG_BLOCK), 0, c->sA, job.v, flags.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> hf((size_t)n_chunks);
    HIP_TRY(hipMemcpyAsync(hf.data(), flags.p, (size_t)n_chunks * 4, hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    std::vector<int64_t> os, ooff;
    std::vector<int32_t> ol, ob;
    for (int64_t i = 0; i < n_chunks; i++) if (!hf[(size_t)i]) { os.push_back(chunk_start0[i]); ol.push_back(chunk_len[i]); }
    if (!os.empty()) {
        ooff.resize(os.size() + 1);
        const int rc = segment_chunks_impl(c, os.data(), ol.data(), (int64_t)os.size(), &P,
                                           [&](int64_t total) { ob.resize((size_t)std::max<int64_t>(1, total)); return ob.data(); }, ooff.data(), err, errlen, false);
        if (rc != WGBSSEG_OK) return rc;
    }
    std::vector<std::vector<int32_t>> plain((size_t)n_chunks);
    for (int64_t i = 0; i < n_chunks; i++)
        if (hf[(size_t)i]) {
            wgbsseg_params Pc = P;                             // (max_cpg is already cut to the longest chunk of the call; the kernels cut it to this chunk)
            const int rc = plain_segment_chunk(c, chunk_start0[i], chunk_len[i], &Pc, plain[(size_t)i], err, errlen);
            if (rc != WGBSSEG_OK) return rc;
        }
    int64_t total = 0;
    size_t oi = 0;
    for (int64_t i = 0; i < n_chunks; i++) {
        borders_off[i] = total;
        if (hf[(size_t)i]) total += (int64_t)plain[(size_t)i].size();
        else { total += ooff[oi + 1] - ooff[oi]; oi++; }
    }
    borders_off[n_chunks] = total;
    int32_t* out = (*alloc)(total);
    if (!out) { set_err(err, errlen, "borders_out too small: need %lld ints", (long long)total); return WGBSSEG_E_CAPACITY; }
    oi = 0;
    for (int64_t i = 0; i < n_chunks; i++) {
        if (hf[(size_t)i]) memcpy(out + borders_off[i], plain[(size_t)i].data(), plain[(size_t)i].size() * 4);
        else { memcpy(out + borders_off[i], ob.data() + ooff[oi], (size_t)(ooff[oi + 1] - ooff[oi]) * 4); oi++; }
    }
    c->last_valid = false;
    return WGBSSEG_OK;
}

int Batch::tile_plan(char* err, size_t errlen)
{
    BatchPlan& p = plan;
    const float pc = P.pseudo_count;
    const int n_stages = p.n_stages;
    CostArgs base;
    memset(&base, 0, sizeof(base));
    base.pc = pc; base.pc2 = pc + pc;
    base.xcd_group = 64;
    base.cmap = 3;                                             // the block -> start map: a byte per eight blocks (cost_lds)
    for (int k = 0; k < 3; k++) { ca[k] = base; ca[k].NS = p.NS[k]; ca[k].rows = p.rows[k]; }
    if (p.term_mode[0] == 2) {   // the k-scaled tables of the tile classes (same IEEE operations as on the device): built and uploaded when the pseudo count or a
                                 // class's exponent rows differ from what the context holds — a follow-up batch of the same call, the next call of a bench, reuse them
        const bool same = c->lookup_pc == pc && c->lookup_rows[0] == p.rows[0] && c->lookup_rows[1] == p.rows[1] && c->lookup_rows[2] == p.rows[2] && c->lookup.p;
        if (!same) {
            static const wg_log_tables host_tabs = WG_LOG_TABLES_INIT;
            c->h_lookup.resize((size_t)(p.rows[0] + p.rows[1] + p.rows[2]) * 80);
            wg_d2* dst = c->h_lookup.data();
            for (int rows : p.rows) {
                for (int x = 0; x < rows * 16; x++) dst[x] = wg_ks_iy_entry(&host_tabs, rows, x);
                for (int x = 0; x < rows * 64; x++) dst[rows * 16 + x] = wg_ks_ky_entry(&host_tabs, rows, x);
                dst += (size_t)rows * 80;
            }
            HIP_TRY(c->lookup.ensure(c->h_lookup.size() * sizeof(wg_d2)));
            HIP_TRY(hipMemcpyAsync(c->lookup.p, c->h_lookup.data(), c->h_lookup.size() * sizeof(wg_d2), hipMemcpyHostToDevice, c->sA));   // h_lookup lives in the context
            c->lookup_pc = pc;
            for (int k = 0; k < 3; k++) c->lookup_rows[k] = p.rows[k];
        }
        const wg_d2* tab = c->lookup.as<wg_d2>();
        for (int k = 0; k < 3; k++) { ca[k].tab = tab; tab += (size_t)p.rows[k] * 80; }
    }
    const size_t sb_bytes = (size_t)(n_stages + 1) * 4;
    HIP_TRY(c->plan_sb.ensure(sb_bytes));
    const void* src = p.sb;
    if (c->h_sb.ensure(sb_bytes)) { memcpy(c->h_sb.p, src, sb_bytes); src = c->h_sb.p; }      // (page-locked: the copy does not block)
    HIP_TRY(hipMemcpyAsync(c->plan_sb.p, src, sb_bytes, hipMemcpyHostToDevice, c->sA));
    HIP_TRY(c->plan_cbase.ensure((size_t)n_stages * nC * 8));
    HIP_TRY(c->plan_cum0.ensure((size_t)n_stages * nC * 4));
    HIP_TRY(c->plan_tbase.ensure((size_t)n_stages * (nC + 1) * 8 * 3));
    HIP_TRY(c->plan_cnt.ensure((size_t)n_stages * nC * 4 * 3));
    HIP_TRY(c->plan_pairs.ensure((size_t)n_stages * 8));
    HIP_TRY(c->plan_tiles.ensure((size_t)n_stages * 8 * 3));
    PlanArgs pa = {c->plan_sb.as<int32_t>(), p.TI, p.WA, WG_WIDE_TK, n_stages, p.WMED};
    uint32_t* cntA = c->plan_cnt.as<uint32_t>();
    uint32_t* cntB = cntA + (size_t)n_stages * nC;
    uint32_t* cntM = cntB + (size_t)n_stages * nC;
    int64_t* tbaseA = c->plan_tbase.as<int64_t>();
    int64_t* tbaseB = tbaseA + (size_t)n_stages * (nC + 1);
    int64_t* tbaseM = tbaseB + (size_t)n_stages * (nC + 1);
    if (!p.all_narrow) {
        hipLaunchKernelGGL(k_tile_count, dim3((unsigned)nC, (unsigned)n_stages), dim3(WG_BLOCK), 0, c->sA, job.v, pa, cntA, cntB, cntM);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_stage_plan, dim3((unsigned)n_stages), dim3(WG_PLAN_BLOCK), 0, c->sA, job.v, pa, (const uint32_t*)(p.all_narrow ? nullptr : cntA),
                       (const uint32_t*)(p.all_narrow ? nullptr : cntB), (const uint32_t*)(p.all_narrow ? nullptr : cntM),
                       c->plan_cbase.as<int64_t>(), c->plan_cum0.as<uint32_t>(), tbaseA, tbaseB, tbaseM, c->plan_pairs.as<int64_t>(), c->plan_tiles.as<int64_t>());
    HIP_TRY(hipGetLastError());
    if (!p.all_narrow) {
        // medium tiles and a pseudo count whose short division has not been tried on THEIR operand pairs yet (0 <= nmeth <= ntotal <=
        // 255 * 252: 2.1e9 pairs, ~2 ms, once per context and pseudo count, and only for a job that has windows > 60 at all)
        const bool check_div_m = c->divs_enabled && p.term_mode[2] == 2 && p.WMED > 0 && c->divs_m_pc != pc;
        int rc;
        if (check_div_m && (rc = queue_div_check(c, pc, WG_MEDIUM_WMAX, hst + 3, err, errlen)) != WGBSSEG_OK) return rc;
        HIP_TRY(hipMemcpyAsync(p.stage_pairs.data(), c->plan_pairs.p, (size_t)n_stages * 8, hipMemcpyDeviceToHost, c->sA));
        HIP_TRY(hipMemcpyAsync(p.stage_tiles.data(), c->plan_tiles.p, (size_t)n_stages * 24, hipMemcpyDeviceToHost, c->sA));
        HIP_TRY(hipStreamSynchronize(c->sA));
        if (check_div_m) {
            c->divs_m_ok = *reinterpret_cast<const unsigned int*>(&hst[3]) == 0u;
            c->divs_m_pc = pc;
            if (profiling()) fprintf(stderr, "[wgbsseg] short division core for pseudo count %g on the operand pairs of a MEDIUM tile: %s\n", (double)pc, c->divs_m_ok ? "verified on every pair" : "NOT exact, the full core stays");
        }
    }
    for (int k = 0; k < 3; k++) {
        tile0[k].assign((size_t)n_stages + 1, 0);
        for (int stg = 0; stg < n_stages; stg++) tile0[k][(size_t)stg + 1] = tile0[k][(size_t)stg] + p.stage_tiles[3 * (size_t)stg + k];
        if (tile0[k][(size_t)n_stages] > 0x7fffffffLL) { set_err(err, errlen, "too many scoring tiles in one call"); return WGBSSEG_E_ARG; }
    }
    for (int k = 0; k < 3; k++) HIP_TRY(c->tiles[k].ensure((size_t)std::max<int64_t>(1, tile0[k][(size_t)n_stages]) * sizeof(TileDesc)));
    for (int stg = 0; stg < n_stages; stg++) {
        hipLaunchKernelGGL(k_tile_emit, dim3((unsigned)nC), dim3(WG_BLOCK), 0, c->sA, job.v, pa, stg, tbaseA, tbaseB, tbaseM,
                           c->tiles[0].as<TileDesc>() + tile0[0][(size_t)stg], c->tiles[1].as<TileDesc>() + tile0[1][(size_t)stg],
                           c->tiles[2].as<TileDesc>() + tile0[2][(size_t)stg]);
        HIP_TRY(hipGetLastError());
    }
    if (p.gated) {
        HIP_TRY(c->stage_ctr.ensure((size_t)n_stages * 4));
        HIP_TRY(hipMemsetAsync(c->stage_ctr.p, 0, (size_t)n_stages * 4, c->sA));
    }
    HIP_TRY(hipEventRecord(c->ev[EV_PLAN], c->sA));
    if (p.gated) HIP_TRY(hipStreamWaitEvent(c->sA2, c->ev[EV_PLAN], 0));
    mark(4);
    return WGBSSEG_OK;
}

int Batch::stages(char* err, size_t errlen)
{
    const BatchPlan& p = plan;
    const JobView& v = job.v;
    const int n_stages = p.n_stages;
    const int64_t max_stage_pairs = std::max<int64_t>(1, *std::max_element(p.stage_pairs.begin(), p.stage_pairs.end()));
    for (int k = 0; k < p.nbuf; k++) HIP_TRY(c->cost[k].ensure((size_t)max_stage_pairs * 8));
    HIP_TRY(c->dpstate.ensure((size_t)nC * (size_t)p.state_stride * 8));
    HIP_TRY(c->tmp_borders.ensure((size_t)(job.sites_padded + nC) * 4));
    HIP_TRY(c->nb.ensure((size_t)nC * 4));
    // the batch's result on the device: the CSR offsets of the chunks' border lists, then the lists — one buffer, so that a small batch
    // (a follow-up batch of junction patches) comes home in ONE copy
    out_head = (size_t)round_up((int64_t)(nC + 1) * 8, 16);
    c->out_par ^= 1;                                             // (the other buffer may still be feeding k_copy_out of the previous batch)
    outb = &c->out_borders[c->out_par];
    HIP_TRY(outb->ensure(out_head + (size_t)(J + nC) * 4));
    for (auto* evs : {&c->ev_cost0, &c->ev_cost1, &c->ev_dp0, &c->ev_dp1, &c->ev_fork, &c->ev_join}) grow_events(*evs, n_stages);
    StageView sv;
    sv.cbase = c->plan_cbase.as<int64_t>(); sv.cum0 = c->plan_cum0.as<uint32_t>();
    sv.tbaseA = c->plan_tbase.as<int64_t>(); sv.tbaseB = sv.tbaseA + (size_t)n_stages * (nC + 1);
    sv.sb = c->plan_sb.as<int32_t>();
    DpArgs da = {p.ringN, {c->dp_wlean ? 0 : 1, 0, 0}};       // pad[0] = 1: the narrow batches of a wide job on the generic step
#ifdef WGBSSEG_DP_TIMING
    da.pad[1] = (int)env_int("WGBSSEG_DP_DEBUG", 0);      // timing builds only: see k_dp (results are WRONG in these modes)
#endif
    c->last_dp_chunks = nC; c->last_dp_stride = p.state_stride;
    // LDS of k_dp: two arranged batches (64 steps x 64 lanes, or 32 steps x 64 lanes x {A, B}) + M ring + fetched ring entries + flags + ring of windows / row offsets
    const size_t lds_dp = 2 * 4096 * 8 + 128 * 8 + 64 * 12 + 16 + 1024 * 6;
    double* const dps = c->dpstate.as<double>();
    if (st.wide_units) HIP_TRY(hipStreamWaitEvent(c->sA, c->ev[EV_SCAN_END], 0));      // wide tiles read the carries: scoring after the scan
    if (st.wide_units && p.gated) HIP_TRY(hipStreamWaitEvent(c->sA2, c->ev[EV_SCAN_END], 0));
    // Two scoring streams.  A scoring launch ends in a tail of partly filled workgroup slots (1280 on the chip), and a stage
    // with more than one tile class pays one per class: there the medium and wide tiles go to a second stream, beside the
    // narrow ones (they write disjoint rows of the cost buffer), forked off the first stream when the stage may begin
    // and joined before the stage's end is recorded (ev_fork / ev_join).  Measured, islands x32: scoring 29.49 -> 28.70 ms, x8 9.35 -> 9.14 ms.
    // The STAGES of a staged job alternate between the two streams only behind k_stage_gate (gated jobs, plan_stages): without the gate it
    // was measured and lost — the one-eighth share (8 stages) scored in 3.40 instead of 3.49 ms but its recurrences, which run beside the
    // next stage's scoring, fell behind (step 4.56 -> 4.79 ms); x200 / x512 gained 0.1-0.5 %.
    const bool divsA = c->divs_enabled && c->divs_ok && c->divs_pc == P.pseudo_count;
    const bool divsM = c->divs_enabled && c->divs_m_ok && c->divs_m_pc == P.pseudo_count;
    const int fast[3] = {p.term_mode[0] == 2 && divsA ? 3 : p.term_mode[0], p.term_mode[1], p.term_mode[2] == 2 && divsM ? 3 : p.term_mode[2]};
    ran_dp16.assign((size_t)n_stages, 0);
    for (int stg = 0; stg < n_stages; stg++) {
        const int64_t* const nt = &p.stage_tiles[3 * (size_t)stg];      // the stage's tiles per class
        hipStream_t const sP = p.gated && (stg & 1) ? c->sA2 : c->sA;
        sv.stage = stg;
        double* cbuf = c->cost[stg % p.nbuf].as<double>();
        const bool side = nt[0] > 0 && (nt[1] > 0 || nt[2] > 0);
        hipStream_t const sSide = side ? (p.gated && (stg & 1) ? c->sA : c->sA2) : sP;
        if (stg >= p.nbuf) HIP_TRY(hipStreamWaitEvent(sP, c->ev_dp1[stg - p.nbuf], 0));   // buffer free again
        if (p.gated) {
            const int64_t before = stg > 0 ? nt[-3] + nt[-2] + nt[-1] : 0;      // the previous stage's tiles of every class
            if (before > 0) {
                // the wait's bound: ten times what the stage before should take at 5e11 evaluations/s (its scored blocks are an upper bound for an all-narrow job), between
                // 5 ms and 2 s — a gate that opens early lets two stages interleave (the recurrence of the first starts late); one that waits for a launch which some other
                // context's work holds up (a context created on this device while the batch is in flight) gives up after a time in proportion to the job
                const double est_s = 10.0 * (double)p.stage_pairs[(size_t)stg - 1] * c->n_samples / 5e11;
                const long long max_ticks = (long long)(1e8 * std::min(2.0, std::max(0.005, est_s)));
                hipLaunchKernelGGL(k_stage_gate, dim3(1), dim3(64), 0, sP, (const uint32_t*)(c->stage_ctr.as<uint32_t>() + (stg - 1)),
                                   (uint32_t)std::max<int64_t>(1, before - c->stage_gate), max_ticks);
                HIP_TRY(hipGetLastError());
            }
            for (CostArgs& a : ca) a.finished = c->stage_ctr.as<uint32_t>() + stg;
        }
        HIP_TRY(hipEventRecord(c->ev_cost0[stg], sP));
        if (side) { HIP_TRY(hipEventRecord(c->ev_fork[stg], sP)); HIP_TRY(hipStreamWaitEvent(sSide, c->ev_fork[stg], 0)); }
        for (int k : {0, 2, 1})          // narrow tiles on the stage's stream; medium (the narrow tiles' arithmetic on rows of 269 entries), then wide ones beside them
            if (nt[k] > 0)
                HIP_TRY(launch_cost_class(k, fast[k], p.TI, v, sv, ca[k], c->tiles[k].as<TileDesc>() + tile0[k][(size_t)stg], nt[k], cbuf, p.lds[k], k == 0 ? sP : sSide));
        if (side) { HIP_TRY(hipEventRecord(c->ev_join[stg], sSide)); HIP_TRY(hipStreamWaitEvent(sP, c->ev_join[stg], 0)); }
        HIP_TRY(hipEventRecord(c->ev_cost1[stg], sP));
        HIP_TRY(hipStreamWaitEvent(c->sB, c->ev_cost1[stg], 0));
        HIP_TRY(hipEventRecord(c->ev_dp0[stg], c->sB));
        // worker waves per chunk, measured: 64-step batches (no window > 64): 7 (whole genome 3 -> 2.14 ms, 7 -> 1.77 ms,
        // 5 / 11 / 15 -> 2.8-3.1 ms); 32-step batches (islands): round 1 measured 3 workers 4.8 ms, 7 -> 5.8 ms; round 3 (the batch loops written per role
        // since round 2: 127 instead of 174 VGPRs) 3 -> 4.28 ms, 7 -> 3.52, with the lean step in the narrow batches 3.34 (11 workers: 5.0): 7 is the default now.  64-step batches again in round 3: 5 -> 1.83, 7 -> 1.66, 11 -> 1.65 ms.
        // 16-step batches at the footprint of one scoring workgroup when the recurrence of a stage runs beside the scoring of
        // the next one: whenever the call is staged.  Windows <= 60 (no wide tile in the job): the step with the batched bookkeeping, 6.75 instead
        // of 10 VALU instructions.
        // the LAST stage's recurrence has the chip to itself: the 64-step-batch kernel is twice as fast there
        const bool dp16 = p.dp_mode == 0 && n_stages > 1 && stg + 1 < n_stages;
        ran_dp16[(size_t)stg] = dp16;
        if (dp16)                                  hipLaunchKernelGGL((k_dp16<3>), dim3((unsigned)nC), dim3(64 * 4), (size_t)(2 * 16 * 64 * 8 + WG_DP_META_RING * 6), c->sB, v, sv, cbuf, dps, p.state_stride);
        else if (p.dp_mode == 0 && p.all_narrow)   hipLaunchKernelGGL((k_dp<7, 64, true>), dim3((unsigned)nC), dim3(64 * 8), lds_dp, c->sB, v, sv, cbuf, da, dps, p.state_stride);
        else if (p.dp_mode == 0)                   hipLaunchKernelGGL((k_dp<7, 64>), dim3((unsigned)nC), dim3(64 * 8), lds_dp, c->sB, v, sv, cbuf, da, dps, p.state_stride);
        else if (p.dp_mode == 1)                   hipLaunchKernelGGL((k_dp<7, 32>), dim3((unsigned)nC), dim3(64 * 8), lds_dp, c->sB, v, sv, cbuf, da, dps, p.state_stride);
        else                                       hipLaunchKernelGGL((k_dp<15, 32>), dim3((unsigned)nC), dim3(64 * 16), lds_dp, c->sB, v, sv, cbuf, da, dps, p.state_stride);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev_dp1[stg], c->sB));
    }
    return WGBSSEG_OK;
}

int Batch::deliver(char* err, size_t errlen)
{
    int64_t* const d_boff = outb->as<int64_t>();
    int32_t* const d_bord = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(outb->p) + out_head);
    HIP_TRY(hipEventRecord(c->ev[EV_TRACE0], c->sB));
    hipLaunchKernelGGL(k_trace, dim3((unsigned)nC), dim3(WG_BLOCK), 0, c->sB, job.v, c->tmp_borders.as<int32_t>(), c->nb.as<int32_t>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_border_offsets, dim3(1), dim3(WG_BLOCK), 0, c->sB, c->nb.as<int32_t>(), nC, d_boff);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_gather_borders, dim3((unsigned)nC), dim3(WG_BLOCK), 0, c->sB, job.v, c->tmp_borders.as<int32_t>(), c->nb.as<int32_t>(),
                       (const int64_t*)d_boff, d_bord);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(c->ev[EV_TRACE1], c->sB));
    // A chunk has at most len + 1 borders: a batch whose upper bound is small comes home in one copy (offsets + lists, through a page-locked
    // landing area); a large one sends the offsets first and then exactly the lists — or, when the caller can use them (EarlyOut), the offsets
    // with the edges of the leading items' lists, then the other items' lists, and the leading lists by k_copy_out behind the caller's back.
    const size_t small_bytes = out_head + (size_t)(J + nC) * 4;
    const bool small = small_bytes <= (512u << 10);
    const int64_t n_lead = (early && !small && early->n_lead > 0 && early->n_lead <= nC) ? early->n_lead : 0;
    // early delivery: the edges of the leading lists and, behind them, the lists of the other items (their size bounded by len + 1 each) ride
    // home with the offsets in one copy
    size_t rest_cap = 0;
    if (n_lead) for (int64_t i = n_lead; i < nC; i++) rest_cap += (size_t)job.h[(size_t)i].len + 1;
    const size_t edge_bytes = (size_t)n_lead * 2 * WG_EDGE * 4, rest_bytes = rest_cap * 4;
    if (n_lead) {
        HIP_TRY(c->edges.ensure(edge_bytes + rest_bytes + 16));
        hipLaunchKernelGGL(k_gather_edges, dim3((unsigned)nC), dim3(WG_BLOCK), 0, c->sB, (const int64_t*)d_boff, (const int32_t*)d_bord, (int)n_lead, c->edges.as<int32_t>(),
                           c->edges.as<int32_t>() + edge_bytes / 4);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->ev[EV_TRACE1], c->sB));
    }
    if (!c->h_out.ensure((small ? small_bytes : out_head) + edge_bytes + rest_bytes)) { set_err(err, errlen, "out of page-locked host memory"); return WGBSSEG_E_NOMEM; }
    HIP_TRY(hipMemcpyAsync(c->h_out.p, outb->p, small ? small_bytes : (size_t)(nC + 1) * 8, hipMemcpyDeviceToHost, c->sB));
    if (n_lead) HIP_TRY(hipMemcpyAsync(reinterpret_cast<char*>(c->h_out.p) + out_head, c->edges.p, edge_bytes + rest_bytes, hipMemcpyDeviceToHost, c->sB));
    if (small || n_lead) HIP_TRY(hipEventRecord(c->ev[EV_HOME], c->sB));
    mark(5);
    if (J >= (1 << 20)) {
        // a large batch: when its recurrence is done, ~0.2 ms of traceback and copies remain — just the time the host threads
        // of the junction stitching need to wake up (stitch.h)
        HIP_TRY(hipEventSynchronize(c->ev_dp1[plan.n_stages - 1]));
        wgstitch::Pool::get().heat();
    }
    HIP_TRY(hipStreamSynchronize(c->sB));
    memcpy(borders_off, c->h_out.p, (size_t)(nC + 1) * 8);
    const int64_t total_b = borders_off[nC];
    int32_t* borders_out = (*alloc)(total_b);
    if (!borders_out) { set_err(err, errlen, "borders_out too small: need %lld ints", (long long)total_b); return WGBSSEG_E_CAPACITY; }
    if (small) memcpy(borders_out, reinterpret_cast<const char*>(c->h_out.p) + out_head, (size_t)total_b * 4);
    else if (n_lead && early->dest_device_visible && (reinterpret_cast<uintptr_t>(borders_out) & 15) == 0) {
        const int64_t lead_b = borders_off[n_lead];              // the leading items' borders: [0, lead_b) of the lists
        // on the scan stream: idle by now, the lowest priority (the follow-up batch's kernels go first) and — as the one stream of its priority — a hardware
        // queue of its own (on a stream of the scoring streams' priority k_copy_out shared a queue with them: the follow-up batch's first kernel waited for it)
        HIP_TRY(hipStreamWaitEvent(c->sC, c->ev[EV_TRACE1], 0));
        hipLaunchKernelGGL(k_copy_out, dim3(512), dim3(WG_BLOCK), 0, c->sC, (const int32_t*)d_bord, borders_out, lead_b);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(c->evD, c->sC));
        c->out_pending = true;
        memcpy(borders_out + lead_b, reinterpret_cast<const char*>(c->h_out.p) + out_head + edge_bytes, (size_t)(total_b - lead_b) * 4);
        early->edges = reinterpret_cast<const int32_t*>(reinterpret_cast<const char*>(c->h_out.p) + out_head);
        early->pending = true;
    } else {
        HIP_TRY(hipMemcpyAsync(borders_out, d_bord, (size_t)total_b * 4, hipMemcpyDeviceToHost, c->sB));
        HIP_TRY(hipEventRecord(c->ev[EV_HOME], c->sB));
        HIP_TRY(hipStreamSynchronize(c->sB));
    }
    mark(6);
    // (events, not stream synchronisations: the scoring stream's work precedes the recurrence's by its events, and the scan stream ends in evS — a stream
    // synchronisation queues a marker of its own, which waited ~0.2 ms behind k_copy_out when the two streams shared a hardware queue)
    HIP_TRY(hipEventSynchronize(c->evS));
    // the scan's verdict (segmentor.cpp:186-189).  With the scan beside the scoring kernel an invalid file is found out at the end
    // of the batch; every kernel downstream of the counts is safe on such data (LDS indices out of a table's range read zeros,
    // the traceback bounds its steps) and what it produced is dropped here.
    if (hst[2].first_bad != ~0ULL) return report_bad_site(c, hst[2], err, errlen);
    return WGBSSEG_OK;
}

int Batch::timings(char* err, size_t errlen)
{
    const int n_stages = plan.n_stages;
    const int64_t total_pairs = (int64_t)st.total_pairs;
    if (marks) {       // device time line of the batch, ms after its first event (scoring / recurrence: first and last stage)
        auto at = [&](hipEvent_t e) { float x = 0; (void)hipEventElapsedTime(&x, c->ev[EV_BEGIN], e); return (double)x; };
        if (n_stages > 1) {
            fprintf(stderr, "[wgbsseg] %d stages%s, bounds", n_stages, plan.gated ? " (gated: alternating scoring streams)" : "");
            for (int q = 0; q <= n_stages; q++) fprintf(stderr, " %d", (int)plan.sb[q]);
            fprintf(stderr, "\n");
        }
        fprintf(stderr, "[wgbsseg] batch of %d chunks, %lld sites: windows done %.3f | stats copied %.3f | scan pass (its own stream) %.3f .. %.3f | plan + tiles done %.3f | "
                "scoring %.3f .. %.3f | recurrence %.3f .. %.3f | trace %.3f .. %.3f | borders on the host %.3f\n", nC, (long long)J,
                at(c->ev[EV_WINDOWS]), at(c->ev[EV_STATS]), at(c->ev[EV_VALIDATE0]), at(c->ev[EV_SCAN_END]), at(c->ev[EV_PLAN]), at(c->ev_cost0[0]), at(c->ev_cost1[n_stages - 1]),
                at(c->ev_dp0[0]), at(c->ev_dp1[n_stages - 1]), at(c->ev[EV_TRACE0]), at(c->ev[EV_TRACE1]), at(c->ev[EV_HOME]));
    }
    wgbsseg_timings& T = c->tim;
    if (!c->accumulate) memset(&T, 0, sizeof(T));
    float ms = 0;
    // the scan pass = k_scan for a job with wide tiles (it reads every chunk row of the batch, after k_validate has read the same bytes), k_validate otherwise
    if (st.wide_units) HIP_TRY(hipEventElapsedTime(&ms, c->ev[EV_SCAN0], c->ev[EV_SCAN1])); else HIP_TRY(hipEventElapsedTime(&ms, c->ev[EV_VALIDATE0], c->ev[EV_VALIDATE1]));
    T.scan_ms += ms;
    // algorithmic bytes of the pass: with wide units k_scan reads every chunk row of the batch; without, k_validate reads the
    // batch's not-yet-validated sites once
    const int64_t scan_bytes = 2 * (st.wide_units ? J : job.val_sites) * c->n_samples;
    if (scan_bytes > T.scan_main_bytes) { T.scan_main_bytes = scan_bytes; T.scan_main_ms = ms; }
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[EV_BEGIN], c->ev[EV_WINDOWS])); T.window_ms += ms;
    float cost_end = 0;      // scoring time = the union of the stages' intervals (neighbouring stages overlap on the two scoring streams)
    for (int stg = 0; stg < n_stages; stg++) {
        float t0 = 0, t1 = 0;
        HIP_TRY(hipEventElapsedTime(&t0, c->ev[EV_BEGIN], c->ev_cost0[stg])); HIP_TRY(hipEventElapsedTime(&t1, c->ev[EV_BEGIN], c->ev_cost1[stg]));
        if (t1 > std::max(t0, cost_end)) T.cost_ms += t1 - std::max(t0, cost_end);
        cost_end = std::max(cost_end, t1);
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_dp0[stg], c->ev_dp1[stg])); T.dp_ms += ms;
    }
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[EV_TRACE0], c->ev[EV_TRACE1])); T.trace_ms += ms;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[EV_BEGIN], c->ev[EV_HOME])); T.total_ms += ms;
    T.sites += J; T.pairs += total_pairs; T.evals += total_pairs * c->n_samples;
    T.scan_bytes += scan_bytes; T.max_window = std::max<int32_t>(T.max_window, plan.Wmax);
    T.n_stages = std::max<int32_t>(T.n_stages, n_stages); T.scan_launches += 1;
    if (plan.term_mode[0] == 2 && c->divs_enabled && c->divs_ok && c->divs_pc == P.pseudo_count) T.div_short = 1;
    c->last_sites = J; c->last_pairs = total_pairs; c->last_stages = n_stages; c->last_valid = true;
    c->last_chunks.resize((size_t)nC);
    for (int i = 0; i < nC; i++) c->last_chunks[(size_t)i] = {job.h[(size_t)i].site_off, job.h[(size_t)i].len, 0, 0};
    c->last_cost_rows_known = false;
    wgbsseg_ctx::LastPlan& lp = c->last_plan;
    lp.n_stages = n_stages; lp.gated = plan.gated; lp.nbuf = plan.nbuf; lp.last_pct = plan.last_pct; lp.dp_mode = plan.dp_mode;
    lp.all_narrow = plan.all_narrow; lp.live_ctx = plan.live_ctx; lp.n_chunks = nC;
    lp.sb.assign(plan.sb, plan.sb + n_stages + 1);
    lp.dp16 = ran_dp16;
    lp.stage_tiles = plan.stage_tiles;
    c->batch_open = false;
    if (marks) {
        hm[7] = wall_s();
        fprintf(stderr, "[wgbsseg]   host clock of the batch, us after entry: tables up %.0f | windows queued %.0f | statistics here %.0f | scoring's tiles queued %.0f | everything queued %.0f | results here %.0f | return %.0f\n",
                (hm[1] - hm[0]) * 1e6, (hm[2] - hm[0]) * 1e6, (hm[3] - hm[0]) * 1e6, (hm[4] - hm[0]) * 1e6, (hm[5] - hm[0]) * 1e6, (hm[6] - hm[0]) * 1e6, (hm[7] - hm[0]) * 1e6);
    }
    return WGBSSEG_OK;
}

}  // namespace

extern "C" {

int wgbsseg_segment_chunks(wgbsseg_ctx* c, const int64_t* chunk_start0, const int32_t* chunk_len, int64_t n_chunks,
                           const wgbsseg_params* P, int32_t* borders_out, int64_t borders_cap, int64_t* borders_off,
                           char* err, size_t errlen)
{
    if (!borders_out) { set_err(err, errlen, "NULL borders pointer"); return WGBSSEG_E_ARG; }
    BorderAlloc alloc = [&](int64_t total) -> int32_t* { return total <= borders_cap ? borders_out : nullptr; };
    return segment_chunks_impl(c, chunk_start0, chunk_len, n_chunks, P, alloc, borders_off, err, errlen);
}

int wgbsseg_segment_chunks_host(const uint8_t* betas, int64_t n_samples, int64_t sample_pitch_bytes, int64_t n_sites_total,
                                const uint32_t* loci, const int64_t* chunk_start0, const int32_t* chunk_len, int64_t n_chunks,
                                const wgbsseg_params* params, int device, int32_t* borders_out, int64_t borders_cap,
                                int64_t* borders_off, char* err, size_t errlen)
{
    if (!betas || n_samples < 1 || sample_pitch_bytes < 2 * n_sites_total) { set_err(err, errlen, "bad beta buffer"); return WGBSSEG_E_ARG; }
    wgbsseg_ctx* c = nullptr;
    int rc = wgbsseg_create(device, &c, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    std::vector<const uint8_t*> ptrs((size_t)n_samples);
    for (int64_t s = 0; s < n_samples; s++) ptrs[(size_t)s] = betas + s * sample_pitch_bytes;
    rc = wgbsseg_set_betas_host(c, ptrs.data(), n_samples, n_sites_total, err, errlen);
    if (rc == WGBSSEG_OK) rc = wgbsseg_set_loci_host(c, loci, n_sites_total, err, errlen);
    if (rc == WGBSSEG_OK) rc = wgbsseg_segment_chunks(c, chunk_start0, chunk_len, n_chunks, params, borders_out, borders_cap, borders_off, err, errlen);
    wgbsseg_destroy(c);
    return rc;
}

}  // extern "C"

namespace {
// One GPU batch on one context: 0-based resident-relative site ranges -> CSR of relative borders in page-locked memory
// that stays alive in the context (buffer `slot` of c->pinned) while ropes point into it.
int run_ctx_batch(wgbsseg_ctx* c, const std::vector<int64_t>& st0, const std::vector<int32_t>& ln, const wgbsseg_params* P, int64_t slot,
                  bool accumulate, const int32_t*& flat, std::vector<int64_t>& off, std::unique_ptr<int32_t[]>& owned, std::string& msg, EarlyOut* early = nullptr)
{
    off.resize(st0.size() + 1);
    int32_t* dst = nullptr;
    BorderAlloc alloc = [&](int64_t total) -> int32_t* {
        if (c->pinned.size() <= (size_t)slot) c->pinned.resize((size_t)slot + 1);
        PinnedBuf& pb = c->pinned[(size_t)slot];
        dst = pb.ensure((size_t)std::max<int64_t>(total, 1) * 4) ? reinterpret_cast<int32_t*>(pb.p) : nullptr;
        if (early) early->dest_device_visible = dst != nullptr;
        if (!dst) { owned.reset(new int32_t[(size_t)std::max<int64_t>(total, 1)]); dst = owned.get(); }   // pageable fallback
        return dst;
    };
    char ebuf[512] = {0};
    const bool acc_before = c->accumulate;
    c->accumulate = accumulate;
    const int rc = segment_chunks_impl(c, st0.data(), ln.data(), (int64_t)st0.size(), P, alloc, off.data(), ebuf, sizeof(ebuf), true, early);
    c->accumulate = acc_before;
    if (rc != WGBSSEG_OK) { msg = ebuf; return rc; }
    flat = dst;
    return WGBSSEG_OK;
}

int map_stitch_rc(int rc, const std::string& msg, char* err, size_t errlen)
{
    if (rc == 0) return WGBSSEG_OK;
    set_err(err, errlen, "%s", msg.c_str());
    return rc == wgstitch::E_CAPACITY ? WGBSSEG_E_CAPACITY : (rc < -1 ? rc : WGBSSEG_E_ARG);
}
}  // namespace

extern "C" {

int wgbsseg_segment_regions(wgbsseg_ctx* c, const int64_t* region_start, const int64_t* region_end, int64_t n_regions,
                            int64_t chunk_size, const wgbsseg_params* P, int32_t* borders_out, int64_t borders_cap,
                            int64_t* borders_off, int64_t* stats, char* err, size_t errlen)
{
    if (!c || !P) { set_err(err, errlen, "bad arguments to segment_regions"); return WGBSSEG_E_ARG; }
    int64_t n_batches = 0;
    wgstitch::BatchFn run_batch = [&](const std::vector<wgstitch::Sites>& todo, wgstitch::BatchResult& res, std::string& msg) -> int {
        std::vector<int64_t> st0(todo.size()), off;
        std::vector<int32_t> ln(todo.size());
        for (size_t i = 0; i < todo.size(); i++) {
            st0[i] = todo[i].first - 1;
            if (todo[i].second - todo[i].first > 0x7fffffff) { msg = "chunk too long"; return WGBSSEG_E_ARG; }
            ln[i] = (int32_t)(todo[i].second - todo[i].first);
        }
        const int32_t* flat = nullptr;
        std::unique_ptr<int32_t[]> owned;
        // the stitcher can start on the edges of the chunks' lists (res.n_lead = its number of chunks): ask for early delivery
        EarlyOut eo;
        eo.n_lead = c->early ? res.n_lead : 0;
        const int rc = run_ctx_batch(c, st0, ln, P, n_batches, n_batches > 0, flat, off, owned, msg, eo.n_lead > 0 ? &eo : nullptr);
        if (rc != WGBSSEG_OK) return rc;
        if (owned) res.owned.push_back(std::move(owned));
        res.set_csr(flat, off.data(), todo.size());
        if (eo.pending) {
            res.edges = eo.edges; res.edge_n = WG_EDGE;
            res.finish = [c](std::string& m) -> int {
                char e[256] = {0};
                const int r = wait_pending_output(c, e, sizeof e);
                if (r != WGBSSEG_OK) m = e;
                return r;
            };
        }
        n_batches++;
        return WGBSSEG_OK;
    };
    std::string msg;
    int rc = wgstitch::segment_regions(region_start, region_end, n_regions, chunk_size, run_batch, borders_out, borders_cap,
                                       borders_off, stats, msg, c->speculate);
    {   // (an error path of the stitcher may have left the first batch's lists on their way: nothing may write into the context's buffers after this call)
        char e[256] = {0};
        const int r2 = wait_pending_output(c, e, sizeof e);
        if (rc == 0 && r2 != WGBSSEG_OK) { rc = r2; msg = e; }
    }
    if (profiling()) {
        fprintf(stderr, "[wgbsseg] segment_regions: %lld batches; allocations since the last report: %lld calls, %.1f MB, %.1f ms; "
                "device ms: scan %.2f window %.2f cost %.2f dp %.2f trace %.2f, time line %.2f\n",
                (long long)n_batches, g_alloc_calls.exchange(0), (double)g_alloc_bytes.exchange(0) * 1e-6, (double)g_alloc_us.exchange(0) * 1e-3,
                c->tim.scan_ms, c->tim.window_ms, c->tim.cost_ms, c->tim.dp_ms, c->tim.trace_ms, c->tim.total_ms);
    }
    return map_stitch_rc(rc, msg, err, errlen);
}

int wgbsseg_set_site_base(wgbsseg_ctx* c, int64_t site_base)
{
    if (!c || site_base < 0) return WGBSSEG_E_ARG;
    c->site_base = site_base;
    return WGBSSEG_OK;
}

// The native chunk grid + stitching around a caller-supplied chunk engine (see include/wgbsseg.h).
int wgbsseg_stitch_regions(const int64_t* region_start, const int64_t* region_end, int64_t n_regions, int64_t chunk_size,
                           wgbsseg_batch_fn fn, void* user, int32_t speculate, int32_t* borders_out, int64_t borders_cap,
                           int64_t* borders_off, int64_t* stats, char* err, size_t errlen)
{
    if (!fn) { set_err(err, errlen, "stitch_regions: no chunk engine"); return WGBSSEG_E_ARG; }
    wgstitch::BatchFn run_batch = [&](const std::vector<wgstitch::Sites>& todo, wgstitch::BatchResult& res, std::string& msg) -> int {
        std::vector<int64_t> s(todo.size()), e(todo.size());
        for (size_t i = 0; i < todo.size(); i++) { s[i] = todo[i].first; e[i] = todo[i].second; }
        res.ptr.assign(todo.size(), nullptr);
        res.cnt.assign(todo.size(), 0);
        const int rc = fn(user, s.data(), e.data(), (int64_t)todo.size(), res.ptr.data(), res.cnt.data());
        if (rc != 0) { msg = "the chunk engine failed (code " + std::to_string(rc) + ")"; return rc < -1 ? rc : WGBSSEG_E_ARG; }
        for (size_t i = 0; i < todo.size(); i++)
            if (!res.ptr[i] || res.cnt[i] < 2 || res.ptr[i][0] != 0 || (int64_t)res.ptr[i][res.cnt[i] - 1] != e[i] - s[i]) {
                msg = "the chunk engine returned a malformed border list for sites [" + std::to_string(s[i]) + ", " + std::to_string(e[i]) + ")";
                return WGBSSEG_E_ARG;
            }
        return 0;
    };
    std::string msg;
    const int rc = wgstitch::segment_regions(region_start, region_end, n_regions, chunk_size, run_batch, borders_out, borders_cap,
                                             borders_off, stats, msg, speculate != 0);
    return map_stitch_rc(rc, msg, err, errlen);
}

// The items of the first batch of wgbsseg_segment_regions / wgbsseg_stitch_regions over these regions (see include/wgbsseg.h).
int wgbsseg_first_batch_items(const int64_t* region_start, const int64_t* region_end, int64_t n_regions, int64_t chunk_size,
                              int32_t speculate, int64_t* starts, int64_t* ends, int64_t cap, int64_t* n_items, int64_t* n_chunks,
                              char* err, size_t errlen)
{
    if (!region_start || !region_end || n_regions < 1 || chunk_size < 1 || !n_items) { set_err(err, errlen, "bad arguments to first_batch_items"); return WGBSSEG_E_ARG; }
    wgstitch::FirstBatch fb;
    std::string msg;
    const int rc = wgstitch::first_batch(region_start, region_end, n_regions, chunk_size, speculate != 0, fb, msg);
    if (rc != 0) return map_stitch_rc(rc, msg, err, errlen);
    *n_items = (int64_t)fb.items.size();
    if (n_chunks) *n_chunks = fb.n_chunks;
    if (starts && ends) {
        if (cap < (int64_t)fb.items.size()) { set_err(err, errlen, "first_batch_items: %lld items, room for %lld", (long long)fb.items.size(), (long long)cap); return WGBSSEG_E_CAPACITY; }
        for (size_t i = 0; i < fb.items.size(); i++) { starts[i] = fb.items[i].first; ends[i] = fb.items[i].second; }
    }
    return WGBSSEG_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------
// Share groups: one process, several GPUs (or several contexts on one GPU).  The chunk grid of a region list is cut
// into contiguous runs of chunks, one per share, balanced by the work the chunks hold (number of scored blocks,
// from the loci); a share keeps only its own window of the beta bytes.  Every batch of the stitching loop is routed
// item by item to the share that holds it and runs on one host thread per share; the reference's pairwise tree
// then runs ONCE, on the host, over all shares' results — the answer does not depend on the number of shares.
// The plan, the routing rule and the rule of the streaming upload are share_plan.h's (no HIP there).
// ------------------------------------------------------------------------------------------------------------
struct wgbsseg_group {
    // streaming upload (wgbsseg_group_load_host_async): one uploader per share; `ready` = sites of the share's window that are
    // resident for EVERY sample, counted from the window's first site
    struct Loader {
        std::thread th;
        std::atomic<int64_t> ready{0};
        std::atomic<int> finished{0};
        int rc = WGBSSEG_OK;
        std::string msg;
        void join() { if (th.joinable()) th.join(); }
        ~Loader() { join(); }
    };
    struct CtxDeleter { void operator()(wgbsseg_ctx* c) const { wgbsseg_destroy(c); } };
    struct Share {
        std::unique_ptr<wgbsseg_ctx, CtxDeleter> ctx;   // (declared first: goes last.  The uploader's thread holds this pointer raw; ~Loader joins it before the context goes)
        wgshare::Span span;
        bool loaded = false;
        std::unique_ptr<Loader> loader;
    };
    std::vector<Share> shares;
    std::vector<int64_t> rs, re;             // the planned regions (1-based half-open)
    int64_t chunk_size = 0, n_sites = 0, halo = 0;
    wgbsseg_params P = {};
    bool planned = false;
    bool streaming = false;
};

namespace {

// f(share, msg) -> code for every share of `which` (ascending); the first failure comes back as "share d: msg" with that share's code.
// pooled: the work-stealing pool, at most 64 threads (plan, load).  Else one thread per share, inline when there is only one, never
// capped (a batch): a share may block while it waits for its uploader, and a capped pool would line the shares behind it up.
template <class F>
int for_shares(const std::vector<int>& which, bool pooled, F f, std::string& msg)
{
    std::vector<int> rcs(which.size(), WGBSSEG_OK);
    std::vector<std::string> msgs(which.size());
    auto one = [&](int64_t i) { rcs[(size_t)i] = f(which[(size_t)i], msgs[(size_t)i]); };
    if (pooled) wgshare::parallel_for((int64_t)which.size(), 64, one);
    else if (which.size() == 1) one(0);
    else {
        std::vector<std::thread> th;
        for (size_t i = 0; i < which.size(); i++) th.emplace_back(one, (int64_t)i);
        for (auto& x : th) x.join();
    }
    for (size_t i = 0; i < which.size(); i++)
        if (rcs[i] != WGBSSEG_OK) { msg = "share " + std::to_string(which[i]) + ": " + msgs[i]; return rcs[i]; }
    return WGBSSEG_OK;
}

std::vector<int> resident_shares(const wgbsseg_group* g)
{
    std::vector<int> which;
    for (size_t d = 0; d < g->shares.size(); d++) if (g->shares[d].span.resident()) which.push_back((int)d);
    return which;
}

void scatter_spans(const std::vector<wgshare::Span>& spans, int64_t* own_lo, int64_t* own_hi, int64_t* win_lo, int64_t* win_hi, int64_t* share_chunks, int64_t* share_work)
{
    for (size_t d = 0; d < spans.size(); d++) {
        if (own_lo) own_lo[d] = spans[d].own_lo;
        if (own_hi) own_hi[d] = spans[d].own_hi;
        if (win_lo) win_lo[d] = spans[d].win_lo;
        if (win_hi) win_hi[d] = spans[d].win_hi;
        if (share_chunks) share_chunks[d] = spans[d].chunks;
        if (share_work) share_work[d] = spans[d].work;
    }
}

// What one call of wgbsseg_group_segment_region_range keeps per share
struct ShareCall {
    bool ran = false;              // the share's timings: reset on its first batch of the FIRST slice of the regions, summed after
    int64_t slot_next = 0;         // page-locked result buffers of the share used by this call so far
    std::vector<size_t> items;                          // the batch under way: its items for this share (indices into todo),
    std::vector<std::unique_ptr<int32_t[]>> owned;      // the fallback buffers they came back in
};

// One batch of the stitcher over a group: `todo`, where its lists go, and the call's state
struct GroupBatch {
    wgbsseg_group* g;
    const std::vector<wgstitch::Sites>& todo;
    wgstitch::BatchResult& res;
    std::vector<ShareCall>& calls;

    // every item to the share that holds it (wgshare::route); none does: a refusal, not a wrong answer
    int route(std::string& msg)
    {
        for (auto& c : calls) c.items.clear();
        for (size_t i = 0; i < todo.size(); i++) {
            const int64_t lo = todo[i].first - 1, hi = todo[i].second - 1;
            if (hi - lo > 0x7fffffff) { msg = "chunk too long"; return WGBSSEG_E_ARG; }
            const int pick = wgshare::route(g->shares, [](const wgbsseg_group::Share& s) -> const wgshare::Span& { return s.span; }, lo, hi);
            if (pick < 0) {
                msg = "sites [" + std::to_string(lo + 1) + ", " + std::to_string(hi + 1) + ") are not resident on any single share (halo " +
                      std::to_string(g->halo) + " sites): a junction patch outgrew it; rerun on one share";
                return WGBSSEG_E_STATE;
            }
            calls[(size_t)pick].items.push_back(i);
        }
        res.ptr.assign(todo.size(), nullptr);
        res.cnt.assign(todo.size(), 0);
        return WGBSSEG_OK;
    }

    // one launch sequence of share d over the items `it`; their lists into res
    int run_items(int d, const std::vector<size_t>& it, std::string& msg)
    {
        auto& sh = g->shares[(size_t)d];
        ShareCall& call = calls[(size_t)d];
        std::vector<int64_t> st0(it.size()), off;
        std::vector<int32_t> ln(it.size());
        for (size_t k = 0; k < it.size(); k++) {
            st0[k] = todo[it[k]].first - 1 - sh.span.win_lo;
            ln[k] = (int32_t)(todo[it[k]].second - todo[it[k]].first);
        }
        const int32_t* flat = nullptr;
        std::unique_ptr<int32_t[]> own;
        const int rc = run_ctx_batch(sh.ctx.get(), st0, ln, &g->P, call.slot_next++, call.ran, flat, off, own, msg);
        if (rc != WGBSSEG_OK) return rc;
        if (own) call.owned.push_back(std::move(own));
        call.ran = true;
        for (size_t k = 0; k < it.size(); k++) { res.ptr[it[k]] = flat + off[k]; res.cnt[it[k]] = off[k + 1] - off[k]; }
        return WGBSSEG_OK;
    }

    // the share's bytes are still arriving (front to back): segment what is resident while the rest is on its way —
    // items in order of their last site, a sub-batch whenever a fair part of the share has landed (wgshare::take_upto)
    int run_streaming(int d, const wgbsseg_group::Loader* L, std::string& msg)
    {
        const wgshare::Span& span = g->shares[(size_t)d].span;
        std::vector<size_t> order(calls[(size_t)d].items);
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return todo[a].second < todo[b].second; });
        std::vector<wgshare::Range> sites(order.size());
        for (size_t k = 0; k < order.size(); k++) sites[k] = {todo[order[k]].first - 1, todo[order[k]].second - 1};
        const int64_t min_take = wgshare::min_take(g->chunk_size, span);
        for (size_t pos = 0, end = 0; pos < order.size(); pos = end) {
            for (;;) {
                const bool fin = L->finished.load() != 0;
                const int64_t r = L->ready.load();
                if (fin && L->rc != WGBSSEG_OK) { msg = L->msg; return L->rc; }
                end = fin ? order.size() : wgshare::take_upto(sites, pos, span.win_lo + r, min_take);
                if (end > pos) break;
                std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
            const int rc = run_items(d, std::vector<size_t>(order.begin() + (ptrdiff_t)pos, order.begin() + (ptrdiff_t)end), msg);
            if (rc != WGBSSEG_OK) return rc;
        }
        return WGBSSEG_OK;
    }

    int run_share(int d, std::string& msg)
    {
        const auto* L = g->streaming ? g->shares[(size_t)d].loader.get() : nullptr;
        if (L && !L->finished.load()) return run_streaming(d, L, msg);
        if (L && L->rc != WGBSSEG_OK) { msg = L->msg; return L->rc; }
        return run_items(d, calls[(size_t)d].items, msg);
    }
};

}  // namespace

extern "C" {

int wgbsseg_group_create(const int32_t* devices, int32_t n_shares, wgbsseg_group** out, char* err, size_t errlen)
{
    if (!out) { set_err(err, errlen, "out is NULL"); return WGBSSEG_E_ARG; }
    *out = nullptr;
    if (!devices || n_shares < 1 || n_shares > 1024) { set_err(err, errlen, "group_create: need 1..1024 shares"); return WGBSSEG_E_ARG; }
    std::unique_ptr<wgbsseg_group> g(new (std::nothrow) wgbsseg_group());
    if (!g) { set_err(err, errlen, "out of host memory"); return WGBSSEG_E_NOMEM; }
    // Shares that double up on a device (dry runs of the N > 1 form on fewer GPUs): their scan streams run at the scoring streams' priority.  The lowest priority
    // is right where k_validate competes with the kernels of its OWN batch only; beside seven other shares' scoring kernels it would wait for the end of THEIR batches
    // (measured: a group of eight on one MI355X 34.4 -> 38.7-40.6 ms per step).
    bool doubled = false;
    for (int32_t a = 0; a < n_shares && !doubled; a++) for (int32_t b = a + 1; b < n_shares; b++) if (devices[a] == devices[b]) { doubled = true; break; }
    g->shares.resize((size_t)n_shares);
    for (int32_t d = 0; d < n_shares; d++) {
        wgbsseg_ctx* c = nullptr;
        const int rc = create_ctx(devices[d], !doubled, &c, err, errlen);
        if (rc != WGBSSEG_OK) return rc;                    // (the shares made so far go with g)
        g->shares[(size_t)d].ctx.reset(c);
    }
    *out = g.release();
    return WGBSSEG_OK;
}

void wgbsseg_group_destroy(wgbsseg_group* g)
{
    if (!g) return;
    for (auto& sh : g->shares) if (sh.loader) sh.loader->join();
    // releasing gigabytes of device buffers takes milliseconds per context: do the shares side by side
    wgshare::parallel_for((int64_t)g->shares.size(), 64, [&](int64_t d) { g->shares[(size_t)d].ctx.reset(); });
    delete g;
}

int32_t wgbsseg_group_size(const wgbsseg_group* g) { return g ? (int32_t)g->shares.size() : 0; }

int wgbsseg_plan_shares(const uint32_t* loci, int64_t n_sites, const int64_t* region_start, const int64_t* region_end, int64_t n_regions,
                        int64_t chunk_size, const wgbsseg_params* P, int32_t n_shares, int64_t halo, int64_t* own_lo, int64_t* own_hi,
                        int64_t* win_lo, int64_t* win_hi, int64_t* share_chunks, int64_t* share_work, char* err, size_t errlen)
{
    return wgbsseg_plan_shares_weighted(loci, n_sites, region_start, region_end, n_regions, chunk_size, P, n_shares, nullptr, halo, own_lo, own_hi,
                                        win_lo, win_hi, share_chunks, share_work, err, errlen);
}

int wgbsseg_plan_shares_weighted(const uint32_t* loci, int64_t n_sites, const int64_t* region_start, const int64_t* region_end, int64_t n_regions,
                                 int64_t chunk_size, const wgbsseg_params* P, int32_t n_shares, const double* weights, int64_t halo, int64_t* own_lo,
                                 int64_t* own_hi, int64_t* win_lo, int64_t* win_hi, int64_t* share_chunks, int64_t* share_work, char* err, size_t errlen)
{
    if (!own_lo || !own_hi) { set_err(err, errlen, "bad arguments to plan_shares"); return WGBSSEG_E_ARG; }
    std::vector<wgshare::Span> spans;
    std::string msg;
    const int rc = wgshare::plan_shares(loci, n_sites, region_start, region_end, n_regions, chunk_size, P, n_shares, weights, halo, spans, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    scatter_spans(spans, own_lo, own_hi, win_lo, win_hi, share_chunks, share_work);
    return WGBSSEG_OK;
}

int wgbsseg_group_plan(wgbsseg_group* g, const uint32_t* loci, int64_t n_sites, const int64_t* region_start, const int64_t* region_end,
                       int64_t n_regions, int64_t chunk_size, const wgbsseg_params* P, int64_t halo, int64_t* win_lo, int64_t* win_hi,
                       int64_t* share_chunks, int64_t* share_work, char* err, size_t errlen)
{
    if (!g) { set_err(err, errlen, "group is NULL"); return WGBSSEG_E_ARG; }
    g->planned = false;
    for (auto& s : g->shares) { s.span = wgshare::Span(); s.loaded = false; }
    std::vector<wgshare::Span> spans;
    std::string msg;
    halo = wgshare::resolve_halo(halo, chunk_size);
    int rc = wgshare::plan_shares(loci, n_sites, region_start, region_end, n_regions, chunk_size, P, (int32_t)g->shares.size(), nullptr, halo, spans, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    for (size_t d = 0; d < spans.size(); d++) g->shares[d].span = spans[d];
    g->rs.assign(region_start, region_start + n_regions);
    g->re.assign(region_end, region_end + n_regions);
    g->chunk_size = chunk_size; g->n_sites = n_sites; g->halo = halo; g->P = *P;
    // every share's window of the loci goes to its device now (4 bytes per site)
    rc = for_shares(resident_shares(g), true, [&](int d, std::string& m) {
        const wgshare::Span& s = g->shares[(size_t)d].span;
        wgbsseg_ctx* c = g->shares[(size_t)d].ctx.get();
        char eb[512] = {0};
        const int r = wgbsseg_set_loci_host(c, loci + s.win_lo, s.win_hi - s.win_lo, eb, sizeof(eb));
        c->site_base = s.win_lo;
        m = eb;
        return r;
    }, msg);
    if (rc != WGBSSEG_OK) { set_err(err, errlen, "%s", msg.c_str()); return rc; }
    scatter_spans(spans, nullptr, nullptr, win_lo, win_hi, share_chunks, share_work);
    g->planned = true;
    return WGBSSEG_OK;
}

int wgbsseg_group_load_host(wgbsseg_group* g, const uint8_t* const* samples, int64_t n_samples, int64_t n_sites, char* err, size_t errlen)
{
    if (!g || !g->planned) { set_err(err, errlen, "group_load_host: call wgbsseg_group_plan first"); return WGBSSEG_E_STATE; }
    if (!samples || n_samples < 1 || n_sites != g->n_sites) { set_err(err, errlen, "group_load_host: bad arguments (the plan is for %lld sites)", (long long)g->n_sites); return WGBSSEG_E_ARG; }
    std::string msg;
    const int rc = for_shares(resident_shares(g), true, [&](int d, std::string& m) {
        auto& sh = g->shares[(size_t)d];
        std::vector<const uint8_t*> ptrs((size_t)n_samples);
        for (int64_t s = 0; s < n_samples; s++) ptrs[(size_t)s] = samples[s] + 2 * sh.span.win_lo;
        char eb[512] = {0};
        const int r = wgbsseg_set_betas_host(sh.ctx.get(), ptrs.data(), n_samples, sh.span.win_hi - sh.span.win_lo, eb, sizeof(eb));
        m = eb;
        if (r == WGBSSEG_OK) sh.loaded = true;
        return r;
    }, msg);
    if (rc != WGBSSEG_OK) set_err(err, errlen, "%s", msg.c_str());
    return rc;
}

int wgbsseg_group_load_host_async(wgbsseg_group* g, const uint8_t* const* samples, int64_t n_samples, int64_t n_sites, char* err, size_t errlen)
{
    if (!g || !g->planned) { set_err(err, errlen, "group_load_host_async: call wgbsseg_group_plan first"); return WGBSSEG_E_STATE; }
    if (!samples || n_samples < 1 || n_sites != g->n_sites) { set_err(err, errlen, "group_load_host_async: bad arguments (the plan is for %lld sites)", (long long)g->n_sites); return WGBSSEG_E_ARG; }
    for (int64_t s = 0; s < n_samples; s++) if (!samples[s]) { set_err(err, errlen, "samples[%lld] is NULL", (long long)s); return WGBSSEG_E_ARG; }
    for (auto& sh : g->shares) sh.loader.reset();            // (joins the uploader of an earlier call)
    // the device rows exist (and the contexts point at them) before any byte moves; the uploaders then fill them front to back.
    // A failure here leaves no share half-way: nothing counts as loaded, no loader runs, the group is not streaming.
    auto fail = [&](hipError_t e, const char* what) {
        for (auto& sh : g->shares) { sh.loaded = false; sh.ctx->last_valid = false; }
        g->streaming = false;
        set_err(err, errlen, "group_load_host_async: %s: %s", what, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? WGBSSEG_E_NOMEM : WGBSSEG_E_HIP;
    };
    const std::vector<int> which = resident_shares(g);
    for (int d : which) {
        const auto& sh = g->shares[(size_t)d];
        hipError_t e = hipSetDevice(sh.ctx->device);
        if (e != hipSuccess) return fail(e, "hipSetDevice");
        e = own_rows(sh.ctx.get(), n_samples, sh.span.win_hi - sh.span.win_lo, 1);
        if (e != hipSuccess) return fail(e, "device rows of a share");
    }
    std::vector<const uint8_t*> base(samples, samples + n_samples);
    for (int d : which) {
        auto& sh = g->shares[(size_t)d];
        sh.loader.reset(new wgbsseg_group::Loader());
        auto* L = sh.loader.get();
        wgbsseg_ctx* c = sh.ctx.get();
        const int64_t lo = sh.span.win_lo, hi = sh.span.win_hi;
        L->th = std::thread([L, c, base, lo, hi, n_samples]() {
            std::vector<const uint8_t*> ptrs((size_t)n_samples);
            for (int64_t s = 0; s < n_samples; s++) ptrs[(size_t)s] = base[(size_t)s] + 2 * lo;
            L->rc = upload_rows_streaming(c, c->betas_own.as<uint8_t>(), c->pitch, ptrs.data(), n_samples, 2 * (hi - lo), L->ready, L->msg);
            L->ready.store(L->rc == WGBSSEG_OK ? hi - lo : L->ready.load());
            L->finished.store(1);
        });
        sh.loaded = true;
    }
    g->streaming = true;
    return WGBSSEG_OK;
}

int wgbsseg_group_load_wait(wgbsseg_group* g, char* err, size_t errlen)
{
    if (!g) { set_err(err, errlen, "group is NULL"); return WGBSSEG_E_ARG; }
    for (auto& sh : g->shares) if (sh.loader) sh.loader->join();
    g->streaming = false;
    for (size_t d = 0; d < g->shares.size(); d++) {
        const auto* L = g->shares[d].loader.get();
        if (L && L->rc != WGBSSEG_OK) { set_err(err, errlen, "share %d: %s", (int)d, L->msg.c_str()); return L->rc; }
    }
    return WGBSSEG_OK;
}

int wgbsseg_group_share_set_device(wgbsseg_group* g, int32_t share, const void* base, int64_t n_samples, int64_t pitch_bytes, char* err, size_t errlen)
{
    if (!g || !g->planned) { set_err(err, errlen, "group_share_set_device: call wgbsseg_group_plan first"); return WGBSSEG_E_STATE; }
    if (share < 0 || share >= (int32_t)g->shares.size()) { set_err(err, errlen, "no share %d", (int)share); return WGBSSEG_E_ARG; }
    auto& sh = g->shares[(size_t)share];
    if (!sh.span.resident()) return WGBSSEG_OK;             // a share without chunks needs no data
    const int rc = wgbsseg_set_betas_device(sh.ctx.get(), base, n_samples, pitch_bytes, sh.span.win_hi - sh.span.win_lo, err, errlen);
    if (rc == WGBSSEG_OK) sh.loaded = true;
    return rc;
}

int wgbsseg_group_segment_regions(wgbsseg_group* g, int32_t* borders_out, int64_t borders_cap, int64_t* borders_off, int64_t* stats,
                                  char* err, size_t errlen)
{
    if (!g || !g->planned) { set_err(err, errlen, "group_segment_regions: call wgbsseg_group_plan first"); return WGBSSEG_E_STATE; }
    return wgbsseg_group_segment_region_range(g, 0, (int64_t)g->rs.size(), borders_out, borders_cap, borders_off, stats, err, errlen);
}

int wgbsseg_group_segment_region_range(wgbsseg_group* g, int64_t first_region, int64_t end_region, int32_t* borders_out, int64_t borders_cap, int64_t* borders_off,
                                       int64_t* stats, char* err, size_t errlen)
{
    if (!g || !g->planned) { set_err(err, errlen, "group_segment_regions: call wgbsseg_group_plan first"); return WGBSSEG_E_STATE; }
    if (first_region < 0 || end_region <= first_region || end_region > (int64_t)g->rs.size()) { set_err(err, errlen, "group_segment_region_range: regions [%lld, %lld) of %lld planned", (long long)first_region, (long long)end_region, (long long)g->rs.size()); return WGBSSEG_E_ARG; }
    for (int d : resident_shares(g))
        if (!g->shares[(size_t)d].loaded) { set_err(err, errlen, "share %d has no beta data yet", d); return WGBSSEG_E_STATE; }
    std::vector<ShareCall> calls(g->shares.size());
    for (auto& c : calls) c.ran = first_region > 0;
    wgstitch::BatchFn run_batch = [&](const std::vector<wgstitch::Sites>& todo, wgstitch::BatchResult& res, std::string& msg) -> int {
        GroupBatch batch{g, todo, res, calls};
        int rc = batch.route(msg);
        if (rc != WGBSSEG_OK) return rc;
        std::vector<int> busy;
        for (size_t d = 0; d < calls.size(); d++) if (!calls[d].items.empty()) busy.push_back((int)d);
        rc = for_shares(busy, false, [&](int d, std::string& m) { return batch.run_share(d, m); }, msg);
        if (rc != WGBSSEG_OK) return rc;
        for (int d : busy) {                                // the fallback buffers of this batch go with its result
            for (auto& o : calls[(size_t)d].owned) res.owned.push_back(std::move(o));
            calls[(size_t)d].owned.clear();
        }
        return WGBSSEG_OK;
    };
    std::string msg;
    const int rc = wgstitch::segment_regions(g->rs.data() + first_region, g->re.data() + first_region, end_region - first_region, g->chunk_size, run_batch, borders_out,
                                             borders_cap, borders_off, stats, msg, g->shares[0].ctx->speculate);
    if (g->streaming && (end_region == (int64_t)g->rs.size() || rc != 0)) {      // every byte has been consumed by now; collect the uploaders
        char eb[512] = {0};
        const int lrc = wgbsseg_group_load_wait(g, eb, sizeof(eb));
        if (rc == 0 && lrc != WGBSSEG_OK) { set_err(err, errlen, "%s", eb); return lrc; }
    }
    return map_stitch_rc(rc, msg, err, errlen);
}

int wgbsseg_group_get_timings(const wgbsseg_group* g, int32_t share, wgbsseg_timings* out)
{
    if (!g || share < 0 || share >= (int32_t)g->shares.size()) return WGBSSEG_E_ARG;
    return wgbsseg_get_timings(g->shares[(size_t)share].ctx.get(), out);
}

int wgbsseg_scan_only(wgbsseg_ctx* c, const int64_t* chunk_start0, const int32_t* chunk_len, int64_t n_chunks, int repeat, int want_carry,
                      double* ms_per_launch, int64_t* bytes_per_launch, int64_t* carry_bytes_per_launch, char* err, size_t errlen)
{
    Job job;
    int rc = build_job(c, chunk_start0, chunk_len, n_chunks, job, false, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    rc = plan_validation(c, job, true, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    c->validated.clear();
    if (repeat < 1) repeat = 1;
    want_carry = want_carry ? 1 : 0;
    // want_carry 0: k_validate, the read-only pass of a job without wide tiles;
    // 1: k_scan — per-sample prefix sums of (meth, cov), a carry per 128 sites, the validation — as a job with wide tiles runs it
    auto one = [&]() { return want_carry ? launch_scan(c, job, c->sA, err, errlen) : launch_validate(c, job, c->sA, err, errlen); };
    rc = one();           // warm-up
    if (rc != WGBSSEG_OK) return rc;
    HIP_TRY(hipEventRecord(c->ev[0], c->sA));
    for (int r = 0; r < repeat; r++) { rc = one(); if (rc != WGBSSEG_OK) return rc; }
    HIP_TRY(hipEventRecord(c->ev[1], c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    if (ms_per_launch) *ms_per_launch = (double)ms / repeat;
    if (bytes_per_launch) *bytes_per_launch = 2 * (want_carry ? job.sites : job.val_sites) * c->n_samples;
    if (carry_bytes_per_launch) *carry_bytes_per_launch = want_carry ? (int64_t)sizeof(uint2) * job.carry_entries : 0;
    JobStatus st;
    HIP_TRY(hipMemcpyAsync(&st, c->status.p, sizeof(st), hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    if (st.first_bad != ~0ULL) return report_bad_site(c, st, err, errlen);
    return WGBSSEG_OK;
}

int wgbsseg_prefix_sums(wgbsseg_ctx* c, int64_t start0, int64_t len, uint32_t* out, char* err, size_t errlen)
{
    if (!out || len < 1 || len > 0x7fffffff) { set_err(err, errlen, "bad arguments to prefix_sums"); return WGBSSEG_E_ARG; }
    const int32_t l32 = (int32_t)len;
    Job job;
    int rc = build_job(c, &start0, &l32, 1, job, false, err, errlen);
    if (rc != WGBSSEG_OK) return rc;
    rc = launch_scan(c, job, c->sA, err, errlen);           // the carries are what k_prefix_materialise builds on
    if (rc != WGBSSEG_OK) return rc;
    const size_t bytes = (size_t)c->n_samples * (size_t)(len + 1) * 8;
    HIP_TRY(c->dbg_a.ensure(bytes));
    const int nG = job.h[0].nG;
    hipLaunchKernelGGL(k_prefix_materialise, dim3((unsigned)nG, (unsigned)c->n_samples), dim3(64), 0, c->sA, job.v, nG, c->dbg_a.as<uint32_t>(), l32);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->dbg_a.p, bytes, hipMemcpyDeviceToHost, c->sA));
    JobStatus st;
    HIP_TRY(hipMemcpyAsync(&st, c->status.p, sizeof(st), hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    if (st.first_bad != ~0ULL) return report_bad_site(c, st, err, errlen);
    c->last_valid = false;
    return WGBSSEG_OK;
}

}  // extern "C"

#include "row_engines.h"      // the calls on the resident rows (block_sums, marker_stats, sample_stats, the pair calls, beta2bed, the probe table, convert_regions)

// the text tables: loci and CpG columns, block and BED files parsed and written on the host (add_loci.h, table_io.h)
extern "C" {

int wgbsseg_add_loci(const uint32_t* loci, int64_t n_sites, const int64_t* chrom_cum, const char* const* chrom_names,
                     int32_t n_chroms, const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks,
                     const char* path, int32_t append, int32_t threads, char* err, size_t errlen)
{
    if (!loci || !chrom_cum || !chrom_names || n_chroms < 1 || n_sites < 1 || n_blocks < 0 || (n_blocks && (!start_cpg || !end_cpg))) {
        set_err(err, errlen, "add_loci: bad argument"); return WGBSSEG_E_ARG;
    }
    if (chrom_cum[n_chroms - 1] != n_sites) { set_err(err, errlen, "add_loci: chromosome sizes sum to %lld, loci has %lld sites", (long long)chrom_cum[n_chroms - 1], (long long)n_sites); return WGBSSEG_E_ARG; }
    wgadd::Genome g = {loci, n_sites, chrom_cum, chrom_names, n_chroms};
    std::string msg;
    int rc = 0;
    if (path) {
        // a regular file: format on all cores, then write the shards side by side at their offsets
        const int fd = open(path, O_WRONLY | O_CREAT | (append ? 0 : O_TRUNC), 0666);
        if (fd < 0) { set_err(err, errlen, "add_loci: cannot open %s", path); return WGBSSEG_E_ARG; }
        const off_t base = append ? lseek(fd, 0, SEEK_END) : 0;
        rc = base < 0 ? 3 : wgadd::add_loci_fd(g, start_cpg, end_cpg, n_blocks, fd, (int64_t)base, threads, msg);
        if (close(fd) != 0 && rc == 0) { set_err(err, errlen, "add_loci: write to %s failed", path); return WGBSSEG_E_ARG; }
        if (rc == 3 && msg.empty()) msg = "write failed";
    } else {
        rc = wgadd::add_loci(g, start_cpg, end_cpg, n_blocks, stdout, threads, msg);
    }
    if (rc) { set_err(err, errlen, "%s", msg.c_str()); return WGBSSEG_E_ARG; }
    return WGBSSEG_OK;
}

int wgbsseg_add_loci_borders(const uint32_t* loci, int64_t n_sites, const int64_t* chrom_cum, const char* const* chrom_names, int32_t n_chroms,
                             const int32_t* borders, const int64_t* borders_off, int64_t n_regions, int64_t min_cpg,
                             const char* path, int32_t append, int32_t threads, int64_t* n_written, int64_t* n_dropped, char* err, size_t errlen)
{
    if (n_written) *n_written = 0;
    if (n_dropped) *n_dropped = 0;
    if (!loci || !chrom_cum || !chrom_names || n_chroms < 1 || n_sites < 1 || n_regions < 0 || (n_regions && (!borders || !borders_off))) {
        set_err(err, errlen, "add_loci_borders: bad argument"); return WGBSSEG_E_ARG;
    }
    if (chrom_cum[n_chroms - 1] != n_sites) { set_err(err, errlen, "add_loci: chromosome sizes sum to %lld, loci has %lld sites", (long long)chrom_cum[n_chroms - 1], (long long)n_sites); return WGBSSEG_E_ARG; }
    // the rows must come out sorted by startCpG (segment.py:169 sorts them): region lists in ascending order, each ascending
    {
        int64_t last_r = -1;                                      // the last region that held a border, and that border
        int32_t last_b = 0;
        for (int64_t r = 0; r < n_regions; r++) {
            if (borders_off[r + 1] < borders_off[r] || (r == 0 && borders_off[0] < 0)) { set_err(err, errlen, "add_loci_borders: offsets not ascending"); return WGBSSEG_E_ARG; }
            if (borders_off[r + 1] == borders_off[r]) continue;
            if (last_r >= 0 && borders[borders_off[r]] < last_b) {
                set_err(err, errlen, "add_loci_borders: region %lld begins before region %lld ends (sort the blocks first)", (long long)r, (long long)last_r); return WGBSSEG_E_ARG;
            }
            // ... and ascending INSIDE the region: a descending pair would be counted as a dropped short block (b - a < min_cpg) where the
            // array form's check_row refuses "endCpG < startCpG" — refused here too, so that n_dropped counts short blocks only
            const int32_t* p = borders + borders_off[r];
            const int64_t nb = borders_off[r + 1] - borders_off[r];
            int32_t desc = 0;
            for (int64_t j = 0; j + 1 < nb; j++) desc |= (int32_t)(p[j + 1] < p[j]);
            if (desc) {
                int64_t j = 0;
                while (p[j + 1] >= p[j]) j++;
                set_err(err, errlen, "add_loci_borders: region %lld: border %lld (%d) follows %d (endCpG < startCpG; each region's borders must ascend)",
                        (long long)r, (long long)(j + 1), (int)p[j + 1], (int)p[j]);
                return WGBSSEG_E_ARG;
            }
            last_r = r; last_b = borders[borders_off[r + 1] - 1];
        }
    }
    wgadd::Genome g = {loci, n_sites, chrom_cum, chrom_names, n_chroms};
    wgadd::BorderRows rows{borders, borders_off, n_regions, min_cpg, {}};
    rows.index();
    const int64_t total = rows.total();
    std::string msg;
    int rc = 0;
    int64_t written = 0;
    if (path) {
        const int fd = open(path, O_WRONLY | O_CREAT | (append ? 0 : O_TRUNC), 0666);
        if (fd < 0) { set_err(err, errlen, "add_loci: cannot open %s", path); return WGBSSEG_E_ARG; }
        const off_t base = append ? lseek(fd, 0, SEEK_END) : 0;
        rc = base < 0 ? 3 : wgadd::add_loci_fd_rows(g, rows, total, fd, (int64_t)base, threads, msg, &written);
        if (close(fd) != 0 && rc == 0) { set_err(err, errlen, "add_loci: write to %s failed", path); return WGBSSEG_E_ARG; }
        if (rc == 3 && msg.empty()) msg = "write failed";
    } else {
        rc = wgadd::add_loci_rows(g, rows, total, stdout, threads, msg, &written);
    }
    if (n_written) *n_written = written;
    if (n_dropped) *n_dropped = rc ? 0 : total - written;
    if (rc) { set_err(err, errlen, "%s", msg.c_str()); return WGBSSEG_E_ARG; }
    return WGBSSEG_OK;
}

int wgbsseg_blocks_parse(const char* text, int64_t len, int64_t max_rows, int64_t cap, int64_t* line_off, int32_t* len3,
                         int64_t* start_cpg, int64_t* end_cpg, uint8_t* na, int64_t* n_rows,
                         int64_t* bp_start, int64_t* bp_end, int32_t* bp_ok, int32_t* first_fields)
{
    if (!n_rows) return WGBSSEG_E_ARG;
    *n_rows = 0;
    if (!text || len < 0 || cap < 0 || (cap && (!line_off || !len3 || !start_cpg || !end_cpg || !na))) return WGBSSEG_E_ARG;
    const int rc = wgtab::parse_blocks(text, len, max_rows, cap, line_off, len3, start_cpg, end_cpg, na, n_rows, bp_start, bp_end, bp_ok, first_fields);
    return rc == 0 ? WGBSSEG_OK : (rc == 1 ? 1 : WGBSSEG_E_ARG);
}

namespace {
int open_for_rows(const char* path, int append, int64_t* base, char* err, size_t errlen)
{
    const int fd = open(path, O_WRONLY | O_CREAT | (append ? 0 : O_TRUNC), 0666);
    if (fd < 0) { set_err(err, errlen, "cannot open %s", path); return -1; }
    const off_t b = append ? lseek(fd, 0, SEEK_END) : 0;
    if (b < 0) { close(fd); set_err(err, errlen, "cannot seek in %s", path); return -1; }
    *base = (int64_t)b;
    return fd;
}
}  // namespace

int wgbsseg_blocks_write_table(const char* path, int32_t append, const char* text, const int64_t* line_off, const int32_t* len3,
                               const int64_t* start_cpg, const int64_t* end_cpg, const uint8_t* na, int64_t n_rows,
                               const double* values, int64_t n_cols, int64_t stride, int32_t digits, int32_t threads, char* err, size_t errlen)
{
    if (n_rows < 0 || n_cols < 0 || stride < n_cols || (n_rows && (!text || !line_off || !len3 || !start_cpg || !end_cpg || !na || (n_cols && !values)))) {
        set_err(err, errlen, "write_table: bad argument"); return WGBSSEG_E_ARG;
    }
    int64_t base = -1;                                   // path NULL: standard output, whatever it is — shards in order
    const int fd = path ? open_for_rows(path, append, &base, err, errlen) : 1;
    if (fd < 0) return WGBSSEG_E_ARG;
    const wgtab::Rows R = {text, line_off, len3, start_cpg, end_cpg, na};
    std::string msg;
    const int rc = wgtab::write_table(fd, base, R, n_rows, values, n_cols, stride, digits, threads, msg);
    if (path && close(fd) != 0 && rc == 0) { set_err(err, errlen, "write to %s failed", path); return WGBSSEG_E_ARG; }
    if (rc) { set_err(err, errlen, "%s", msg.c_str()); return WGBSSEG_E_ARG; }
    return WGBSSEG_OK;
}

int wgbsseg_blocks_write_bedgraph(const char* path, const char* text, const int64_t* line_off, const int32_t* len3, int64_t n_rows,
                                  const void* rows, int32_t wide, int32_t threads, char* err, size_t errlen)
{
    if (!path || n_rows < 0 || (n_rows && (!text || !line_off || !len3 || !rows))) { set_err(err, errlen, "write_bedgraph: bad argument"); return WGBSSEG_E_ARG; }
    int64_t base = 0;
    const int fd = open_for_rows(path, 0, &base, err, errlen);
    if (fd < 0) return WGBSSEG_E_ARG;
    const wgtab::Rows R = {text, line_off, len3, nullptr, nullptr, nullptr};
    std::string msg;
    const int rc = wide ? wgtab::write_bedgraph<uint16_t>(fd, base, R, n_rows, static_cast<const uint16_t*>(rows), threads, msg)
                        : wgtab::write_bedgraph<uint8_t>(fd, base, R, n_rows, static_cast<const uint8_t*>(rows), threads, msg);
    if (close(fd) != 0 && rc == 0) { set_err(err, errlen, "write to %s failed", path); return WGBSSEG_E_ARG; }
    if (rc) { set_err(err, errlen, "%s", msg.c_str()); return WGBSSEG_E_ARG; }
    return WGBSSEG_OK;
}

int wgbsseg_bed_parse(const char* text, int64_t len, int64_t cap, const char* const* chrom_names, int32_t n_chroms, int64_t* line_off,
                      int32_t* len3, int32_t* row_len, int32_t* chrom, int64_t* start, int64_t* end, int64_t* n_rows, int32_t* width, int32_t* header)
{
    if (!n_rows || !width || !header) return WGBSSEG_E_ARG;
    *n_rows = 0; *width = 0; *header = 0;
    if (!text || len < 0 || cap < 0 || n_chroms < 0 || (n_chroms && !chrom_names) || (cap && (!line_off || !len3 || !row_len || !chrom || !start || !end))) return WGBSSEG_E_ARG;
    const int rc = wgtab::parse_bed(text, len, cap, chrom_names, n_chroms, line_off, len3, row_len, chrom, start, end, n_rows, width, header);
    return rc == 0 ? WGBSSEG_OK : (rc == 1 ? 1 : WGBSSEG_E_ARG);
}

int64_t wgbsseg_debug_canonical_float(const char* tokens, int64_t len, uint8_t* out, int64_t out_cap)
{
    if (!tokens || len < 0 || !out) return -1;
    int64_t n = 0;
    for (int64_t a = 0; a < len;) {
        const char* nl = static_cast<const char*>(memchr(tokens + a, '\n', (size_t)(len - a)));
        const int64_t b = nl ? (int64_t)(nl - tokens) : len;
        if (n >= out_cap) return -1;
        out[n++] = wgtab::canonical_float(tokens + a, (size_t)(b - a)) ? 1 : 0;
        a = b + 1;
    }
    return n;
}

int wgbsseg_bed_write_annotated(const char* path, const char* text, const int64_t* line_off, const int32_t* len3, const int32_t* row_len,
                                const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_rows, int32_t threads, char* err, size_t errlen)
{
    if (n_rows < 0 || (n_rows && (!text || !line_off || !len3 || !row_len || !start_cpg || !end_cpg))) { set_err(err, errlen, "bed_write_annotated: bad argument"); return WGBSSEG_E_ARG; }
    int64_t base = -1;                                   // path NULL: standard output
    const int fd = path ? open_for_rows(path, 0, &base, err, errlen) : 1;
    if (fd < 0) return WGBSSEG_E_ARG;
    std::string msg;
    const int rc = wgtab::write_annotated_bed(fd, base, text, line_off, len3, row_len, start_cpg, end_cpg, n_rows, threads, msg);
    if (path && close(fd) != 0 && rc == 0) { set_err(err, errlen, "write to %s failed", path); return WGBSSEG_E_ARG; }
    if (rc) { set_err(err, errlen, "%s", msg.c_str()); return WGBSSEG_E_ARG; }
    return WGBSSEG_OK;
}

int64_t wgbsseg_format_fixed(const double* v, int64_t n, int32_t digits, char* out, int64_t out_cap)
{
    if (n < 0 || (n && (!v || !out))) return -1;
    char* p = out;
    for (int64_t i = 0; i < n; i++) {
        if (out_cap - (p - out) < 420) return -1;
        p = wgtab::put_fixed(p, v[i], digits);
        *p++ = '\n';
    }
    return (int64_t)(p - out);
}

}  // extern "C"

#include "pat_engines.h"      // the engines that take pat text in chunks (pat2beta, homog, frag_len, test_bimodal, view) and their entry points

// what is left of the segmenter context's calls: its timings and the wgbsseg_debug_* views of its buffers and arithmetic
namespace {

// wgbsseg_debug_fetch("cost") of a staged job whose stages each kept a buffer to themselves (n_stages <= nbuf: stage s scored into cost[s % nbuf]).
// A stage holds the WHOLE rows of the start sites [sb[s], min(sb[s+1], len)) of every chunk — a block that ends beyond the bound lies with its start
// (k_stage_plan: a chunk's blocks in a stage are cum[s1] - cum[s0]; k_cost, k_dp: row k at cbase[s][chunk] + cum[k] - cum0[s][chunk]) — so chunk c's dense rows
// are, stage after stage, one run of cum[s1] - cum[s0] blocks at cbase[s][c].  What k_stage_plan left in plan_cum0 must be the chunk's cum at the bound.
int64_t fetch_staged_cost(wgbsseg_ctx* c, double* out)
{
    const std::vector<wgbsseg_ctx::LastChunk>& tab = c->last_chunks;
    const wgbsseg_ctx::LastPlan& lp = c->last_plan;
    const size_t nC = tab.size(), nS = (size_t)c->last_stages;
    if (lp.n_stages != c->last_stages || lp.sb.size() != nS + 1 || (size_t)lp.n_chunks != nC) return WGBSSEG_E_STATE;
    const size_t padded = (size_t)(tab.back().site_off + tab.back().len);
    if (nS * nC * 8 > c->plan_cbase.cap || nS * nC * 4 > c->plan_cum0.cap || nC * 8 > c->chunk_pairs.cap || padded * 4 > c->cum32.cap) return WGBSSEG_E_STATE;
    std::vector<int64_t> cbase(nS * nC), pairs(nC);
    std::vector<uint32_t> cum0(nS * nC), cum(padded);
    if (hipMemcpy(cbase.data(), c->plan_cbase.p, nS * nC * 8, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
    if (hipMemcpy(cum0.data(), c->plan_cum0.p, nS * nC * 4, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
    if (hipMemcpy(pairs.data(), c->chunk_pairs.p, nC * 8, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
    if (hipMemcpy(cum.data(), c->cum32.p, padded * 4, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
    int64_t at = 0;                                               // dense row 0 of the chunk
    for (size_t i = 0; i < nC; i++) {
        const int64_t len = tab[i].len;
        if (pairs[i] < 0 || at + pairs[i] > c->last_pairs) return WGBSSEG_E_STATE;
        for (size_t s = 0; s < nS && lp.sb[s] < len; s++) {       // (a chunk that ends before a stage begins has nothing in it)
            const int64_t s0 = lp.sb[s], s1 = std::min<int64_t>(lp.sb[s + 1], len);
            const int64_t r0 = cum[(size_t)(tab[i].site_off + s0)], r1 = s1 < len ? (int64_t)cum[(size_t)(tab[i].site_off + s1)] : pairs[i];
            const int64_t src = cbase[s * nC + i];
            if ((int64_t)cum0[s * nC + i] != r0 || r1 < r0 || r1 > pairs[i] || src < 0) return WGBSSEG_E_STATE;
            const DevBuf& buf = c->cost[s % (size_t)lp.nbuf];
            if ((size_t)(src + (r1 - r0)) * 8 > buf.cap) return WGBSSEG_E_STATE;
            if (r1 > r0 && hipMemcpy(out + at + r0, buf.as<double>() + src, (size_t)(r1 - r0) * 8, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
        }
        at += pairs[i];
    }
    return at == c->last_pairs ? c->last_pairs * 8 : (int64_t)WGBSSEG_E_STATE;
}

}  // namespace

extern "C" {

int wgbsseg_get_timings(const wgbsseg_ctx* c, wgbsseg_timings* out)
{
    if (!c || !out) return WGBSSEG_E_ARG;
    *out = c->tim;
    return WGBSSEG_OK;
}

int64_t wgbsseg_debug_fetch(wgbsseg_ctx* c, const char* what, void* out, int64_t cap_bytes)
{
    if (!c || !what || !out || !c->last_valid) return WGBSSEG_E_STATE;
    const std::vector<wgbsseg_ctx::LastChunk>& tab = c->last_chunks;
    const DevBuf* sites = nullptr;         // one of the job-site arrays: every chunk from entry site_off (a multiple of 8) on
    int64_t elem = 0;
    if (!strcmp(what, "window")) { sites = &c->W16; elem = 2; }
    else if (!strcmp(what, "cum")) { sites = &c->cum32; elem = 4; }
    else if (!strcmp(what, "back")) { sites = &c->back16; elem = 2; }
    if (sites) {
        // dense: chunk after chunk in the caller's order, the padding between the chunks' slices left out
        if (tab.empty()) return WGBSSEG_E_STATE;
        const int64_t bytes = c->last_sites * elem;
        const int64_t padded = (tab.back().site_off + tab.back().len) * elem;
        if (bytes > cap_bytes) return WGBSSEG_E_CAPACITY;
        if ((size_t)padded > sites->cap) return WGBSSEG_E_STATE;
        if (hipSetDevice(c->device) != hipSuccess) return WGBSSEG_E_HIP;
        if (tab.size() == 1) {
            if (hipMemcpy(out, sites->p, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
            return bytes;
        }
        std::vector<char> host((size_t)padded);
        if (hipMemcpy(host.data(), sites->p, (size_t)padded, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
        int64_t at = 0;
        for (const auto& ch : tab) {
            memcpy(static_cast<char*>(out) + at, host.data() + ch.site_off * elem, (size_t)(ch.len * elem));
            at += ch.len * elem;
        }
        return at == bytes ? bytes : (int64_t)WGBSSEG_E_STATE;
    }
    if (!strcmp(what, "dpstate")) {
        const int64_t bytes = c->last_dp_chunks * c->last_dp_stride * 8;
        if (bytes > cap_bytes) return WGBSSEG_E_CAPACITY;
        if (hipSetDevice(c->device) != hipSuccess) return WGBSSEG_E_HIP;
        if (hipMemcpy(out, c->dpstate.p, (size_t)bytes, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
        return bytes;
    }
    if (strcmp(what, "cost")) return WGBSSEG_E_ARG;
    // the scored blocks of a one-stage job: the rows of chunk 0, then of chunk 1, ...; where a chunk's rows lie in the cost buffer is the stage
    // plan's business (k_stage_plan: row 0 of plan_cbase), how many blocks it has the windows pass's (chunk_pairs)
    if (c->last_stages < 1 || tab.empty()) return WGBSSEG_E_STATE;
    if (c->last_stages > c->last_plan.nbuf) return WGBSSEG_E_STATE;        // a later stage has scored into an earlier one's buffer
    const int64_t bytes = c->last_pairs * 8;
    if (bytes > cap_bytes) return WGBSSEG_E_CAPACITY;
    if (hipSetDevice(c->device) != hipSuccess) return WGBSSEG_E_HIP;
    if (c->last_stages > 1) return fetch_staged_cost(c, static_cast<double*>(out));
    if (!c->last_cost_rows_known) {
        const size_t nC = tab.size();
        if (nC * 8 > c->plan_cbase.cap || nC * 8 > c->chunk_pairs.cap) return WGBSSEG_E_STATE;
        std::vector<int64_t> row0(nC), rows(nC);
        if (hipMemcpy(row0.data(), c->plan_cbase.p, nC * 8, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
        if (hipMemcpy(rows.data(), c->chunk_pairs.p, nC * 8, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
        for (size_t i = 0; i < nC; i++) { c->last_chunks[i].cost_row0 = row0[i]; c->last_chunks[i].cost_rows = rows[i]; }
        c->last_cost_rows_known = true;
    }
    int64_t at = 0;
    for (size_t i = 0; i < tab.size();) {                        // (chunks that follow each other in the buffer come home in one copy)
        size_t j = i;
        int64_t run = 0;
        while (j < tab.size() && tab[j].cost_row0 == tab[i].cost_row0 + run) { run += tab[j].cost_rows; j++; }
        if (tab[i].cost_row0 < 0 || run < 0 || at + run > c->last_pairs || (size_t)((tab[i].cost_row0 + run) * 8) > c->cost[0].cap) return WGBSSEG_E_STATE;
        if (run > 0 && hipMemcpy(static_cast<char*>(out) + at * 8, c->cost[0].as<double>() + tab[i].cost_row0, (size_t)run * 8, hipMemcpyDeviceToHost) != hipSuccess) return WGBSSEG_E_HIP;
        at += run;
        i = j;
    }
    return at == c->last_pairs ? bytes : (int64_t)WGBSSEG_E_STATE;
}

int64_t wgbsseg_debug_last_plan(const wgbsseg_ctx* c, int64_t* out, int64_t cap)
{
    if (!c || !out || !c->last_valid) return WGBSSEG_E_STATE;
    const wgbsseg_ctx::LastPlan& lp = c->last_plan;
    const int64_t nS = lp.n_stages, need = 8 + (nS + 1) + nS + 3 * nS;
    if (nS < 1 || (int64_t)lp.sb.size() != nS + 1 || (int64_t)lp.dp16.size() != nS || (int64_t)lp.stage_tiles.size() != 3 * nS) return WGBSSEG_E_STATE;
    if (cap < need) return WGBSSEG_E_CAPACITY;
    const int64_t head[8] = {nS, lp.gated, lp.nbuf, lp.last_pct, lp.dp_mode, lp.all_narrow, lp.live_ctx, lp.n_chunks};
    int64_t* o = std::copy(head, head + 8, out);
    o = std::copy(lp.sb.begin(), lp.sb.end(), o);
    o = std::copy(lp.dp16.begin(), lp.dp16.end(), o);
    std::copy(lp.stage_tiles.begin(), lp.stage_tiles.end(), o);
    return need;
}

int wgbsseg_debug_sample_terms(wgbsseg_ctx* c, const float* nmeth, const float* ntotal, int64_t count, float pseudo_count, float* out)
{
    char* err = nullptr; size_t errlen = 0;
    if (!c || !nmeth || !ntotal || !out || count < 1) return WGBSSEG_E_ARG;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->dbg_a.ensure((size_t)count * 4)); HIP_TRY(c->dbg_b.ensure((size_t)count * 4)); HIP_TRY(c->dbg_c.ensure((size_t)count * 4));
    HIP_TRY(hipMemcpyAsync(c->dbg_a.p, nmeth, (size_t)count * 4, hipMemcpyHostToDevice, c->sA));
    HIP_TRY(hipMemcpyAsync(c->dbg_b.p, ntotal, (size_t)count * 4, hipMemcpyHostToDevice, c->sA));
    const unsigned blocks = (unsigned)std::min<int64_t>((count + 255) / 256, 8192);
    const int fast = wg_term_mode(pseudo_count);                                         // the library's own dispatch rule
    const int rows = fast == 2 ? wg_lookup_rows(pseudo_count, 255.0 * 8000) : 0;       // block totals up to 255 * 8000 < 2^21: the longest the guard-free form serves
    if (rows > WG_KY_KMIN + 1) return WGBSSEG_E_ARG;
    hipLaunchKernelGGL(k_debug_terms, dim3(blocks), dim3(256), 0, c->sA, c->dbg_a.as<float>(), c->dbg_b.as<float>(), count, pseudo_count, c->dbg_c.as<float>(), fast, rows);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->dbg_c.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    return WGBSSEG_OK;
}

int wgbsseg_debug_div(wgbsseg_ctx* c, const float* a, const float* b, int64_t count, uint32_t* out_fast, uint32_t* out_ieee)
{
    char* err = nullptr; size_t errlen = 0;
    if (!c || !a || !b || !out_fast || !out_ieee || count < 1) return WGBSSEG_E_ARG;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->dbg_a.ensure((size_t)count * 8)); HIP_TRY(c->dbg_b.ensure((size_t)count * 8));
    float* da = c->dbg_a.as<float>(); float* db = da + count;
    uint32_t* o1 = c->dbg_b.as<uint32_t>(); uint32_t* o2 = o1 + count;
    HIP_TRY(hipMemcpyAsync(da, a, (size_t)count * 4, hipMemcpyHostToDevice, c->sA));
    HIP_TRY(hipMemcpyAsync(db, b, (size_t)count * 4, hipMemcpyHostToDevice, c->sA));
    const unsigned blocks = (unsigned)std::min<int64_t>((count + 255) / 256, 16384);
    hipLaunchKernelGGL(k_debug_div, dim3(blocks), dim3(256), 0, c->sA, da, db, count, o1, o2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_fast, o1, (size_t)count * 4, hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipMemcpyAsync(out_ieee, o2, (size_t)count * 4, hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    return WGBSSEG_OK;
}

int wgbsseg_debug_div_short(wgbsseg_ctx* c, const float* a, const float* b, int64_t count, uint32_t* out)
{
    char* err = nullptr; size_t errlen = 0;
    if (!c || !a || !b || !out || count < 1) return WGBSSEG_E_ARG;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->dbg_a.ensure((size_t)count * 8)); HIP_TRY(c->dbg_b.ensure((size_t)count * 4));
    float* da = c->dbg_a.as<float>(); float* db = da + count;
    HIP_TRY(hipMemcpyAsync(da, a, (size_t)count * 4, hipMemcpyHostToDevice, c->sA));
    HIP_TRY(hipMemcpyAsync(db, b, (size_t)count * 4, hipMemcpyHostToDevice, c->sA));
    const unsigned blocks = (unsigned)std::min<int64_t>((count + 255) / 256, 16384);
    hipLaunchKernelGGL(k_debug_div_short, dim3(blocks), dim3(256), 0, c->sA, da, db, count, c->dbg_b.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->dbg_b.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    return WGBSSEG_OK;
}

int wgbsseg_debug_check_div(wgbsseg_ctx* c, float pseudo_count, int32_t max_total, int64_t* mismatches)
{
    char* err = nullptr; size_t errlen = 0;
    if (!c || !mismatches || max_total < 0 || max_total > (1 << 21)) return WGBSSEG_E_ARG;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->divcheck.ensure(4));
    HIP_TRY(hipMemsetAsync(c->divcheck.p, 0, 4, c->sA));
    hipLaunchKernelGGL(k_check_div, dim3((unsigned)max_total + 1), dim3(WG_BLOCK), 0, c->sA, pseudo_count, pseudo_count + pseudo_count,
                       (int)max_total, c->divcheck.as<unsigned int>());
    HIP_TRY(hipGetLastError());
    unsigned int n = 0;
    HIP_TRY(hipMemcpyAsync(&n, c->divcheck.p, 4, hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    *mismatches = (int64_t)n;
    return WGBSSEG_OK;
}

int wgbsseg_debug_log2(wgbsseg_ctx* c, uint32_t first_bits, int64_t count, uint32_t* out_f, uint64_t* out_d, uint64_t* out_fast)
{
    char* err = nullptr; size_t errlen = 0;
    if (!c || count < 1 || (!out_f && !out_d && !out_fast)) return WGBSSEG_E_ARG;
    HIP_TRY(hipSetDevice(c->device));
    if (out_f) HIP_TRY(c->dbg_a.ensure((size_t)count * 4));
    if (out_d) HIP_TRY(c->dbg_b.ensure((size_t)count * 8));
    if (out_fast) HIP_TRY(c->dbg_c.ensure((size_t)count * 8));
    const unsigned blocks = (unsigned)std::min<int64_t>((count + 255) / 256, 16384);
    hipLaunchKernelGGL(k_debug_log2, dim3(blocks), dim3(256), 0, c->sA, first_bits, count, out_f ? c->dbg_a.as<uint32_t>() : nullptr,
                       out_d ? c->dbg_b.as<uint64_t>() : nullptr, out_fast ? c->dbg_c.as<uint64_t>() : nullptr);
    HIP_TRY(hipGetLastError());
    if (out_f) HIP_TRY(hipMemcpyAsync(out_f, c->dbg_a.p, (size_t)count * 4, hipMemcpyDeviceToHost, c->sA));
    if (out_d) HIP_TRY(hipMemcpyAsync(out_d, c->dbg_b.p, (size_t)count * 8, hipMemcpyDeviceToHost, c->sA));
    if (out_fast) HIP_TRY(hipMemcpyAsync(out_fast, c->dbg_c.p, (size_t)count * 8, hipMemcpyDeviceToHost, c->sA));
    HIP_TRY(hipStreamSynchronize(c->sA));
    return WGBSSEG_OK;
}

}  // extern "C"
