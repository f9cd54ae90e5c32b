/*
 * wgbsseg.h — C ABI of the MI355X-native `wgbstools segment` hot path (libwgbsseg.so, built by hipcc for gfx950).
 *
 * What it replaces.  The reference has no FFI on this path: its boundary is a PROCESS boundary.
 * src/python/segment.py:41-59 (`segment_process`) runs, per chunk of CpG sites,
 *     tabix rev.CpG.bed.gz chr:start-(end-1) | cut -f2 | segmentor b1.beta ... -s start-1 -n end-start
 *                                                         -max_cpg M -ps P -max_bp B
 * and parses the integers `segmentor` prints (src/segment_betas/main.cpp:89-112 ->
 * segmentor::dp_wrapper segmentor.cpp:193-214 -> read_beta_file :164-190, load_dists :36-48, dp :60-159,
 * traceback :50-58, print_borders :30-34).  One call of wgbsseg_segment_chunks() stands for a whole
 * Pool.starmap(segment_process, chunks) (segment.py:144-146): same inputs (beta bytes, loci, -s/-n per chunk,
 * -max_cpg/-ps/-max_bp), same outputs (per chunk the ascending border list including 0 and n, relative to the
 * chunk start), bit-exact.  INTEGRATION.md shows the ctypes stub a maintainer would put in segment.py.
 *
 * Conventions: plain pointers and sizes, no C++/torch types.  The caller owns every host buffer for the
 * duration of a call; the library never keeps a host pointer after returning.  Device buffers passed with the
 * *_device setters are borrowed (the caller keeps them alive until they are replaced or the context is
 * destroyed).  All calls on one context must come from one thread at a time; different contexts (one per GPU)
 * are independent.  Every entry point returns WGBSSEG_OK or a negative code and, when `err` is non-NULL,
 * a NUL-terminated message.  There is NO CPU fallback: without a gfx950 device wgbsseg_create() fails.
 */
#ifndef WGBSSEG_H
#define WGBSSEG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WGBSSEG_VERSION 380            /* 0.3.8: wgbsseg_fasta_*, wgbsseg_debug_fasta_walk (`wgbstools init_genome`: the CpG dictionary from FASTA text on the device).  0.3.7: wgbsseg_patview_set_sam, wgbsseg_patview_sam_info (`wgbstools bam2pat`: SAM reads called, paired and merged on the device).  0.3.6: wgbsseg_bedbeta_* (`wgbstools bed2beta`: BED methylation calls joined to the CpG dictionary on the device).  0.3.5.1: wgbsseg_debug_last_plan (test hook: the staging form of the last call); wgbsseg_debug_fetch("cost") serves staged calls with n_stages <= nbuf.  0.3.5:wgbsseg_patview_set_labels, wgbsseg_patview_label_rank, wgbsseg_patview_set_source, wgbsseg_patview_sample_info (`wgbstools mix_pat`: pat reads thinned and labelled on the device).  0.3.4: wgbsseg_patview_set_mask, wgbsseg_patview_mask_info, wgbsseg_patview_mask_ms (`wgbstools mask_pat`: sites hidden from pat reads on the device).  0.3.3: wgbsseg_patview_next_file, wgbsseg_merge_rows, wgbsseg_last_merge_rows_ms (`wgbstools merge`: pat and beta files of replicates pooled on the device).  0.3.2: wgbsseg_patview_* (`wgbstools view` / `cview`: pat reads filtered, sorted and collapsed on the device).  0.3.1: wgbsseg_bgzf_deflate, wgbsseg_bgzf_deflate_bound, wgbsseg_beta2bed_bgzf, wgbsseg_bgzf_deflate_ms, wgbsseg_bgzf_deflate_pass_ms (BGZF members deflated on the device).  0.3.0: wgbsseg_fraglen_* (`wgbstools frag_len`: the read-length histogram of a pat file).  0.2.9: wgbsseg_{patbeta,homog,bimodal}_feed_bgzf and _inflate_ms, wgbsseg_bgzf_inflate (BGZF members inflated on the device).  0.2.8: wgbsseg_site_counts, wgbsseg_site_table, wgbsseg_site_table_pass_ms, wgbsseg_site_table_limits (`wgbstools beta_to_450k`).  0.2.7: wgbsseg_beta2bed, wgbsseg_beta2bed_pass_ms, wgbsseg_beta2bed_limits, WGBSSEG_E_IO (`wgbstools beta2bed`).  0.2.6: wgbsseg_pair_ranges, wgbsseg_pair_hist, wgbsseg_pair_hist_limits (`wgbstools compare_betas`).  0.2.5: wgbsseg_sample_stats (`wgbstools beta_cov` / `beta_stats`).  0.2.4.1: wgbsseg_debug_bimodal_terms.  0.2.4: wgbsseg_bimodal_* (`wgbstools test_bimodal`).  0.2.3: wgbsseg_homog_* and wgbsseg_debug_homog_bins (`wgbstools homog`).  0.2.1: round 4 changed wgbsseg_scan_only's argument list and added wgbsseg_add_loci_borders without a bump; a binding compares wgbsseg_version() with the header it was written against */
#define WGBSSEG_MAX_CPG 65535          /* longest block, in sites (min(max_cpg, longest chunk)): see wgbsseg_segment_chunks */

#define WGBSSEG_OK              0
#define WGBSSEG_E_ARG          -1      /* bad argument (message says which) */
#define WGBSSEG_E_METH_GT_COV  -2      /* a requested site has #meth > #cov: segmentor.cpp:181-188 "invalid data" */
#define WGBSSEG_E_NOMEM        -3
#define WGBSSEG_E_HIP          -4      /* HIP runtime error / no usable device */
#define WGBSSEG_E_LOCI_ORDER   -5      /* (internal since round 4: chunks whose loci do not ascend take the plain path — the reference's loops as written, segmentor.cpp:114-117 — and are no error) */
#define WGBSSEG_E_CAPACITY     -6      /* borders_out too small */
#define WGBSSEG_E_STATE        -7      /* betas / loci not set */
#define WGBSSEG_E_IO           -8      /* a write to the caller's file descriptor failed; the message holds "errno N" */

typedef struct wgbsseg_ctx wgbsseg_ctx;

/* struct Params of segmentor.h:16-23, minus start/nr_sites (those are per chunk). */
typedef struct wgbsseg_params {
    float    pseudo_count;   /* -ps      (segment.py passes --pcount, default 15: segment.py:269)            */
    uint32_t max_cpg;        /* -max_cpg (segment.py passes min(--max_cpg, --max_bp/2): segment.py:65)       */
    uint32_t max_bp;         /* -max_bp  (must be >= 1: with 0 the reference reads uninitialised memory, segmentor.cpp:38,114) */
} wgbsseg_params;

/* HIP-event timings of the last wgbsseg_segment_chunks() call, milliseconds, and its work counters. */
typedef struct wgbsseg_timings {
    double scan_ms;          /* scan pass over the beta bytes: validation (+ carries when the job has wide tiles)  */
    double window_ms;        /* window extents from loci + CSR offsets                                 */
    double cost_ms;          /* block log-likelihood evaluation, summed over stages                    */
    double dp_ms;            /* changepoint recurrence, summed over stages                             */
    double trace_ms;         /* traceback + compaction                                                 */
    double total_ms;         /* first kernel start -> borders on the host (device time line)           */
    int64_t sites;           /* sum of chunk lengths                                                   */
    int64_t pairs;           /* sum over sites of the window F_k = candidate blocks scored             */
    int64_t evals;           /* pairs * n_samples = per-(block, sample) likelihood evaluations         */
    int64_t scan_bytes;      /* algorithmic bytes of the scan pass: 2 * n_samples * sites              */
    int32_t max_window;      /* largest F_k                                                            */
    int32_t n_stages;
    int32_t scan_launches;   /* kernel launches behind scan_ms (1 per batch)                           */
    int32_t div_short;       /* 1: the narrow scoring tiles of the call ran the verified 4-instruction division core */
    double  scan_main_ms;    /* duration of the largest scan launch of the call (the batch holding the chunks) */
    int64_t scan_main_bytes; /* its algorithmic bytes                                                  */
} wgbsseg_timings;

int wgbsseg_version(void);

/* Number of visible gfx950 devices (0 if none / no HIP runtime). */
int wgbsseg_device_count(void);

/* Create a context bound to HIP device `device` (its own streams and scratch memory). */
int wgbsseg_create(int device, wgbsseg_ctx** out, char* err, size_t errlen);
void wgbsseg_destroy(wgbsseg_ctx* ctx);

/*
 * Beta data: n_samples arrays of n_sites x 2 uint8 (#meth, #cov) — the `.beta` file format
 * (docs/beta_format.md:3-8; what read_beta_file segmentor.cpp:164-177 reads).  Sample order = argv order of the
 * reference (it fixes the order of the double accumulation, segmentor.cpp:120-136).
 * _host: copies every sample into one device allocation [n_samples][pitch] (pitch = 2*n_sites rounded up to 256 B);
 *        the pointers may be pageable memory (e.g. memory-mapped .beta files): above 32 MB the copy runs on a few host
 *        threads through page-locked staging pieces (WGBSSEG_UPLOAD_THREADS, default 4).  Blocking.
 * _device: borrows a device buffer with that layout; `base` and `pitch_bytes` must be multiples of 16.
 */
int wgbsseg_set_betas_host(wgbsseg_ctx* ctx, const uint8_t* const* samples, int64_t n_samples, int64_t n_sites,
                           char* err, size_t errlen);
/* .lbeta rows (uint16 pairs, docs/beta_format.md:41-44; utils_wgbs.py:311-319 reads them as np.uint16) for the block
 * reduction only: wgbsseg_block_sums accepts them, the segment calls refuse (the reference's segmentor reads uint8 only). */
int wgbsseg_set_lbetas_host(wgbsseg_ctx* ctx, const uint16_t* const* samples, int64_t n_samples, int64_t n_sites,
                            char* err, size_t errlen);
int wgbsseg_set_betas_device(wgbsseg_ctx* ctx, const void* base, int64_t n_samples, int64_t pitch_bytes,
                             int64_t n_sites, char* err, size_t errlen);

/* loci[i] = bp position of CpG i+1 (column 2 of CpG.bed.gz; what `tabix | cut -f2` feeds load_dists, segmentor.cpp:36-48).
 * _device: borrows a device array of n_sites uint32; `loci` must be a multiple of 4 bytes (any such address: no 16-byte
 *          alignment, no padding behind the last entry is needed; nothing outside [loci, loci + n_sites) is read), else
 *          WGBSSEG_E_ARG and the context keeps the loci it had. */
int wgbsseg_set_loci_host(wgbsseg_ctx* ctx, const uint32_t* loci, int64_t n_sites, char* err, size_t errlen);
int wgbsseg_set_loci_device(wgbsseg_ctx* ctx, const void* loci, int64_t n_sites, char* err, size_t errlen);

/*
 * Segment n_chunks chunks of the resident data.  Chunk c covers 0-based sites
 * [chunk_start0[c], chunk_start0[c] + chunk_len[c])  (== segmentor's -s / -n).
 * Output (CSR): chunk c's borders — ascending, relative to its start, first 0, last chunk_len[c], exactly the
 * integers the reference prints (segmentor.cpp:30-34) — are borders_out[borders_off[c] .. borders_off[c+1]).
 * borders_off has n_chunks+1 entries; borders_cap >= sum(chunk_len) + n_chunks always suffices.
 * Errors the reference also raises: #meth > #cov inside a requested chunk (message names sample and site).
 * Rejected up front (WGBSSEG_E_ARG), every one of them:
 *   - max_bp == 0: the reference then reads loci it never loaded (segmentor.cpp:38,114: undefined behaviour); unreachable from its CLI (segment.py:65-66);
 *   - max_cpg < 1;
 *   - pseudo_count < 0 or NaN: the reference computes SOMETHING there (p = (nmeth + pc) / (ntotal + 2 pc) may leave [0, 1]: log2 of a negative number is
 *     NaN, the double sum goes NaN and its comparisons decide the borders), but nothing a user can mean — `-ps` is a pseudo COUNT, segment.py:276 defaults
 *     it to 15 — and the exactness proofs of csrc/exact_log2.h cover pseudo counts >= 0 only.  A deliberate divergence: an error here, garbage there;
 *   - a chunk that is empty, longer than 2^30 sites or outside the resident sites; NULL pointers; n_chunks < 1;
 *   - blocks of more than WGBSSEG_MAX_CPG =
 * 65535 sites — i.e. min(max_cpg, longest chunk of the call) > 65535 (a window never exceeds its chunk, segmentor.cpp:110).
 * The reference sizes its ring to any max_cpg (segmentor.cpp:92-95); but with 255 * block sites >= 2^24 (65,794 sites) its own
 * float sums of the counts (segmentor.cpp:122-123) stop being exact, so nothing above that is reproducible from prefix sums
 * (SURVEY.md 8b grants this rejection), and windows are stored in 16 bits here, which moves the line from 65,793 to 65,535.
 * Up to round 2 the limit was 8000 (block totals < 2^21, which the guard-free form of the likelihood term rests on,
 * csrc/exact_log2.h); windows beyond that now score with the general guarded form (same bits, ~45 % more instructions).
 */
int wgbsseg_segment_chunks(wgbsseg_ctx* ctx, const int64_t* chunk_start0, const int32_t* chunk_len,
                           int64_t n_chunks, const wgbsseg_params* params,
                           int32_t* borders_out, int64_t borders_cap, int64_t* borders_off,
                           char* err, size_t errlen);

/*
 * Region-level form of the whole driver loop of segment.py:137-165 (SegmentByChunks.run + merge_df_list +
 * stitch_2_dfs), native: regions (1-based half-open CpG ranges [region_start, region_end), e.g. one per chromosome)
 * are cut into chunks `range(start, end, chunk_size) + [end]` (segment.py:124-135), every chunk and every
 * junction's first-attempt patch [b-p1, b+p2), p = min(50, operand span) (segment.py:209-216) go to the GPU as one
 * batch, then the junctions are stitched in the reference's pairwise order with its overlap / merge2 /
 * patch-doubling rules (segment.py:219-252); failed attempts are re-batched.  Output (CSR over regions): the
 * merged ABSOLUTE 1-based border list of each region as int32 (first region_start, last region_end); consecutive pairs
 * are the blocks (startCpG, endCpG) the reference writes (segment.py:154).  borders_cap >= sum(region lengths) +
 * n_regions always suffices.  stats (optional, 8 x int64): chunks, patch DPs run, GPU batches, patches planned up
 * front, host wall microseconds of the whole call / of the first batch / of the follow-up batches, total borders.
 * wgbsseg_get_timings() afterwards returns the sums over all batches of the call.
 */
int wgbsseg_segment_regions(wgbsseg_ctx* ctx, const int64_t* region_start, const int64_t* region_end, int64_t n_regions,
                            int64_t chunk_size, const wgbsseg_params* params,
                            int32_t* borders_out, int64_t borders_cap, int64_t* borders_off, int64_t* stats,
                            char* err, size_t errlen);

/*
 * The native chunk grid + junction stitching of wgbsseg_segment_regions around a CALLER-SUPPLIED chunk engine: `fn` is
 * called with batches of 1-based half-open site ranges (chunks and junction patches) and must set, for every range i,
 * out_ptr[i] / out_cnt[i] to the range's border list RELATIVE to its start (int32, ascending, first 0, last end-start —
 * what `segmentor` prints, segmentor.cpp:30-34); the lists must stay valid until wgbsseg_stitch_regions returns.
 * Non-zero return of `fn` aborts.  Used by the multi-process driver (rank 0 stitches what the ranks' GPUs produced) and
 * by the CPU test-suite (engine = the oracle).  speculate != 0: ask for a junction's possible second attempts together
 * with the first (fewer, larger batches).  No device is touched by this call itself.
 */
typedef int (*wgbsseg_batch_fn)(void* user, const int64_t* starts, const int64_t* ends, int64_t n,
                                const int32_t** out_ptr, int64_t* out_cnt);
int wgbsseg_stitch_regions(const int64_t* region_start, const int64_t* region_end, int64_t n_regions, int64_t chunk_size,
                           wgbsseg_batch_fn fn, void* user, int32_t speculate, int32_t* borders_out, int64_t borders_cap,
                           int64_t* borders_off, int64_t* stats, char* err, size_t errlen);

/*
 * The site ranges of the FIRST batch wgbsseg_segment_regions / wgbsseg_stitch_regions hand to their chunk engine for these
 * regions: the chunks of the grid (segment.py:124-135; *n_chunks of them, region by region), then the junction patches
 * planned up front (first attempts, and with speculate != 0 the three possible second attempts: segment.py:209-227), 1-based
 * half-open, no repeats.  A pure function of the arguments: the ranks of a multi-process run (one process per GPU) each
 * work out this list, compute the items whose first site they hold, and rank 0 hands the gathered lists to
 * wgbsseg_stitch_regions as its first batch.  starts / ends may be NULL to ask for *n_items only.
 */
int wgbsseg_first_batch_items(const int64_t* region_start, const int64_t* region_end, int64_t n_regions, int64_t chunk_size,
                              int32_t speculate, int64_t* starts, int64_t* ends, int64_t cap, int64_t* n_items, int64_t* n_chunks,
                              char* err, size_t errlen);

/* Absolute 0-based index of resident site 0 (default 0).  Coordinates of every call stay relative to the resident data;
 * the base only makes error messages ("invalid data ... site N") name absolute sites when a context holds a slice. */
int wgbsseg_set_site_base(wgbsseg_ctx* ctx, int64_t site_base);

/*
 * Share groups: the whole `Pool(threads)` of segment.py:144-146 spread over several GPUs from ONE process (the
 * reference's `-@`).  A group owns one context per share (devices[d]: a device may appear more than once).
 *   wgbsseg_group_plan     cuts the chunk grid of the regions (segment.py:124-135) into n_shares contiguous runs of chunks
 *                          balanced by WORK (the number of candidate blocks the chunks hold, counted from the host loci
 *                          with the window rule of segmentor.cpp:111-117, plus a per-site term), uploads every share's
 *                          window of the loci, and reports the 0-based site window [win_lo, win_hi) each share must hold:
 *                          its chunks +- `halo` sites (halo < 0: max(chunk_size, 4096)), lower edge on a multiple of 128.
 *   wgbsseg_group_load_host        every share uploads ITS window of the beta bytes (samples[s] = whole-genome array of
 *                          sample s, e.g. a memory-mapped .beta file), all shares side by side.
 *   wgbsseg_group_share_set_device lends share `share` a device buffer that holds exactly its window: row s at
 *                          base + s * pitch_bytes, n = win_hi - win_lo sites (base, pitch multiples of 16).
 *   wgbsseg_group_segment_regions  = wgbsseg_segment_regions over the planned regions: every batch of the stitching loop
 *                          (chunks + junction patches, then the follow-ups) is routed item by item to the share holding
 *                          it and runs on one host thread per share; the reference's pairwise tree (segment.py:157-165)
 *                          runs ONCE on the host over all results, so the borders are those of a one-GPU run whatever
 *                          the number of shares.  No device-to-device traffic.  A junction patch that outgrows the halo
 *                          (patch doubling past `halo` sites at a share boundary) fails with WGBSSEG_E_STATE.
 * share_chunks / share_work (optional, n_shares each): chunks and work units given to each share.
 */
typedef struct wgbsseg_group wgbsseg_group;
/* The planner on its own (host only, no device): own_lo/own_hi = 0-based sites [lo, hi) of the chunks given to each of the
 * n_shares shares (hi == lo: none), win_* = those +- halo.  The multi-process driver (one rank per GPU) cuts the genome
 * with it so that every rank computes the same shares.  (The planner, the routing of a batch and the rule of the streaming upload:
 * csrc/share_plan.h.) */
int wgbsseg_plan_shares(const uint32_t* loci, int64_t n_sites, const int64_t* region_start, const int64_t* region_end,
                        int64_t n_regions, int64_t chunk_size, const wgbsseg_params* params, int32_t n_shares, int64_t halo,
                        int64_t* own_lo, int64_t* own_hi, int64_t* win_lo, int64_t* win_hi, int64_t* share_chunks,
                        int64_t* share_work, char* err, size_t errlen);
/* The same with unequal targets: share d takes weights[d] / sum(weights) of the work (NULL: equal shares).  The multi-process driver
 * gives rank 0 — which also runs the stitching tree of every step — a smaller share than the other ranks. */
int wgbsseg_plan_shares_weighted(const uint32_t* loci, int64_t n_sites, const int64_t* region_start, const int64_t* region_end,
                                 int64_t n_regions, int64_t chunk_size, const wgbsseg_params* params, int32_t n_shares, const double* weights,
                                 int64_t halo, int64_t* own_lo, int64_t* own_hi, int64_t* win_lo, int64_t* win_hi,
                                 int64_t* share_chunks, int64_t* share_work, char* err, size_t errlen);
int wgbsseg_group_create(const int32_t* devices, int32_t n_shares, wgbsseg_group** out, char* err, size_t errlen);
void wgbsseg_group_destroy(wgbsseg_group* g);
int32_t wgbsseg_group_size(const wgbsseg_group* g);
int wgbsseg_group_plan(wgbsseg_group* g, const uint32_t* loci, int64_t n_sites, const int64_t* region_start,
                       const int64_t* region_end, int64_t n_regions, int64_t chunk_size, const wgbsseg_params* params,
                       int64_t halo, int64_t* win_lo, int64_t* win_hi, int64_t* share_chunks, int64_t* share_work,
                       char* err, size_t errlen);
int wgbsseg_group_load_host(wgbsseg_group* g, const uint8_t* const* samples, int64_t n_samples, int64_t n_sites,
                            char* err, size_t errlen);
/* The same upload without waiting for it: returns once the device rows exist; every share's bytes then arrive front to back
 * on background threads (site-major: piece k of every sample before piece k+1 of any), and wgbsseg_group_segment_regions
 * segments what is resident while the rest is on its way (the first batch of a share runs as a few sub-batches).  The
 * sample buffers must stay valid until wgbsseg_group_segment_regions or wgbsseg_group_load_wait has returned. */
int wgbsseg_group_load_host_async(wgbsseg_group* g, const uint8_t* const* samples, int64_t n_samples, int64_t n_sites,
                                  char* err, size_t errlen);
int wgbsseg_group_load_wait(wgbsseg_group* g, char* err, size_t errlen);
int wgbsseg_group_share_set_device(wgbsseg_group* g, int32_t share, const void* base, int64_t n_samples,
                                   int64_t pitch_bytes, char* err, size_t errlen);
int wgbsseg_group_segment_regions(wgbsseg_group* g, int32_t* borders_out, int64_t borders_cap, int64_t* borders_off,
                                  int64_t* stats, char* err, size_t errlen);

/*
 * The same over a SLICE of the planned regions, [first_region, end_region): regions never interact (segment.py:84-86,129-134), so a caller may
 * take them in slices and do something with one slice's blocks — write their BED rows — while the next slice is segmented and the beta bytes of
 * the later regions are still on their way up (wgbsseg_group_load_host_async streams site-major): `wgbstools segment` does when WGBSSEG_BED_SLICES asks
 * for more than one slice (opt-in; by default it takes all regions as one).  borders_off has
 * end_region - first_region + 1 entries.  The slices of one pass must be taken in ascending order; the uploaders are collected with the last one.
 */
int wgbsseg_group_segment_region_range(wgbsseg_group* g, int64_t first_region, int64_t end_region, int32_t* borders_out, int64_t borders_cap,
                                       int64_t* borders_off, int64_t* stats, char* err, size_t errlen);
int wgbsseg_group_get_timings(const wgbsseg_group* g, int32_t share, wgbsseg_timings* out);

/*
 * One-shot form (host buffers in, host borders out): creates a context on `device`, uploads, segments, destroys.
 * betas = [n_samples][sample_pitch_bytes] host bytes, each row holding n_sites_total x 2 uint8.
 */
int wgbsseg_segment_chunks_host(const uint8_t* betas, int64_t n_samples, int64_t sample_pitch_bytes,
                                int64_t n_sites_total, const uint32_t* loci,
                                const int64_t* chunk_start0, const int32_t* chunk_len, int64_t n_chunks,
                                const wgbsseg_params* params, int device,
                                int32_t* borders_out, int64_t borders_cap, int64_t* borders_off,
                                char* err, size_t errlen);

/*
 * Materialised per-sample prefix sums of one site range (the quantity the scan pass and the LDS tiles of the
 * scoring kernel are built from; also what a block-sum reduction such as beta_to_blocks.py:101-105 needs):
 * out[s][t][0] = sum_{u<t} meth_s[start0+u], out[s][t][1] = sum_{u<t} cov_s[start0+u], t = 0..len  (uint32).
 * out is a HOST buffer of n_samples*(len+1)*2 uint32.
 */
int wgbsseg_prefix_sums(wgbsseg_ctx* ctx, int64_t start0, int64_t len, uint32_t* out, char* err, size_t errlen);

/* The scan/validation pass alone over the given chunks (bandwidth benchmark): runs it `repeat` times and
 * returns the mean HIP-event time per launch in *ms_per_launch and the algorithmic bytes per launch (2 bytes per
 * sample and site read).  want_carry 0: the read-only pass of a job without wide scoring tiles (k_validate: what is left
 * of segmentor.cpp:164-190 there is the read and its `meth > cov` abort); 1: the prefix-sum pass proper (k_scan: per-sample
 * prefix sums of (meth, cov), one carry per 128 sites written, the same validation) as jobs with windows beyond 252 sites
 * run it; *carry_bytes_per_launch = the carries it writes (implementation traffic, not credited as algorithmic). */
int wgbsseg_scan_only(wgbsseg_ctx* ctx, const int64_t* chunk_start0, const int32_t* chunk_len, int64_t n_chunks,
                      int repeat, int want_carry, double* ms_per_launch, int64_t* bytes_per_launch,
                      int64_t* carry_bytes_per_launch, char* err, size_t errlen);

/*
 * Block sums: (#meth, #cov) of every block in every resident sample — the reduction of the reference's
 * beta_to_blocks / beta_to_table (beta_to_blocks.py:101-126 reduce_data: np.add.reduceat over the (meth, cov) rows,
 * or the per-row slice sums of its slow_method for tables that are not "nice"), the immediate consumer of the BED this
 * library produces.  Blocks are 0-based half-open site ranges [start0, end0) = [startCpG-1, endCpG-1); any order,
 * overlaps and empty blocks (sum 0: the reference's NA rows) are allowed.  out is a HOST buffer [n_samples][n_blocks]:
 *   mode 0  uint32[2]   the sums
 *   mode 1  uint8[2]    .bin  rows: cov > 255   -> meth = trunc(meth / cov * 255),   cov = 255   (utils_wgbs.py:277-290)
 *   mode 2  uint16[2]   .lbeta rows: the same with 65535
 *   mode 3  double      meth / cov, NaN where cov < min_cov                                    (utils_wgbs.py:270-274)
 */
int wgbsseg_block_sums(wgbsseg_ctx* ctx, const int64_t* start0, const int64_t* end0, int64_t n_blocks, int32_t mode,
                       uint32_t min_cov, void* out, char* err, size_t errlen);
/*
 * find_markers' per-block group statistics (find_markers.py:188-196, :318-335) over the ratio table the LAST wgbsseg_block_sums
 * call left on the device (it must have been a mode-3 call over n_blocks blocks): for a target set and a background set of
 * sample indexes (argument order of the setter; visited in the given order) out[b] = {n_tg, sum_tg, min_tg, max_tg, n_bg, sum_bg,
 * min_bg, max_bg} as doubles — the number of samples with a value (coverage >= min_cov), their sequential sum (nanmean =
 * sum / n), smallest and largest value (NaN when none).  out is a HOST buffer of n_blocks * 8 doubles.
 */
int wgbsseg_marker_stats(wgbsseg_ctx* ctx, const int32_t* tg, int32_t n_tg, const int32_t* bg, int32_t n_bg, int64_t n_blocks,
                         double* out, char* err, size_t errlen);
/* HIP-event time of the kernel of the last wgbsseg_block_sums call (ms) */
double wgbsseg_last_block_sums_ms(const wgbsseg_ctx* ctx);

/*
 * Per-sample statistics over the union of site ranges — what `wgbstools beta_cov` and `beta_stats` print per file
 * (beta_cov.py:62-69, beta_stats.py:28-56), every field an integer:
 *   n_sites               sum of (end0 - start0)
 *   meth_sum, cov_sum     sums of the two columns
 *   covered, covered_at   sites with cov > 0 / cov >= depth_at
 *   orphans               sites with cov == 0 and meth > 0 (numpy's meth / cov is inf there)
 *   max_cov               largest cov (0 over no sites)
 *   ratio_hi:ratio_lo     the EXACT sum of the doubles fl(fl(meth / cov) * 100.0) over the sites with cov > 0, a 128-bit
 *                         unsigned integer in units of 2^-62 (every such double is a multiple of 2^-62 for uint8 and uint16
 *                         counts): independent of summation order, so of launch geometry and of how the ranges are cut
 * Ranges are 0-based half-open [start0[i], end0[i]) inside [0, n_sites of the resident rows], ascending and disjoint
 * (start0[i] >= end0[i - 1]); empty ranges are allowed and n_ranges == 0 gives all-zero results.  Works on uint8 rows
 * (wgbsseg_set_betas_*) and uint16 rows (wgbsseg_set_lbetas_host).  A list that breaks the rules is refused with
 * WGBSSEG_E_ARG and a message naming the first offending range.  out is a HOST buffer of n_samples entries.  The kernels'
 * HIP-event time is what wgbsseg_last_block_sums_ms returns afterwards.
 */
typedef struct {
    uint64_t n_sites, meth_sum, cov_sum, covered, covered_at, orphans, ratio_lo, ratio_hi;
    uint32_t max_cov, reserved;
} wgbsseg_sample_stat;
int wgbsseg_sample_stats(wgbsseg_ctx* ctx, const int64_t* start0, const int64_t* end0, int64_t n_ranges, int32_t depth_at,
                         wgbsseg_sample_stat* out, char* err, size_t errlen);

/*
 * The sum of resident rows, site by site, with the saturation rule of `wgbstools merge` (merge.py:123-140 merge_betas,
 * utils_wgbs.py:277-290 trim_to_uint8).  samples: n_samples >= 1 indexes of resident rows (at most 65,536; a row may be named twice).
 * Per site M = the sum of meth and C = the sum of cov, exact integers; with max = 255 (65535 when lbeta_out is not 0): where C > max,
 * M = (int64)trunc(fl(fl((double)M / (double)C) * (double)max)) — two IEEE double operations, then the C cast — and C = max; then both
 * wrap to the width of the result (uint8, or uint16 when lbeta_out), as numpy's astype does: meth > cov in the input is not checked.
 * Works on uint8 rows (wgbsseg_set_betas_*, borrowed rows included: nothing beyond 2 * n_sites bytes of a row is read) and uint16 rows
 * (wgbsseg_set_lbetas_host).  out is a HOST buffer of n_sites x 2 uint8, or uint16 when lbeta_out.  Refused with WGBSSEG_E_ARG:
 * n_samples < 1 or > 65,536, an index that names no resident row, out == NULL.  wgbsseg_last_merge_rows_ms: the HIP-event time of the
 * kernel of the last call (ms).
 */
int wgbsseg_merge_rows(wgbsseg_ctx* ctx, const int32_t* samples, int32_t n_samples, int32_t lbeta_out, void* out, char* err, size_t errlen);
double wgbsseg_last_merge_rows_ms(const wgbsseg_ctx* ctx);

/*
 * Pairwise 2-D histograms of the resident samples — what `wgbstools compare_betas` draws per pair of files
 * (compare_betas.py:11-20: np.histogram2d of the two files' meth / cov over the sites both cover), in two passes because the
 * cell edges of a pair come from the pair's own values.  Pair i = samples (a[i], b[i]); a pair may repeat, a == b is allowed.
 * A site counts for a pair when min(cov_a, cov_b) >= min_cov; its values are fl(meth / cov), one IEEE double division
 * (meth > cov is not checked: a ratio above 1 is a value like any other).
 *
 * wgbsseg_pair_ranges   out[i] = the number of such sites and the smallest and largest ratio of either sample over them
 *                       (all four doubles 0 when n == 0): what np.histogram2d takes its range from.  Independent of launch
 *                       geometry: min and max run on the doubles' bit patterns as integers.
 * wgbsseg_pair_hist     edges = HOST doubles [n_pairs][2][bins + 1], axis 0 for sample b (x), axis 1 for sample a (y);
 *                       counts = HOST uint64 [n_pairs][bins][bins], counts[i][x_cell][y_cell].  The cell of a value v is
 *                       searchsorted(edges, v, 'right') - 1, v == the last edge falls in the last cell, v outside
 *                       [edges[0], edges[bins]] is dropped: np.histogram2d's rule, nothing approximated.  Integer counting:
 *                       a repeat gives the same bytes.
 * wgbsseg_pair_hist_limits   the largest `bins` wgbsseg_pair_hist takes (what one workgroup's LDS holds beside the edges) and
 *                       the run of sites one workgroup counts; either pointer may be NULL.
 *
 * Both work on uint8 rows (wgbsseg_set_betas_*) and uint16 rows (wgbsseg_set_lbetas_host); without rows: WGBSSEG_E_STATE.
 * Refused with WGBSSEG_E_ARG and a message naming the offender: NULL pointers, n_pairs < 1, min_cov < 1 (a site without
 * coverage has no ratio), a sample index outside the resident samples, bins < 1 or above the limit, edges that are not finite
 * or not strictly ascending.  The kernels' HIP-event time is what wgbsseg_last_block_sums_ms returns afterwards.
 */
typedef struct {
    uint64_t n;
    double a_min, a_max, b_min, b_max;
} wgbsseg_pair_range;
int wgbsseg_pair_ranges(wgbsseg_ctx* ctx, const int32_t* a, const int32_t* b, int64_t n_pairs, int32_t min_cov,
                        wgbsseg_pair_range* out, char* err, size_t errlen);
int wgbsseg_pair_hist(wgbsseg_ctx* ctx, const int32_t* a, const int32_t* b, int64_t n_pairs, int32_t min_cov, int32_t bins,
                      const double* edges, uint64_t* counts, char* err, size_t errlen);
void wgbsseg_pair_hist_limits(int32_t* max_bins, int64_t* run_sites);

/*
 * One resident sample as BED text, a line per site — what `wgbstools beta2bed` prints (beta2bed.py:11-19 over the lines of
 * view_beta.sh / view_lbeta.sh), formatted on the device and written to the file descriptor `fd`.  For the resident sites
 * [start0, end0) in ascending order:
 *
 *   base line    name \t loc-1 \t loc+1 \t meth \t cov \n      loc: the site's locus (wgbsseg_set_loci_*), name: of the last
 *                chromosome i with chrom_cum[i-1] <= site (chrom_cum = cumulative site counts, resident-relative)
 *   min_cov N    a site with cov < N counts as meth = cov = 0 (N = 1: nothing changes)
 *   keep_na 0    sites whose cov is 0 after that are dropped
 *   mean         the line is  name \t loc-1 \t loc+1 \t R \n,  R = printf "%.3g" of the double meth / cov, byte for byte what
 *                C prints, ties included (csrc/bed_fmt.h); -1 where cov is 0
 *   mult         NULL, or one count per site of [start0, end0): the line is written that many times, copies adjacent (0: not
 *                at all) — how `-L` repeats a site per overlapping BED row.  65535 is reserved and refused.
 *
 * The text is produced slab by slab (opts->slab_sites sites, 0 = the default of wgbsseg_beta2bed_limits): a length pass and
 * a scan, then a pass that formats into LDS and copies out with wide stores; slab k+1 is computed while slab k is written
 * to fd.  Nothing the size of the whole text is allocated.  opts->stage_bytes (0 = the default, the maximum) is the most a
 * workgroup's text may take to be staged in LDS; a workgroup with more writes straight to global memory (csrc/bed_plan.h).
 * Both parameters change speed only, never a byte.
 *
 * lines_written / bytes_written (either may be NULL): what went to fd.  Works on uint8 rows (wgbsseg_set_betas_*) and uint16
 * rows (wgbsseg_set_lbetas_host).  Without rows or loci (or loci of another length): WGBSSEG_E_STATE.  WGBSSEG_E_ARG with a
 * message naming the offender: a sample outside the resident samples, a range outside the resident sites, min_cov < 1, a
 * chrom_cum that descends or does not end at the resident site count, a name longer than 31 bytes, a multiplicity of 65535,
 * stage_bytes or slab_sites outside their limits.  WGBSSEG_E_CAPACITY: one slab's text would reach 4 GiB (multiplicities
 * only): pass a smaller slab_sites.  WGBSSEG_E_IO: write(2) failed; the message holds "errno N".  The kernels' HIP-event
 * time is what wgbsseg_last_block_sums_ms returns afterwards; wgbsseg_beta2bed_pass_ms splits it into the length + scan
 * passes and the emit pass (either pointer may be NULL).
 */
typedef struct {
    int32_t min_cov, mean, keep_na;
    int32_t stage_bytes;       /* 0 = default */
    int64_t slab_sites;        /* 0 = default */
} wgbsseg_bed_opts;
int wgbsseg_beta2bed(wgbsseg_ctx* ctx, int32_t sample, int64_t start0, int64_t end0, const uint16_t* mult,
                     const int64_t* chrom_cum, const char* const* chrom_names, int32_t n_chroms,
                     const wgbsseg_bed_opts* opts, int fd, int64_t* lines_written, int64_t* bytes_written,
                     char* err, size_t errlen);
void wgbsseg_beta2bed_pass_ms(const wgbsseg_ctx* ctx, double* length_ms, double* emit_ms);

/*
 * The same text as BGZF (the SAM specification, 4.1: gzip members of at most 64 KiB that `bgzip -d`, `gzip -d`, `tabix` and
 * wgbsseg_bgzf_inflate read): the arguments of wgbsseg_beta2bed and text_bytes.  Behind a slab's emit pass its text is cut into members
 * of 65280 bytes (the last one shorter), each deflated by one wavefront (csrc/deflate_core.h, csrc/deflate_kernels.h) and packed densely
 * on the device; only the compressed bytes come to the host and go to fd.  The end-of-file member (28 bytes) follows the last slab; a call
 * without a line writes it alone.  The text the file inflates to never depends on slab_sites or stage_bytes.  The compressed bytes do
 * depend on slab_sites, since members are cut per slab.  bytes_written: what went to fd; text_bytes (may be NULL): the text before
 * compression.  wgbsseg_bgzf_deflate_ms: the device time of the deflate and pack launches of the last call (-1 without a context);
 * wgbsseg_bgzf_deflate_pass_ms splits it (either pointer may be NULL).
 *
 * wgbsseg_bgzf_deflate: n bytes of host text -> BGZF bytes in out[0 .. *out_len), with the end-of-file member when eof is not 0.  out_cap
 * must be at least wgbsseg_bgzf_deflate_bound(n) (every member stored, plus the end-of-file member), else WGBSSEG_E_CAPACITY: the size is
 * known only when the device is done.  n = 0 gives no member, or the end-of-file member alone.  The same bytes as the encoder's host twin
 * (deflate_member_host) gives member by member.  The counterpart of wgbsseg_bgzf_inflate.
 */
int wgbsseg_beta2bed_bgzf(wgbsseg_ctx* ctx, int32_t sample, int64_t start0, int64_t end0, const uint16_t* mult,
                          const int64_t* chrom_cum, const char* const* chrom_names, int32_t n_chroms,
                          const wgbsseg_bed_opts* opts, int fd, int64_t* lines_written, int64_t* bytes_written, int64_t* text_bytes,
                          char* err, size_t errlen);
double wgbsseg_bgzf_deflate_ms(const wgbsseg_ctx* ctx);
void wgbsseg_bgzf_deflate_pass_ms(const wgbsseg_ctx* ctx, double* deflate_ms, double* pack_ms);
int64_t wgbsseg_bgzf_deflate_bound(int64_t n);
int wgbsseg_bgzf_deflate(int device, const void* text, int64_t n, void* out, int64_t out_cap, int64_t* out_len, int eof, char* err, size_t errlen);
/* the default and the largest slab_sites, the largest (= default) stage_bytes, the longest chromosome name; any pointer may be NULL */
void wgbsseg_beta2bed_limits(int64_t* default_slab, int64_t* max_slab, int32_t* max_stage_bytes, int32_t* max_name);

/*
 * The probe table: the counts of chosen sites in chosen resident samples — what `wgbstools beta_to_450k` prints for the sites
 * of the Illumina 450K / EPIC arrays.  Row r is the resident site site0[r] (0-based; any order, repeats allowed), column j the
 * resident sample samples[j] (repeats allowed).
 *
 * wgbsseg_site_counts: out[r][j] = {meth, cov} of that site in that sample, a HOST buffer of n_rows * n_cols * 2 uint16.
 *
 * wgbsseg_site_table: the table as CSV text, formatted on the device and written to the file descriptor `fd`; row r is
 *
 *     label_r , v , v , ... v \n        label_r = the bytes labels[label_off[r] .. label_off[r + 1]), copied as they are (the
 *                                       caller has quoted them where CSV asks for it); label_off has n_rows + 1 entries
 *     v                                 NA where cov < opts->min_cov; else printf "%.3f" of the double meth / cov, byte for byte
 *                                       what C prints, ties included (csrc/bed_fmt.h).  min_cov 0 lets cov = 0 through:
 *                                       0 / 0 is NA, meth / 0 with meth > 0 is inf.  meth > cov is a value like any other.
 *
 * The text is produced slab by slab (opts->slab_rows rows; 0 = the default: default_slab_rows of wgbsseg_site_table_limits,
 * fewer for wide rows, csrc/array_plan.h): one pass gathers the slab's counts into a compact table, a length pass and a scan
 * place every field, an emit pass formats into LDS and copies out with wide stores; slab k+1 is computed while slab k is
 * written to fd, through the buffers wgbsseg_beta2bed uses.  Nothing the size of the whole text is allocated.  slab_rows
 * changes speed only, never a byte.  lines_written / bytes_written (either may be NULL): what went to fd.
 *
 * Both work on uint8 rows (wgbsseg_set_betas_*) and uint16 rows (wgbsseg_set_lbetas_host); without rows: WGBSSEG_E_STATE.
 * WGBSSEG_E_ARG with a message naming the offender: NULL pointers, n_rows < 0, n_cols < 1 or above max_cols, a sample outside
 * the resident samples, a site outside the resident sites (the row is named), min_cov < 0, a label_off that descends, a label
 * longer than max_label bytes, slab_rows outside its limits.  n_rows = 0 writes nothing and returns 0.  WGBSSEG_E_IO:
 * write(2) failed; the message holds "errno N"; the context stays usable.  The kernels' HIP-event time is what
 * wgbsseg_last_block_sums_ms returns afterwards; wgbsseg_site_table_pass_ms splits it into the gather pass, the length + scan
 * passes and the emit pass (any pointer may be NULL).
 */
int wgbsseg_site_counts(wgbsseg_ctx* ctx, const int64_t* site0, int64_t n_rows, const int32_t* samples, int32_t n_cols,
                        uint16_t* out, char* err, size_t errlen);
typedef struct {
    int32_t min_cov;
    int32_t reserved;          /* 0 */
    int64_t slab_rows;         /* 0 = default */
} wgbsseg_site_table_opts;
int wgbsseg_site_table(wgbsseg_ctx* ctx, const int64_t* site0, int64_t n_rows, const int32_t* samples, int32_t n_cols,
                       const char* labels, const int64_t* label_off, const wgbsseg_site_table_opts* opts, int fd,
                       int64_t* lines_written, int64_t* bytes_written, char* err, size_t errlen);
void wgbsseg_site_table_pass_ms(const wgbsseg_ctx* ctx, double* gather_ms, double* length_ms, double* emit_ms);
/* the largest default and the largest slab_rows, the longest label, the most columns; any pointer may be NULL */
void wgbsseg_site_table_limits(int64_t* default_slab_rows, int64_t* max_slab_rows, int32_t* max_label, int32_t* max_cols);

/*
 * BED regions -> CpG index ranges: the join of `wgbstools convert -L` (convert.py:147-185 chr_thread, :133-145
 * slow_conversion + genomic_region.py:126-161), the step users run right before `segment -L` and `beta_to_blocks`; the
 * inverse direction is wgbsseg_add_loci below.  Against the loci resident in `ctx` (wgbsseg_set_loci_*; no betas
 * needed).  Region i lies on the chromosome whose CpGs are the 0-based sites [chrom_lo[i], chrom_hi[i]) (equal: unknown
 * chromosome -> NA) and whose length is chrom_bp[i] base pairs; (start[i], end[i]) is its bp interval.  slow[i] selects the
 * reference's rule set for the row's chromosome — it uses the as-of joins when the chromosome's regions do not overlap
 * (slow 0): startCpG = first CpG with locus >= start, endCpG = first CpG with locus >= end (+1 when exactly on `end`; last
 * CpG of the chromosome + 1 when none); and one GenomicRegion per row when they do (slow 1): CpGs with start <= locus <= end,
 * endCpG = last + 1 (last itself when its locus == end); end <= start, start < 1, end > chrom_bp: no answer.
 * Output: 1-based global indexes; (0, 0) where the reference writes NA (no CpG inside).
 */
int wgbsseg_convert_regions(wgbsseg_ctx* ctx, const int64_t* chrom_lo, const int64_t* chrom_hi, const int64_t* chrom_bp,
                            const int64_t* start, const int64_t* end, const uint8_t* slow, int64_t n,
                            int64_t* start_cpg, int64_t* end_cpg, char* err, size_t errlen);

/*
 * Blocks -> BED rows: the path's last step (segment.py:186-190 -> convert.py:242-248 add_bed_to_cpgs, which pipes the
 * blocks through the reference's `add_loci` binary: src/cpg2bed/add_loci.cpp:22-57, cpg_dict.cpp:40-131).  Host-side,
 * no device involved, no ctx needed.  For every block i (1-based half-open CpG interval) one row
 *     chrom \t loci[startCpG-1] \t loci[endCpG-2]+1 \t startCpG \t endCpG \n        (start+2 when endCpG == startCpG)
 * appended to `path` (NULL: stdout), in input order.  chrom_cum = cumulative CpG counts of the chromosomes in
 * CpG.chrome.size order (last = n_sites).  Validations and messages are the reference's (add_loci.cpp:38-49,
 * cpg_dict.cpp:130): on the first offending row the rows before it have been written and the call returns
 * WGBSSEG_E_ARG with err = "[wt add_loci] line N: endCpG < startCpG | startCpG < 1 | endCpG < 1 | Cross chromosomes"
 * or "[ cpg_dict ] Could not find chromosome for site: N".  threads <= 0: all host cores.
 */
int wgbsseg_add_loci(const uint32_t* loci, int64_t n_sites, const int64_t* chrom_cum, const char* const* chrom_names,
                     int32_t n_chroms, const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks,
                     const char* path, int32_t append, int32_t threads, char* err, size_t errlen);

/* The same rows straight from the merged border lists of a segmentation (round 4) — what wgbsseg_segment_regions /
 * wgbsseg_group_segment_regions leave: region r's ascending 1-based borders are borders[borders_off[r] .. borders_off[r+1]) — without
 * building (start, end) arrays first: a row is a pair of consecutive borders of a region (segment.py:154), written when
 * endCpG - startCpG >= min_cpg (the filter of segment.py:172-175 dump_result); *n_written / *n_dropped count both kinds (the numbers of
 * dump_result's stderr summary).  The regions must be given in ascending order (the rows come out sorted by startCpG as segment.py:169
 * sorts them; refused otherwise).  Same validations, messages, path / append / threads as wgbsseg_add_loci. */
int wgbsseg_add_loci_borders(const uint32_t* loci, int64_t n_sites, const int64_t* chrom_cum, const char* const* chrom_names,
                             int32_t n_chroms, const int32_t* borders, const int64_t* borders_off, int64_t n_regions,
                             int64_t min_cpg, const char* path, int32_t append, int32_t threads,
                             int64_t* n_written, int64_t* n_dropped, char* err, size_t errlen);

/*
 * The text either side of the block reduction (`wgbstools beta_to_table`: beta_to_table.py:59-127, `beta_to_blocks --bedGraph`:
 * beta_to_blocks.py:112-126; the reference reads the blocks table with pandas.read_csv and prints with DataFrame.to_csv).  Host
 * side, no device, no ctx.
 *
 * wgbsseg_blocks_parse: the bytes of a blocks table (tab-separated chr, start, end, startCpG, endCpG [, more]; '#' comments,
 * blank lines and a header line are skipped) -> per row the offset of its first byte (line_off), the length of its
 * "chr \t start \t end" text (len3), the two CpG columns and na = 1 where one of them is missing (NA, empty, ...).  A FAST PATH:
 * returns WGBSSEG_OK with *n_rows rows (at most max_rows when max_rows >= 0), or 1 when the text is not a plain table — a row
 * with fewer than five fields, a CpG field that is neither digits nor a missing-value spelling, carriage returns, non-ASCII
 * bytes, no row at all — and the caller then parses it line by line (the Python host owns those cases and their messages).
 * WGBSSEG_E_ARG: more than `cap` rows (cap = number of '\n' + 1 always suffices).
 * Optional outputs (NULL: not wanted): bp_start / bp_end = the rows' second and third fields as integers, valid when *bp_ok = 1
 * (every row's are plain digits) — `find_markers` filters blocks by their length in base pairs; *first_fields = fields (at most
 * 7) of the first line that is neither a comment nor blank: a table has the two annotation columns when that line has 7.
 *
 * wgbsseg_blocks_write_table: one output row per parsed row r: its "chr \t start \t end" bytes, startCpG, endCpG (NA where
 * na[r]), then values[r * stride + c], c < n_cols, as printf("%.<digits>f") (NaN: NA), tab-separated, '\n'; appended to `path`
 * (append 0: the file is truncated first; path NULL: written to the process's standard output).  The digits are those of the exact binary value rounded half to even, as glibc's
 * printf and Python's % operator print them.  wgbsseg_blocks_write_bedgraph: chr, start, end, meth / cov as %.2f (-1 for
 * 0 / 0), cov — from rows of uint8 (wide 0) or uint16 (wide 1) pairs.  threads <= 0: all host cores (at most 32).
 * wgbsseg_format_fixed: the number formatter alone, one value per line into `out` (test hook); returns the bytes written, -1
 * when out_cap is too small.
 */
int wgbsseg_blocks_parse(const char* text, int64_t len, int64_t max_rows, int64_t cap, int64_t* line_off, int32_t* len3,
                         int64_t* start_cpg, int64_t* end_cpg, uint8_t* na, int64_t* n_rows,
                         int64_t* bp_start, int64_t* bp_end, int32_t* bp_ok, int32_t* first_fields);
int wgbsseg_blocks_write_table(const char* path, int32_t append, const char* text, const int64_t* line_off, const int32_t* len3,
                               const int64_t* start_cpg, const int64_t* end_cpg, const uint8_t* na, int64_t n_rows,
                               const double* values, int64_t n_cols, int64_t stride, int32_t digits, int32_t threads, char* err, size_t errlen);
int wgbsseg_blocks_write_bedgraph(const char* path, const char* text, const int64_t* line_off, const int32_t* len3, int64_t n_rows,
                                  const void* rows, int32_t wide, int32_t threads, char* err, size_t errlen);
int64_t wgbsseg_format_fixed(const double* v, int64_t n, int32_t digits, char* out, int64_t out_cap);

/*
 * The text of `wgbstools convert -L` (convert.py:44-89: pandas.read_csv of a BED table, the two CpG columns inserted after the
 * third, DataFrame.to_csv).  Host side.  wgbsseg_bed_parse: rows of a BED table whose text can go back out VERBATIM around the
 * new columns -> per row its offset, the length of "chr \t start \t end" (len3) and of the whole row (row_len), the index of
 * its chromosome in chrom_names (-1: none of them), start and end.  A FAST PATH like wgbsseg_blocks_parse: returns 1 — and the
 * caller's own parser takes over — for anything a round trip through pandas would re-print: '#' comments, rows
 * of different widths, starts / ends that are not plain integers, columns that read as numbers and would print differently
 * (integers with gaps come back as floats, 0.50 as 0.5, +5 as 5; plain integers and decimals in their shortest form pass) or
 * hold missing-value spellings other than NA, carriage returns, non-ASCII bytes, an empty table.  *width = fields per row;
 * *header = 1 when the first line was a header (second and third fields not numbers): it is skipped, the caller prints the
 * reference's note, and every column of such a table is text.
 * wgbsseg_bed_write_annotated: row r as its first len3 bytes, \t startCpG \t endCpG (NA for 0), the rest of the row, \n — to
 * `path` (truncated first; NULL: standard output).
 */
int wgbsseg_bed_parse(const char* text, int64_t len, int64_t cap, const char* const* chrom_names, int32_t n_chroms, int64_t* line_off,
                      int32_t* len3, int32_t* row_len, int32_t* chrom, int64_t* start, int64_t* end, int64_t* n_rows, int32_t* width, int32_t* header);
/* test hook: out[i] = 1 when the i-th newline-separated token is a decimal number that prints as it reads after a round trip
 * through a float (csrc/table_io.h: canonical_float); returns the number of tokens, -1 when out_cap is too small */
int64_t wgbsseg_debug_canonical_float(const char* tokens, int64_t len, uint8_t* out, int64_t out_cap);
int wgbsseg_bed_write_annotated(const char* path, const char* text, const int64_t* line_off, const int32_t* len3, const int32_t* row_len,
                                const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_rows, int32_t threads, char* err, size_t errlen);

/*
 * pat -> beta: the producer of the path's input (`wgbstools pat2beta`: pat2beta.py:17-44 pipes `gunzip -c x.pat.gz` into
 * the reference's stdin2beta binary, src/pat2beta/stdin2beta.cpp:59-123, and trims the counts with trim_to_uint8,
 * utils_wgbs.py:277-290).  An accumulator holds (#meth, #cov) of the CpGs [start_cpg, end_cpg) (1-based, half-open; the whole
 * genome: [1, nr_sites + 1)) on one device.  feed(): a chunk of pat TEXT made of whole lines
 * "chr \t first CpG index \t pattern over {C,T,H,.} \t count [\t ...]": every site under a C / T / H gains `count`
 * coverage, under C / H also `count` methylated; reads outside the range are skipped, empty lines too.  Asynchronous (the
 * text is copied): the caller decompresses the next chunk meanwhile.  finish(): `.beta` rows (uint8 pairs; lbeta != 0:
 * `.lbeta`, uint16 pairs) into out[2 * (end - start)], coverage above the type's maximum M scaled to (trunc(meth / cov * M), M).
 * A line with fewer than four fields, or whose site / count is not a number, is an error (the reference prints "failed
 * calculating beta" and writes nothing): finish() returns WGBSSEG_E_ARG naming the byte offset of the line.
 */
typedef struct wgbsseg_patbeta wgbsseg_patbeta;
int wgbsseg_patbeta_create(int device, int64_t start_cpg, int64_t end_cpg, wgbsseg_patbeta** out, char* err, size_t errlen);
int wgbsseg_patbeta_feed(wgbsseg_patbeta* pb, const char* text, int64_t n_bytes, char* err, size_t errlen);
int wgbsseg_patbeta_finish(wgbsseg_patbeta* pb, int32_t lbeta, void* out, char* err, size_t errlen);
void wgbsseg_patbeta_destroy(wgbsseg_patbeta* pb);
/* device time (ms, HIP events) of the counting-kernel launches of all chunks fed so far; waits for them.  < 0: error */
double wgbsseg_patbeta_kernel_ms(wgbsseg_patbeta* pb);

/*
 * pat -> per-block U / X / M read counts (`wgbstools homog`: homog.py:61-131 pipes `gunzip -c x.pat.gz` into the reference's
 * homog binary, src/homog/homog.cpp:154-260).  create(): the blocks [start_cpg[j], end_cpg[j]) already sorted by
 * (startCpG, endCpG) (refused otherwise; startCpG >= 1, endCpG > startCpG, endCpG < 2^31), the bin edges range[0 .. n_bins]
 * (ascending float32, 1 <= n_bins <= 8), min_cpgs (the reference's -l) and inclusive (--inclusive).  feed(): a chunk of pat
 * TEXT made of whole lines, as for wgbsseg_patbeta_feed (asynchronous, the text is copied).  A read `chr, s, pattern, count`
 * covering [s, s + len) adds `count` to one bin of every block it overlaps, as long as s < endCpG of the LAST block: the
 * pattern clipped to the overlap (inclusive: the whole pattern) must be at least min_cpgs long and hold at least min_cpgs
 * C / H / T; meth = (float)#C,H / (float)#C,H,T picks bin b with range[b] <= meth < range[b + 1] (meth == 1: the last bin).
 * finish(): counts[n_blocks * n_bins] (int32, row-major, sorted block order).  finish() returns WGBSSEG_E_ARG naming the byte
 * offset of the first malformed line (fewer than four fields, a site / count that is not a number), or else of the first read
 * that starts before the read before it (the reference's output then depends on the reads' order).
 * wgbsseg_homog_kernel_ms: device time (HIP events) of the counting kernel over all chunks fed so far; waits for them.
 * wgbsseg_debug_homog_bins (test hook, device 0): out[t (t + 1) / 2 + nrC] = the device's bin for every (nrC, nrT) with
 * t = nrC + nrT <= max_total (-1: below range[0]).
 */
typedef struct wgbsseg_homog wgbsseg_homog;
int wgbsseg_homog_create(int device, const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, const float* range, int32_t n_bins,
                         int32_t min_cpgs, int32_t inclusive, wgbsseg_homog** out, char* err, size_t errlen);
int wgbsseg_homog_feed(wgbsseg_homog* h, const char* text, int64_t n_bytes, char* err, size_t errlen);
int wgbsseg_homog_finish(wgbsseg_homog* h, int32_t* counts, char* err, size_t errlen);
void wgbsseg_homog_destroy(wgbsseg_homog* h);
double wgbsseg_homog_kernel_ms(wgbsseg_homog* h);
int wgbsseg_debug_homog_bins(const float* range, int32_t n_bins, int32_t max_total, int8_t* out);

/*
 * pat -> per-block two-allele EM test (`wgbstools test_bimodal`: test_bimodal.py:25-176 asks tabix for the reads of each block
 * and runs numpy's EM over them).  create(): the blocks [start_cpg[j], end_cpg[j]) in any order (1 <= startCpG < endCpG < 2^31),
 * strict (--strict: clip the reads to the block), min_len (>= 1), max_lds_cols (< 0: the default; 0 forces every block onto the
 * global-memory path: a test hook).  feed(): a chunk of pat TEXT made of whole lines, as for wgbsseg_homog_feed; it first waits for
 * the previous chunk's parse, runs the EM of the blocks that chunk completed (queued: it overlaps the caller's next inflate) and
 * drops the reads no pending block can reach.  A block uses the reads starting in [max(1, s1 - 150), s2 - 1] (s1 = startCpG,
 * s2 = endCpG), skips those ending at or before s1, clips them with strict, drops those shorter than min_len; each line stands for
 * `count` identical rows; only C and T are observations.  finish(): per block in the order given, ll[3 j ..] = {ll0 (one allele),
 * ll_em (the EM's last likelihood), the sum of the columns' 2e-3 + #C + #T}, counts[3 j ..] = {columns, rows, EM iterations}
 * (rows 0: nothing computed, the reference's p = 1).  The sums are taken in the reference's order: see bimodal_kernels.h.
 * finish() returns WGBSSEG_E_ARG naming the byte offset of the first malformed line, else of the first negative count, else of
 * the first read that starts before the read before it; WGBSSEG_E_CAPACITY for a block of 2^31 rows or more.
 * wgbsseg_bimodal_kernel_ms: device time (HIP events) of all launches so far; waits for them.
 * wgbsseg_debug_bimodal_terms (test hook, device 0): the arithmetic the EM kernel applies to a pair of column counts, for `count`
 * pairs (a[q], b[q]) (count <= 2^28).  With pa = 1e-3 + a, pb = 1e-3 + b, n = pa + pb: out holds six rows of `count` double bit
 * patterns, out[k * count + q] = pa / n, pb / n, log2(pa / n), log2(pb / n), n, a * log2(pa / n) + b * log2(pb / n) for k = 0 .. 5.
 */
typedef struct wgbsseg_bimodal wgbsseg_bimodal;
int wgbsseg_bimodal_create(int device, const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, int32_t strict, int32_t min_len,
                           int32_t max_lds_cols, wgbsseg_bimodal** out, char* err, size_t errlen);
int wgbsseg_bimodal_feed(wgbsseg_bimodal* b, const char* text, int64_t n_bytes, char* err, size_t errlen);
int wgbsseg_bimodal_finish(wgbsseg_bimodal* b, double* ll, int64_t* counts, char* err, size_t errlen);
void wgbsseg_bimodal_destroy(wgbsseg_bimodal* b);
double wgbsseg_bimodal_kernel_ms(wgbsseg_bimodal* b);
int wgbsseg_debug_bimodal_terms(const uint32_t* a, const uint32_t* b, int64_t count, uint64_t* out);

/*
 * BGZF bytes as they lie in a .pat.gz, inflated on the device (the second way to feed the three engines above; an engine takes text or
 * BGZF bytes, not both).  feed_bgzf(): `bytes` = any number of whole BGZF members (gzip members of at most 64 KB of text whose extra
 * field holds the 'BC' subfield), possibly followed by the beginning of one more; *consumed = the bytes of the whole members, the
 * caller hands the rest in again in front of what follows in the file.  The members are inflated by one kernel launch, one member per
 * wavefront, into the text buffer the engine's kernels read; the text behind the call's last newline is kept on the host and put in
 * front of the next call's text, so lines may straddle members and calls, and byte offsets in finish()'s refusals are those of the
 * inflated text, as with feed().  finish() first feeds a last line that has no newline.  Refused at once, naming the file offset: a
 * member that is gzip but not BGZF, a BSIZE smaller than the member's header and trailer, ISIZE > 65536, and a corrupt member among
 * those the host inflates to find the last newline.  A corrupt member met on the device is reported by finish(), before any refusal
 * of the text: "Invalid gzip data: BGZF member at file offset N: <what>".  A stream is accepted where zlib's raw inflate accepts it and
 * its text is ISIZE bytes long; CRC32 is not checked.
 * inflate_ms(): device time (HIP events) of the inflate launches so far; waits for them.  < 0: error.
 * wgbsseg_bgzf_inflate: the whole members of `bytes` inflated on `device` into out[0 .. *out_len) (WGBSSEG_E_CAPACITY when out_cap is
 * too small; *consumed as above); WGBSSEG_E_ARG with the message above for the first corrupt member (its text reads '\n' from where
 * the decoder stopped).
 */
int wgbsseg_patbeta_feed_bgzf(wgbsseg_patbeta* pb, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen);
int wgbsseg_homog_feed_bgzf(wgbsseg_homog* h, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen);
int wgbsseg_bimodal_feed_bgzf(wgbsseg_bimodal* b, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen);
double wgbsseg_patbeta_inflate_ms(wgbsseg_patbeta* pb);
double wgbsseg_homog_inflate_ms(wgbsseg_homog* h);
double wgbsseg_bimodal_inflate_ms(wgbsseg_bimodal* b);
int wgbsseg_bgzf_inflate(int device, const void* bytes, int64_t n_bytes, void* out, int64_t out_cap, int64_t* out_len, int64_t* consumed,
                         char* err, size_t errlen);

/*
 * pat -> the histogram of the reads' lengths in CpGs, weighted by the reads' counts (`wgbstools frag_len`: frag_len.py:21-46 pipes
 * `tabix` or the reference's cview into an awk program).  create(): max_frag (the reference's -m; 1 .. 2^20), and the blocks that
 * select reads: n_blocks == 0 selects every read; otherwise [start_cpg[j], end_cpg[j]) in the order `sort -k1,1n` gives the text
 * "startCpG\tendCpG" (startCpG ascending, refused otherwise; equal starts in the caller's order; startCpG >= 1, endCpG > startCpG,
 * endCpG < 2^31) — one block for a region or a site range.  groups: the cap on the workgroups of a launch (-1: the default; a small
 * value makes every workgroup walk many tiles: a test hook).  feed() / feed_bgzf(): as for wgbsseg_homog (asynchronous, the text is
 * copied; text or BGZF bytes, not both).  A selected read `chr, s, pattern, count` adds count to hist[min(len(pattern), max_frag) - 1].
 * The selection is cview's without --strict on reads sorted by start (src/cview/cview.cpp:87-128): a read is dropped when
 * s >= endCpG of the LAST block given; else, with cur the first block whose endCpG > s, it is selected — whole — iff
 * s + len - 1 >= startCpG[cur].  finish(): hist[max_frag] (int64: exact sums); it first feeds a last line that has no newline, then
 * returns WGBSSEG_E_ARG for a BGZF member refused on the device, else naming the byte offset of the first malformed line (fewer than
 * four fields, a site / count that is not a number, an EMPTY pattern), else — with blocks only — of the first read that starts before
 * the read before it.  kernel_ms / inflate_ms: device time (HIP events) of the histogram / inflate launches so far; wait for them.
 */
typedef struct wgbsseg_fraglen wgbsseg_fraglen;
int wgbsseg_fraglen_create(int device, int32_t max_frag, const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, int32_t groups,
                           wgbsseg_fraglen** out, char* err, size_t errlen);
int wgbsseg_fraglen_feed(wgbsseg_fraglen* h, const char* text, int64_t n_bytes, char* err, size_t errlen);
int wgbsseg_fraglen_feed_bgzf(wgbsseg_fraglen* h, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen);
int wgbsseg_fraglen_finish(wgbsseg_fraglen* h, int64_t* hist, char* err, size_t errlen);
void wgbsseg_fraglen_destroy(wgbsseg_fraglen* h);
double wgbsseg_fraglen_kernel_ms(wgbsseg_fraglen* h);
double wgbsseg_fraglen_inflate_ms(wgbsseg_fraglen* h);

/*
 * pat -> pat: the reads an interval of CpG indexes lets through, cut, sorted and collapsed (`wgbstools view` / `cview` with one
 * block: src/cview/cview.cpp:8-17,:87-167, patter_utils.cpp:260-280, `sort -k2,2n -k3,3`, collapse_pat.pl).  create(): the interval
 * [start_cpg, end_cpg) (start_cpg >= 1, end_cpg > start_cpg, end_cpg < 2^31; the whole genome is [1, nr_sites + 1)); flags, a sum of
 * WGBSSEG_VIEW_STRICT (1), _STRIP (2), _NO_GAPS (4) and _SORT (8); min_len >= 1; initial_records: the first size of the record table
 * (<= 0: the default; a small value makes the table and the arena grow: a test hook).  feed() / feed_bgzf(): as for wgbsseg_homog
 * (text or BGZF bytes, not both); a call first waits for the chunk before it.  Per line `chrom, rs, pattern, count`: dropped when
 * rs >= end_cpg or rs + len - 1 < start_cpg; STRICT cuts the pattern to the interval; STRIP removes trailing, then leading dots
 * (moving rs; nothing but dots: dropped); dropped when min_len exceeds what is left; NO_GAPS drops a read that still holds a '.'.
 * finish(): with SORT the survivors are ordered by rs, then the pattern's bytes, then the chromosome's (a prefix first; ties by input
 * position), else they keep the input order; adjacent lines equal in all three become one with the int64 sum of their counts, a sum
 * <= 0 prints nothing; the text "chrom\trs\tpattern\tsum\n" stays on the device, deflated there into BGZF members (wgbsseg_bgzf_deflate's
 * member rule, the end-of-file member last) when `deflate` is not 0.  *n_lines: the lines; *n_bytes: the bytes read() hands out.
 * finish() first feeds a last line that has no newline, then returns WGBSSEG_E_ARG for a BGZF member refused on the device, else
 * "failed in view: ..." naming the byte offset of the first malformed line (fewer than four fields, a site / count that is not a
 * number, an empty pattern, any byte between the count's digits and the newline), else of the first read that starts before the read
 * before it (always checked), else for a sum of 10^15 or more.  read(): bytes [offset, offset + len) of the result, after finish().
 * kernel_ms / inflate_ms: device time of the chunk launches / inflate launches so far; phase_ms: of finish()'s sort, collapse + emit
 * and deflate.  info(): out[6] = records kept, arena bytes, growths of the record table, growths of the arena, merge passes run,
 * order (0: no sort asked, 1: found in order, no sort run, 2: sorted).
 *
 * Several files in one view (`wgbstools merge`): next_file() between the feeds of two files.  It feeds a last line that has no newline
 * as finish() does, refuses (WGBSSEG_E_ARG) BGZF bytes that the last feed_bgzf() left over — they are no whole member —, and makes the
 * feed forget the file: text or BGZF may change from file to file, member offsets count from 0 again, and the next file may begin
 * below where this one ended (reads ascend inside a file, not across files).  The records of all files share the one table in input
 * order, so finish() sorts and collapses them together and ties still break by (file, line).  After a next_file() call finish() names
 * the file (0-based, in feed order) and the byte offset inside it: "failed in view: file K: invalid line at byte offset N of the file
 * ...", "... file K: the pat file is not sorted: the read at byte offset N of the file ...", and it refuses a count below 1 in any
 * line, "failed in view: file K: count < 1 at byte N" — the reference collapses every file by itself before it merges them, so a run
 * whose sum is <= 0 vanishes there while it would be summed into the other files' runs here; with counts of at least 1 the two agree.
 * Without a next_file() call everything is as described above.  WGBSSEG_E_STATE after finish().
 *
 * Hidden sites (`wgbstools mask_pat`: src/pat2beta/mask_pat.cpp:12-104): set_mask() once, after create() and before the first feed() /
 * feed_bgzf() (WGBSSEG_E_STATE otherwise).  The hidden sites are the union of the blocks [start_cpg[k], end_cpg[k]), which may come in
 * any order and may overlap, nest and repeat; WGBSSEG_E_ARG, with the block's index in the message, for start_cpg < 1, end_cpg <=
 * start_cpg, end_cpg >= 2^31, and for an empty list.  The blocks become a bitmap on the device, built on the feed's stream before the
 * call returns.  Every read is then cut as above with one step between STRICT and STRIP: every pattern byte that is not '.' and whose
 * site rs + i is hidden becomes '.' — selection looks at the read as the file has it, STRIP / min_len / NO_GAPS at the read as the mask
 * leaves it (mask_pat itself is STRIP | SORT with min_len 1).  With a mask finish() refuses a count below 1 in a single file too,
 * "failed in view: count < 1 at byte N", for the reason above: the reference collapses once before it masks.  mask_info(): out[3] =
 * hidden sites (the reference's `loaded N sites`), words of the bitmap, 1 when a mask is set; mask_ms(): device time of the launch that
 * built the bitmap.  Without a set_mask() call everything is as described above.
 *
 * Sources and labels (`wgbstools mix_pat`: src/python/mix_pat.py, merge.py:17-100, src/pat_sampler/sampler.cpp): set_labels() once, after
 * create() and before the first feed (WGBSSEG_E_STATE otherwise, and on an engine that has a mask; set_mask() is refused after it), on an
 * engine created with WGBSSEG_VIEW_SORT.  labels: n <= 255 distinct names, each non-empty and of printable ASCII without white space,
 * '/', '&' and '\' (WGBSSEG_E_ARG otherwise).  A label's rank is its place among them in byte order, a prefix first; label_rank(k): the
 * rank of labels[k] (-1: no such label).  From then on every file needs set_source() — after create() or next_file() and before the
 * file's first feed (WGBSSEG_E_STATE otherwise; a feed of a file without one is WGBSSEG_E_STATE too); WGBSSEG_E_ARG for reps < 1 or above
 * 2^20, T > 2^30, a rank at or above the number of labels (so also without labels).  A read of the file that the cut lets through is
 * thinned: of n = count * reps draws, draw j succeeds when word j & 3 of Philox4x32-10(counter {off lo32, off hi32, j >> 2, stream},
 * key {seed lo32, seed hi32}) is below T = floor(p * 2^32); off is the byte offset of the line in its file's text, so the result does
 * not depend on how the file is cut into calls nor on where it is inflated.  The read goes on with the number of successes as its count,
 * and not at all when that is 0; its line gets the file's label as a fifth column.  finish(): the label is the last key of the order and
 * of the collapse, so lines of two labels never merge; the lines that tie in start, pattern and chromosome — at most one per label — come
 * in the order of the reference's `sort -m -k2,2n -k3,3`: by the decimal text of their sums, a prefix first ("1" < "10" < "9"), then by
 * label.  The text is "chrom\trs\tpattern\tsum\tlabel\n".  A count below 1 is refused as with a mask; a line with count * reps above
 * 2^20 is refused, "failed in view: [file K: ]count * reps above 2^20 at byte N".  sample_info(): out[3] = the reads that reached the
 * sampler, the reads it dropped, the sum of the counts it kept (waits for the stream).  Without these calls everything is as described
 * above.
 */
#define WGBSSEG_VIEW_STRICT 1
#define WGBSSEG_VIEW_STRIP 2
#define WGBSSEG_VIEW_NO_GAPS 4
#define WGBSSEG_VIEW_SORT 8
typedef struct wgbsseg_patview wgbsseg_patview;
int wgbsseg_patview_create(int device, int64_t start_cpg, int64_t end_cpg, int32_t flags, int32_t min_len, int64_t initial_records,
                           wgbsseg_patview** out, char* err, size_t errlen);
int wgbsseg_patview_feed(wgbsseg_patview* v, const char* text, int64_t n_bytes, char* err, size_t errlen);
int wgbsseg_patview_feed_bgzf(wgbsseg_patview* v, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen);
int wgbsseg_patview_finish(wgbsseg_patview* v, int64_t* n_lines, int64_t* n_bytes, int32_t deflate, char* err, size_t errlen);
int wgbsseg_patview_read(wgbsseg_patview* v, int64_t offset, void* buf, int64_t len, char* err, size_t errlen);
void wgbsseg_patview_destroy(wgbsseg_patview* v);
double wgbsseg_patview_kernel_ms(wgbsseg_patview* v);
double wgbsseg_patview_inflate_ms(wgbsseg_patview* v);
void wgbsseg_patview_phase_ms(const wgbsseg_patview* v, double* sort_ms, double* emit_ms, double* deflate_ms);
void wgbsseg_patview_info(const wgbsseg_patview* v, int64_t* out);
int wgbsseg_patview_next_file(wgbsseg_patview* v, char* err, size_t errlen);
int wgbsseg_patview_set_mask(wgbsseg_patview* v, const int64_t* start_cpg, const int64_t* end_cpg, int64_t n_blocks, char* err, size_t errlen);
void wgbsseg_patview_mask_info(const wgbsseg_patview* v, int64_t* out);
double wgbsseg_patview_mask_ms(const wgbsseg_patview* v);
int wgbsseg_patview_set_labels(wgbsseg_patview* v, const char* const* labels, int64_t n, char* err, size_t errlen);
int32_t wgbsseg_patview_label_rank(const wgbsseg_patview* v, int64_t label);
int wgbsseg_patview_set_source(wgbsseg_patview* v, int32_t label_rank, uint32_t T, int32_t reps, uint64_t seed, uint32_t stream, char* err, size_t errlen);
void wgbsseg_patview_sample_info(wgbsseg_patview* v, int64_t* out);

/*
 * SAM text in place of pat text (`wgbstools bam2pat`: src/python/bam2pat.py:144-209, src/pipeline_wgbs/patter.cpp, patter_utils.cpp):
 * set_sam() once, after create() and before the first feed (WGBSSEG_E_STATE otherwise, and on an engine that has a mask or labels;
 * set_mask(), set_labels() and next_file() are refused after it), on an engine created with WGBSSEG_VIEW_SORT and no other flag
 * (WGBSSEG_E_ARG otherwise).  loci, n_sites and the chromosome table are those of wgbsseg_bedbeta_create (below), with its checks and
 * messages.  feed() / feed_bgzf() then take what `samtools view [-h]` prints, cut anywhere between two lines (feed_bgzf: anywhere):
 *   lines     empty lines are skipped; a line that begins with '@' is a header.  Only the first ten fields are read.
 *   filter    a line stays when (FLAG & exclude_flags) == 0, (FLAG & include_flags) == include_flags and MAPQ >= mapq; strand 1 (top)
 *             keeps FLAG 99 / 147 (paired) or 0, strand 2 (bottom) FLAG 83 / 163 (paired) or 16.  A line of fewer than 11 fields, or
 *             whose FLAG or MAPQ is not made of decimal digits, is invalid: it is not filtered and keeps its place among the mates.  A
 *             line that passes the filter and names a chromosome the table does not have is dropped.
 *   one line  CIGAR: M = X copy bases, D N insert 'N', I S skip bases, H nothing; any other operation, '*', a missing number, an
 *             operation past SEQ, a POS that is not decimal digits, a QNAME above 254 bytes: invalid.  At every CpG of RNAME at locus
 *             POS + i inside the adjusted sequence: a top read (paired: not (FLAG & 0x53) == 83 and not (FLAG & 0xA3) == 163; single:
 *             FLAG & 0x10 clear) gives C for "CG", T for "TG" at i; a bottom read gives C for "CG", T for "CA" at i, looked at at
 *             j = i + 1; anything else '.'; clip: '.' when j < clip or j >= length - clip.  The pat runs from the first called site
 *             to the last; none: the read is empty.
 *   mates     paired != 0: two consecutive lines that stay, with equal QNAME and equal RNAME, are a pair — greedily: of k such lines
 *             (1, 2), (3, 4), ... pair and an odd last one is single.  (The reference streams every chromosome by itself, so only lines
 *             of one chromosome meet there; mates are adjacent, as Bismark and bwa-meth write them.)
 *   merge     an empty or invalid side: the other as it is.  Else from the earlier start, a site both call differently becomes '.',
 *             trailing then leading dots go; a span above 300 sites drops the pair; a result shorter than min_cpg is dropped.
 * Every result is a record with count 1; finish() sorts, collapses, writes and deflates them as it does the reads of pat text (the
 * ascending-start check does not apply).  The bytes that come out do not depend on how the text is cut into calls or BGZF members.
 * sam_info(): out[10] = lines, header lines, filtered, invalid, unknown chromosome, empty, short, pairs, lines of a paired file left
 * single, pairs merged too long (waits for the stream).  kernel_ms(): the device time of the SAM kernels.
 */
int wgbsseg_patview_set_sam(wgbsseg_patview* v, const uint32_t* loci, int64_t n_sites, const char* const* chrom_names, const int64_t* chrom_lo, const int64_t* chrom_hi,
                            int32_t n_chroms, int32_t paired, int64_t exclude_flags, int64_t include_flags, int32_t mapq, int32_t strand, int32_t clip, int32_t min_cpg,
                            char* err, size_t errlen);
void wgbsseg_patview_sam_info(wgbsseg_patview* v, int64_t* out);

/*
 * BED methylation calls -> .beta (`wgbstools bed2beta`: bed2beta.py:11-51, a pandas drop_duplicates and a left merge with the CpG
 * dictionary; utils_wgbs.py:277-290 trim_to_uint8).  create(): loci[n_sites] (uint32, the bp position of every CpG; n_sites < 2^31), and
 * the genome's chromosomes: chromosome k is named chrom_names[k] and owns the sites [chrom_lo[k], chrom_hi[k]) (0-based).  WGBSSEG_E_ARG,
 * naming the chromosome, unless 1 <= n_chroms <= 65,535, the names are non-empty, distinct and free of tabs and newlines, the ranges are
 * disjoint and inside [0, n_sites), and the loci ascend strictly inside every chromosome.  flags: WGBSSEG_BED_ADD_ONE (1): a line's
 * position is start + 1; WGBSSEG_BED_HEADER (2): the line at byte offset 0 of the file is a header and is dropped unread (the caller
 * decides: the reference takes the first line for a header exactly when its second field is not made of decimal digits only).  The loci
 * and the table go to the device once, for all files.  feed() / feed_bgzf(): as for wgbsseg_homog (asynchronous, the text is copied; text
 * or BGZF bytes, not both; at most 2^47 bytes of text per file).  Per line `chr \t start \t end \t #meth \t #total [\t ...]` — the third
 * field and everything behind the fifth are not looked at, empty lines are skipped —: with p = start (+ 1) the line matches site i when
 * chr equals a chromosome's name byte for byte and loci[i] == p inside that chromosome's sites.  A line on an unknown chromosome or at a
 * position that is no CpG is dropped and counted.  Of several lines that match one site the FIRST in the file wins, however the file is
 * cut into calls, tiles or BGZF members.  finish(): out[n_sites * 2] (host), per site the winning line's (#meth, #total), where #total >
 * 255 stored as (trunc(#meth / #total * 255), 255) (float64, the reference's order of operations), 0, 0 for a site without a line;
 * stats[6] (may be NULL) = lines read, lines matched, lines dropped for an unknown chromosome, lines dropped for not being a CpG,
 * duplicates dropped among the matched lines, sites set.  It first feeds a last line that has no newline, then returns WGBSSEG_E_ARG for
 * a BGZF member refused on the device, else "failed in bed2beta: the line at byte offset N of the input ..." for the lowest line that has
 * fewer than five fields; whose start, #meth or #total is not 1 to 18 decimal digits and nothing else (no sign, no '.', no exponent, no
 * '\r'); whose #total exceeds 2^31 - 1; or whose #meth exceeds its #total (the reference would wrap it).  next_file(): after finish(),
 * before the next file's first feed: clears the table, the counters and the refusal, makes the feed forget the file (text or BGZF may
 * change, byte and member offsets count from 0 again) and sets the next file's flags; WGBSSEG_E_ARG when the last feed_bgzf() left bytes
 * over (no whole member).  kernel_ms / inflate_ms: device time (HIP events) of the k_bedbeta_scan / inflate launches so far, over all
 * files; wait for them.
 */
#define WGBSSEG_BED_ADD_ONE 1
#define WGBSSEG_BED_HEADER 2
typedef struct wgbsseg_bedbeta wgbsseg_bedbeta;
int wgbsseg_bedbeta_create(int device, const uint32_t* loci, int64_t n_sites, const char* const* chrom_names, const int64_t* chrom_lo,
                           const int64_t* chrom_hi, int32_t n_chroms, int32_t flags, wgbsseg_bedbeta** out, char* err, size_t errlen);
int wgbsseg_bedbeta_feed(wgbsseg_bedbeta* b, const char* text, int64_t n_bytes, char* err, size_t errlen);
int wgbsseg_bedbeta_feed_bgzf(wgbsseg_bedbeta* b, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen);
int wgbsseg_bedbeta_finish(wgbsseg_bedbeta* b, uint8_t* out, int64_t* stats, char* err, size_t errlen);
int wgbsseg_bedbeta_next_file(wgbsseg_bedbeta* b, int32_t flags, char* err, size_t errlen);
void wgbsseg_bedbeta_destroy(wgbsseg_bedbeta* b);
double wgbsseg_bedbeta_kernel_ms(wgbsseg_bedbeta* b);
double wgbsseg_bedbeta_inflate_ms(wgbsseg_bedbeta* b);

/*
 * FASTA text -> the CpG dictionary (`wgbstools init_genome`: init_genome.py:142-179, 246-260, where `samtools faidx`, a regular
 * expression per chromosome, `bgzip` and `tabix` do it).  The rule (csrc/fasta_core.h, the same functions on the host and on the device):
 *   header   a line that begins with '>' — as the first byte of the input or right after '\n' — up to the next '\n'; the sequence's name
 *            is what follows the '>' up to the first space, tab, '\r' or '\n'
 *   bases    every other byte that is not '\n' or '\r' is a base of the current sequence; bases count from 1
 *   sites    a base C / c whose next base in the same sequence is G / g, whatever line breaks lie between them; its locus is the C's number
 * That is the reference's ''.join(s.strip() ...).upper() + finditer('CG') for every FASTA whose lines carry no blanks; a '\r' is skipped
 * wherever it stands.  feed() / feed_bgzf(): the text or the bytes of a BGZF file, not both; asynchronous, the bytes are copied; A CALL
 * MAY END AT ANY BYTE (an unwrapped chromosome is one line of 250 MB): what a call leaves open — the state, the sequence and its bases so
 * far, a C whose next base has not come yet — is carried on the device.  The results do not depend on how the input is cut into calls,
 * tiles or BGZF members.  finish_scan(): once, after the last feed; counts[3] = sequences, sites, bytes of text.  WGBSSEG_E_ARG for a BGZF
 * member refused on the device, else "Invalid FASTA: <what> at byte offset N of the text" for the lowest N among: a byte other than '\n' /
 * '\r' before the first header (the byte); a header with an empty name (its '>'); a name of more than 255 bytes (its '>'); a byte of a
 * sequence outside 0x21 .. 0x7E that is not '\n' or '\r' (the byte); a sequence of more than 2^32 - 2 bases (its '>'); else for two
 * sequences with one name.  sequences(): per sequence, in FASTA order, the offset of its header, its bases, its sites, the length of its
 * name and the name (256 bytes each, zero-padded); any pointer may be NULL.  select(): order[n_order], the sequences the dictionary keeps,
 * in the dictionary's order, each at most once (which sequences are chromosomes and how they are sorted is the caller's rule:
 * init_genome.py's is_valid_chrome and chromosome_order); none: WGBSSEG_E_ARG, "no chromosome is kept".  Their loci are gathered into one
 * array, *n_sites long; loci(): that array (what `loci.u32` holds; n must be *n_sites).  dict(): `name \t locus \t site \n` per selected
 * site, site counting from 1 over the dictionary, formatted on the device; deflate != 0: as BGZF members, the end-of-file member last
 * (what wgbsseg_bgzf_deflate writes).  *n_lines, *n_bytes: of the result, which stays on the device; read(): its bytes [offset, offset +
 * len).  kernel_ms: device time (HIP events) of the measure, scan and pack launches so far; inflate_ms: of the inflate launches; both wait
 * for them.  phase_ms: the gather of select(), the emit and the deflate of dict().
 * wgbsseg_debug_fasta_walk (test hook, no device): the same rule run serially over text[0, n) on the host, into tables with room for
 * cap_seqs sequences and cap_loci loci (WGBSSEG_E_CAPACITY when they do not suffice); counts[2] = sequences, sites; *refused: (offset << 8
 * | reason) of the first refusal (reasons 1 .. 5 in the order above), ~0: none.
 */
typedef struct wgbsseg_fasta wgbsseg_fasta;
int wgbsseg_fasta_create(int device, wgbsseg_fasta** out, char* err, size_t errlen);
int wgbsseg_fasta_feed(wgbsseg_fasta* f, const char* text, int64_t n_bytes, char* err, size_t errlen);
int wgbsseg_fasta_feed_bgzf(wgbsseg_fasta* f, const void* bytes, int64_t n_bytes, int64_t* consumed, char* err, size_t errlen);
int wgbsseg_fasta_finish_scan(wgbsseg_fasta* f, int64_t* counts, char* err, size_t errlen);
int wgbsseg_fasta_sequences(wgbsseg_fasta* f, int64_t* hdr_off, int64_t* n_bases, int64_t* n_sites, int32_t* name_len, char* names, char* err, size_t errlen);
int wgbsseg_fasta_select(wgbsseg_fasta* f, const int64_t* order, int64_t n_order, int64_t* n_sites, char* err, size_t errlen);
int wgbsseg_fasta_loci(wgbsseg_fasta* f, uint32_t* out, int64_t n, char* err, size_t errlen);
int wgbsseg_fasta_dict(wgbsseg_fasta* f, int32_t deflate, int64_t* n_lines, int64_t* n_bytes, char* err, size_t errlen);
int wgbsseg_fasta_read(wgbsseg_fasta* f, int64_t offset, void* buf, int64_t len, char* err, size_t errlen);
void wgbsseg_fasta_destroy(wgbsseg_fasta* f);
double wgbsseg_fasta_kernel_ms(wgbsseg_fasta* f);
double wgbsseg_fasta_inflate_ms(wgbsseg_fasta* f);
void wgbsseg_fasta_phase_ms(const wgbsseg_fasta* f, double* gather_ms, double* emit_ms, double* deflate_ms);
int wgbsseg_debug_fasta_walk(const char* text, int64_t n, int64_t cap_seqs, int64_t cap_loci, int64_t* hdr_off, int64_t* n_bases, int64_t* n_sites, int32_t* name_len,
                             char* names, uint32_t* loci, int64_t* counts, uint64_t* refused);

int wgbsseg_get_timings(const wgbsseg_ctx* ctx, wgbsseg_timings* out);

/*
 * Test hooks (used by tests/ to compare device intermediates with the oracle; not part of the drop-in surface).
 * wgbsseg_debug_fetch copies an intermediate of the LAST wgbsseg_segment_chunks() call to a host buffer:
 *   "window"  uint16[sites]   F_k (number of admissible ends of a block starting at k)
 *   "cum"     uint32[sites]   exclusive prefix of F inside each chunk (row offset of start site k; chunk-relative: 0 at
 *                             every chunk's first site)
 *   "back"    uint16[sites]   i+1-argmax_k of M[i+1]
 *   "cost"    double[pairs]   scored blocks, only if every stage of the call kept a buffer to itself: one stage
 *                             (WGBSSEG_FORCE_STAGES=1 makes it so), two stages, or three gated ones (n_stages <= nbuf of
 *                             wgbsseg_debug_last_plan; WGBSSEG_E_STATE otherwise: a later stage has overwritten an earlier
 *                             one's blocks).  A staged call's rows are put together on the host, stage after stage: the
 *                             whole row of a start site lies in the buffer of the stage that holds the START, also when
 *                             its blocks end beyond the stage bound.
 * Layout, for a call of any number of chunks: DENSE, chunk after chunk in the caller's order.  sites = the sum of the
 * chunks' lengths, and chunk c's entries begin at the sum of the lengths before it — the padding the library keeps
 * between the chunks' slices of its own arrays (each begins at a multiple of 8 entries) is left out.  pairs = the sum
 * of F over all sites; chunk c's rows begin at the sum of F over the chunks before it, wherever the library placed
 * them in its cost buffer.  Inside a chunk the rows are start-major: row k (at the chunk's "cum"[k]) holds the blocks
 * that start at site k and end at k .. k+F_k-1.
 * Returns the number of bytes written, or a negative code (WGBSSEG_E_CAPACITY: cap_bytes is less than that).
 * wgbsseg_debug_last_plan reports the form the LAST wgbsseg_segment_chunks() call took, as the library decided and
 * launched it (copied when the call ended; the hook launches nothing and touches no stream).  With S = out[0]:
 *   out[0] n_stages   out[1] gated (the stages alternated between the scoring streams behind the gate)
 *   out[2] nbuf (scored-block buffers)   out[3] last_pct (length of the last stage in percent of the others')
 *   out[4] dp_mode   out[5] all_narrow (no window beyond the narrow tiles')
 *   out[6] contexts alive on the device when the plan was made   out[7] chunks of the call
 *   out[8 .. 8+S]          the S + 1 stage bounds (chunk-relative sites)
 *   out[9+S .. 8+2S]       per stage: 1 when its recurrence ran as k_dp16
 *   out[9+2S .. 8+5S]      tiles per stage and class: [3 * stage + class], classes 0 narrow, 1 wide, 2 medium
 * Returns the 9 + 5 S entries written, WGBSSEG_E_CAPACITY when cap (in entries) is less, WGBSSEG_E_STATE when there is
 * no finished call to report (none yet, or the rows or loci changed since).
 * wgbsseg_debug_sample_terms evaluates the per-(block,sample) term on the device for arrays of (nmeth, ntotal).
 * wgbsseg_debug_log2 evaluates the device arithmetic for `count` consecutive float bit patterns p starting at
 * `first_bits`: out_f = uint32 bits of log2f(p); out_d = uint64 bits of the exact log2(1.0-(double)p) restatement;
 * out_fast = uint64 bits of the bounded-error fast log2 the scoring kernel tries first (any of them may be NULL).
 */
int64_t wgbsseg_debug_fetch(wgbsseg_ctx* ctx, const char* what, void* out, int64_t cap_bytes);
int64_t wgbsseg_debug_last_plan(const wgbsseg_ctx* ctx, int64_t* out, int64_t cap);
int wgbsseg_debug_sample_terms(wgbsseg_ctx* ctx, const float* nmeth, const float* ntotal, int64_t count,
                               float pseudo_count, float* out);
int wgbsseg_debug_log2(wgbsseg_ctx* ctx, uint32_t first_bits, int64_t count, uint32_t* out_f, uint64_t* out_d,
                       uint64_t* out_fast);
/* wgbsseg_debug_div: the scoring kernel's 8-instruction fp32 division core and the compiler's IEEE `/`, both evaluated
 * on the device for `count` operand pairs (uint32 bit patterns out). */
int wgbsseg_debug_div(wgbsseg_ctx* ctx, const float* a, const float* b, int64_t count, uint32_t* out_fast, uint32_t* out_ieee);
/* wgbsseg_debug_check_div: the verdict the library takes once per context and pseudo count before it lets the narrow scoring
 * tiles use the 4-instruction division core (v_rcp_f32, quotient, one residual correction): the number of operand pairs
 * a = fl(nmeth + pc), b = fl(ntotal + 2 pc), 0 <= nmeth <= ntotal <= max_total, whose quotient differs from IEEE `/`
 * (all evaluated on the device).  The library uses the short core only when this is 0 for max_total = 255 * 60. */
int wgbsseg_debug_check_div(wgbsseg_ctx* ctx, float pseudo_count, int32_t max_total, int64_t* mismatches);
/* wgbsseg_debug_div_short: the short core itself on arrays of operands (bit patterns of the quotients). */
int wgbsseg_debug_div_short(wgbsseg_ctx* ctx, const float* a, const float* b, int64_t count, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* WGBSSEG_H */
