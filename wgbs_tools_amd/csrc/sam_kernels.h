// sam_kernels.h — `wgbstools bam2pat` on gfx950: SAM text in, the records of the view engine out (view_kernels.h sorts, collapses, writes
// and deflates them as it does the reads of a pat file).  Every rule is sam_core.h's; the host side is sam_plan.h and pat_engines.h.
//
// Mapping: one thread per LINE OF THE CHUNK, not per line of a tile.  A SAM line is 300-400 bytes, so a 4 KB tile holds about a dozen:
// with k_pat_count's shape (a workgroup per tile, a thread per line of it) 240 of 256 threads would have no line.  Here the lines of the
// chunk are indexed first — k_sam_count / k_sam_starts, the only kernels that see tiles, find the line starts with pat_kernels.h's staging
// — and every kernel behind them runs one thread per index entry, 256 lines to a workgroup, reading its line's first ten fields from global
// memory (a thread walks its own bytes one after the other: every fetched cache line serves the next 60-odd loads of the same lane).
//
// Per fed chunk:
//   k_sam_count      lines that begin in every 4 KB tile                       -> (k_bed_scan) -> L, which goes home: the grids below are L's
//   k_sam_starts     the first byte of line l, for every l
//   k_sam_eval       a line -> its wg_sam_read (state, chromosome, QNAME length, first site and length of its single-read pat); how many
//                    lines of the workgroup keep their place among the mates (invalid, empty, pat); the counters
//   (k_bed_scan)  k_sam_compact   the kept lines' numbers, in order: part[0, P)
//   k_sam_heads      kept line k begins a run when its QNAME or chromosome differs from kept line k - 1's; line 0 asks the carry, which
//                    says where in its run the chunk begins (shift0).  A single-end file: every line is a run.
//   (k_bed_scan)  k_sam_runs      the run of every kept line and the first kept line of every run: place = k - start[run] (+ shift0)
//   k_sam_measure    every even place is a job: the line alone, or merged with the odd place behind it; kept line 0 at an odd place is
//                    the mate of the carried line.  What the job leaves (wg_sam_res) and its bytes in the arena; the counters
//   (k_bed_scan) x 2 the first record and arena byte of every workgroup; the totals go home, the host makes room (the only way to
//                    bound a pat is to walk it: D and N operations give sites without text)
//   k_sam_pack       the records and their bytes (the chromosome's name, the pat), the cleared count of a carried line that found its
//                    mate, the carry for the next chunk
// No thread's work grows with the NUMBER of lines: the unmapped tail — millions of filtered lines — is dropped by the compaction, a long
// run of one name is cut into pairs by arithmetic on its place.  A thread does walk its own line and the sites under it.
// Plain C++ only.
#pragma once
#include "view_kernels.h"
#include "sam_core.h"
#include "sam_plan.h"

static_assert(WG_SAM_BLOCK == WG_BLOCK, "wg_view_block_incl_u64 scans a workgroup of WG_BLOCK threads");

struct wg_sam_args {
    const char* text;
    int64_t n;
    wg_bb_chroms chroms;
    const uint32_t* loci;
    wg_sam_params par;
};

// what a job leaves: measured once, packed from it
struct wg_sam_res {
    int64_t rs;
    uint32_t len;
    uint16_t first;                    // merged: the span's byte that becomes the pat's first
    uint8_t flags;                     // 1: a record | 2: its count is 1 (else 0: a carried single below --min_cpg) | 4: the carried record's count is cleared
    uint8_t src;                       // 0: line a as it is | 1: line b as it is | 2: merged
};
static_assert(sizeof(wg_sam_res) == 16 && sizeof(wg_sam_read) == 24 && sizeof(wg_sam_carry) == 288, "the tables the host sizes");

#define WG_SAM_JOB_NONE 0
#define WG_SAM_JOB_SINGLE 1
#define WG_SAM_JOB_PAIR 2
#define WG_SAM_JOB_CARRY 3             // the carried line and kept line 0

struct wg_sam_job {
    int kind;
    uint32_t a, b;                     // lines (CARRY: b only)
    uint32_t place;
};

__global__ __launch_bounds__(WG_BLOCK) void k_sam_count(const char* __restrict__ text, int64_t n, uint64_t* __restrict__ tile_lines)
{
    __shared__ PatTile tile;
    const uint32_t total = wg_pat_tile_lines(text, n, (int64_t)blockIdx.x * WG_PAT_TILE, tile);
    if (threadIdx.x == 0) tile_lines[blockIdx.x] = total;
}

__global__ __launch_bounds__(WG_BLOCK) void k_sam_starts(const char* __restrict__ text, int64_t n, const uint64_t* __restrict__ tile_base, uint32_t* __restrict__ lstart)
{
    __shared__ PatTile tile;
    const int64_t base = (int64_t)blockIdx.x * WG_PAT_TILE;
    const uint32_t total = wg_pat_tile_lines(text, n, base, tile);
    const uint64_t at = tile_base[blockIdx.x];
    for (uint32_t l = threadIdx.x; l < total; l += WG_BLOCK) lstart[at + l] = (uint32_t)(base + tile.lstart[l]);
}

// the workgroup's sum of v added to *dst (one atomic per workgroup; integer: no order shows)
__device__ __forceinline__ void wg_sam_count_add(int64_t v, uint64_t* sh, unsigned long long* dst)
{
    uint64_t all;
    (void)wg_view_block_incl_u64((uint64_t)v, sh, all);
    if (threadIdx.x == 0 && all) atomicAdd(dst, (unsigned long long)all);
}

__global__ __launch_bounds__(WG_BLOCK) void k_sam_eval(wg_sam_args a, const uint32_t* __restrict__ lstart, int64_t L, wg_sam_read* __restrict__ reads,
                                                       uint64_t* __restrict__ wg_part, unsigned long long* cnt)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t l = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    int state = 0;
    if (l < L) {
        const wg_sam_text T = {a.text};
        const wg_sam_read r = wg_sam_eval(T, (int64_t)lstart[l], a.n, a.par, a.chroms, a.loci);
        reads[l] = r;
        state = r.state;
    }
    uint64_t kept;
    (void)wg_view_block_incl_u64(wg_sam_participates(state) ? 1u : 0u, sh, kept);
    if (threadIdx.x == 0) wg_part[blockIdx.x] = kept;
    wg_sam_count_add(state == WG_SAM_HEADER, sh, cnt + WG_SAM_N_HEADER);
    wg_sam_count_add(state == WG_SAM_FILTERED, sh, cnt + WG_SAM_N_FILTERED);
    wg_sam_count_add(state == WG_SAM_INVALID, sh, cnt + WG_SAM_N_INVALID);
    wg_sam_count_add(state == WG_SAM_UNKNOWN, sh, cnt + WG_SAM_N_UNKNOWN);
    wg_sam_count_add(state == WG_SAM_EMPTY, sh, cnt + WG_SAM_N_EMPTY);
}

__global__ __launch_bounds__(WG_BLOCK) void k_sam_compact(const wg_sam_read* __restrict__ reads, int64_t L, const uint64_t* __restrict__ part_base, uint32_t* __restrict__ part)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t l = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    const bool keep = l < L && wg_sam_participates(reads[l].state);
    uint64_t all;
    const uint64_t incl = wg_view_block_incl_u64(keep ? 1u : 0u, sh, all);
    if (keep) part[part_base[blockIdx.x] + incl - 1] = (uint32_t)l;
}

// n_part: the total of the kept lines (k_bed_scan's totals[0]); the grid covers L lines, which is no fewer
__global__ __launch_bounds__(WG_BLOCK) void k_sam_heads(wg_sam_args a, const wg_sam_read* __restrict__ reads, const uint32_t* __restrict__ part, const uint64_t* __restrict__ n_part,
                                                        const wg_sam_carry* __restrict__ carry, uint8_t* __restrict__ head, uint64_t* __restrict__ wg_heads, uint32_t* shift0)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t k = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x, P = (int64_t)*n_part;
    uint64_t h = 0;
    if (k < P) {
        const wg_sam_text T = {a.text};
        const wg_sam_read r = reads[part[k]];
        if (k == 0) {
            h = 1;
            const wg_sam_text C = {carry->qname};
            *shift0 = a.par.paired && carry->has && wg_sam_same_read(C, 0, carry->qlen, carry->rank, T, r.line, r.qlen, r.rank) ? carry->place + 1u : 0u;
        } else if (!a.par.paired) h = 1;
        else {
            const wg_sam_read q = reads[part[k - 1]];
            h = wg_sam_same_read(T, q.line, q.qlen, q.rank, T, r.line, r.qlen, r.rank) ? 0u : 1u;
        }
        head[k] = (uint8_t)h;
    }
    uint64_t all;
    (void)wg_view_block_incl_u64(h, sh, all);
    if (threadIdx.x == 0) wg_heads[blockIdx.x] = all;
}

__global__ __launch_bounds__(WG_BLOCK) void k_sam_runs(const uint8_t* __restrict__ head, const uint64_t* __restrict__ head_base, const uint64_t* __restrict__ n_part,
                                                       uint32_t* __restrict__ rid, uint32_t* __restrict__ run_start)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t k = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x, P = (int64_t)*n_part;
    const uint64_t h = k < P ? head[k] : 0u;
    uint64_t all;
    const uint64_t run = head_base[blockIdx.x] + wg_view_block_incl_u64(h, sh, all) - 1;
    if (k < P) {
        rid[k] = (uint32_t)run;
        if (h) run_start[run] = (uint32_t)k;
    }
}

__device__ __forceinline__ wg_sam_job wg_sam_job_of(int64_t k, int64_t P, const uint32_t* __restrict__ part, const uint32_t* __restrict__ rid,
                                                    const uint32_t* __restrict__ run_start, uint32_t shift0)
{
    const uint32_t r = rid[k];
    wg_sam_job j = {WG_SAM_JOB_NONE, part[k], part[k], (uint32_t)(k - run_start[r]) + (r == 0 ? shift0 : 0u)};
    if (!wg_sam_is_first(j.place)) { if (k == 0) j.kind = WG_SAM_JOB_CARRY; }      // (any other odd place: the job of the line in front)
    else if (k + 1 < P && rid[k + 1] == r) { j.kind = WG_SAM_JOB_PAIR; j.b = part[k + 1]; }
    else j.kind = WG_SAM_JOB_SINGLE;
    return j;
}

// the pat of the line `r` as wg_sam_merge reads it
__device__ __forceinline__ wg_sam_pat_of_line<wg_sam_text> wg_sam_pat_of(const wg_sam_args& a, const wg_sam_text& T, const wg_sam_read& r)
{
    return wg_sam_pat_begin(T, wg_sam_geom_again(T, (int64_t)r.line, a.n, r.bottom != 0), a.loci, r.start - 1, (int64_t)a.par.clip);
}

// a result that is one line's pat as it is
__device__ __forceinline__ wg_sam_res wg_sam_res_single(const wg_sam_read& r, uint8_t src, bool provisional, int32_t min_cpg, int64_t& n_short)
{
    wg_sam_res o = {r.start, r.plen, 0, 0, src};
    const bool enough = (int64_t)r.plen >= (int64_t)min_cpg;
    if (enough) o.flags = 3;
    else { n_short++; if (provisional) o.flags = 1; }
    return o;
}

__device__ __forceinline__ wg_sam_res wg_sam_res_merged(const wg_sam_merged& m, int32_t min_cpg, int64_t& n_short, int64_t& n_long, int64_t& n_empty)
{
    wg_sam_res o = {m.rs, (uint32_t)m.len, (uint16_t)m.first, 0, 2};
    if (m.why == WG_SAM_MERGE_TOO_LONG) n_long++;
    else if (m.why == WG_SAM_MERGE_EMPTY) n_empty++;
    else if (m.len >= (int64_t)min_cpg) o.flags = 3;
    else n_short++;
    return o;
}

// the carried single's pat: the bytes of its record
__device__ __forceinline__ wg_sam_pat_of_bytes wg_sam_pat_of_carry(const wg_sam_carry& c, const wg_view_rec* __restrict__ recs, const char* __restrict__ arena)
{
    const wg_view_rec rec = recs[c.rec];
    return {arena + rec.off + rec.clen};
}

__global__ __launch_bounds__(WG_BLOCK) void k_sam_measure(wg_sam_args a, const wg_sam_read* __restrict__ reads, const uint32_t* __restrict__ part, const uint64_t* __restrict__ n_part,
                                                          const uint32_t* __restrict__ rid, const uint32_t* __restrict__ run_start, const uint32_t* shift0,
                                                          const wg_sam_carry* __restrict__ carry, const wg_view_rec* __restrict__ recs, const char* __restrict__ arena,
                                                          wg_sam_res* __restrict__ res, uint64_t* __restrict__ wg_recs, uint64_t* __restrict__ wg_bytes, unsigned long long* cnt)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t k = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x, P = (int64_t)*n_part;
    int64_t n_short = 0, n_long = 0, n_empty = 0, n_pairs = 0, n_single = 0;
    wg_sam_res o = {0, 0, 0, 0, 0};
    uint64_t bytes = 0;
    if (k < P) {
        const wg_sam_text T = {a.text};
        const wg_sam_job j = wg_sam_job_of(k, P, part, rid, run_start, *shift0);
        const int32_t min_cpg = a.par.min_cpg;
        const auto nothing = [](int64_t, char) {};
        if (j.kind == WG_SAM_JOB_SINGLE) {
            const wg_sam_read ra = reads[j.a];
            if (a.par.paired) n_single++;
            if (ra.state == WG_SAM_PAT) o = wg_sam_res_single(ra, 0, a.par.paired && k == P - 1, min_cpg, n_short);
        } else if (j.kind == WG_SAM_JOB_PAIR) {
            const wg_sam_read ra = reads[j.a], rb = reads[j.b];
            n_pairs++;
            if (ra.state == WG_SAM_PAT && rb.state == WG_SAM_PAT)
                o = wg_sam_res_merged(wg_sam_merge(ra.start, ra.plen, wg_sam_pat_of(a, T, ra), rb.start, rb.plen, wg_sam_pat_of(a, T, rb), nothing), min_cpg, n_short, n_long, n_empty);
            else if (ra.state == WG_SAM_PAT) o = wg_sam_res_single(ra, 0, false, min_cpg, n_short);
            else if (rb.state == WG_SAM_PAT) o = wg_sam_res_single(rb, 1, false, min_cpg, n_short);
        } else if (j.kind == WG_SAM_JOB_CARRY) {                    // the chunk before counted the carried line as left single
            const wg_sam_carry c = *carry;
            const wg_sam_read rb = reads[j.b];
            n_pairs++; n_single--;
            if (c.state == WG_SAM_PAT && rb.state == WG_SAM_PAT) {
                if ((int64_t)c.plen < (int64_t)min_cpg) n_short--;      // ... and as short, when it was
                o = wg_sam_res_merged(wg_sam_merge(c.start, c.plen, wg_sam_pat_of_carry(c, recs, arena), rb.start, rb.plen, wg_sam_pat_of(a, T, rb), nothing), min_cpg, n_short, n_long, n_empty);
                o.flags |= 4;
            } else if (rb.state == WG_SAM_PAT) o = wg_sam_res_single(rb, 1, false, min_cpg, n_short);
        }
        res[k] = o;
        if (o.flags & 1) bytes = (uint64_t)(a.chroms.off[reads[j.b].rank + 1] - a.chroms.off[reads[j.b].rank]) + o.len;
    }
    uint64_t rr, bb;
    (void)wg_view_block_incl_u64(o.flags & 1, sh, rr);
    (void)wg_view_block_incl_u64(bytes, sh, bb);
    if (threadIdx.x == 0) { wg_recs[blockIdx.x] = rr; wg_bytes[blockIdx.x] = bb; }
    wg_sam_count_add(n_short, sh, cnt + WG_SAM_N_SHORT);
    wg_sam_count_add(n_pairs, sh, cnt + WG_SAM_N_PAIRS);
    wg_sam_count_add(n_single, sh, cnt + WG_SAM_N_LEFT_SINGLE);
    wg_sam_count_add(n_long, sh, cnt + WG_SAM_N_TOO_LONG);
    wg_sam_count_add(n_empty, sh, cnt + WG_SAM_N_EMPTY);
}

// rec_base / byte_base: the scans of k_sam_measure's totals; rec0 / arena0: what the chunks before left in the two buffers
__global__ __launch_bounds__(WG_BLOCK) void k_sam_pack(wg_sam_args a, const wg_sam_read* __restrict__ reads, const uint32_t* __restrict__ part, const uint64_t* __restrict__ n_part,
                                                       const uint32_t* __restrict__ rid, const uint32_t* __restrict__ run_start, const uint32_t* shift0,
                                                       const wg_sam_carry* __restrict__ carry, wg_sam_carry* __restrict__ carry_out, const wg_sam_res* __restrict__ res,
                                                       const uint64_t* __restrict__ rec_base, const uint64_t* __restrict__ byte_base, uint64_t rec0, uint64_t arena0,
                                                       wg_view_rec* __restrict__ recs, char* __restrict__ arena)
{
    __shared__ uint64_t sh[WG_BLOCK / 64];
    const int64_t k = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x, P = (int64_t)*n_part;
    const wg_sam_text T = {a.text};
    wg_sam_res o = {0, 0, 0, 0, 0};
    wg_sam_job j = {WG_SAM_JOB_NONE, 0, 0, 0};
    uint32_t clen = 0;
    int32_t rank = 0;
    if (k < P) {
        o = res[k];
        j = wg_sam_job_of(k, P, part, rid, run_start, *shift0);
        rank = reads[j.b].rank;
        clen = a.chroms.off[rank + 1] - a.chroms.off[rank];
    }
    const bool keep = (o.flags & 1) != 0;
    const uint64_t mine = keep ? (uint64_t)clen + o.len : 0u;
    uint64_t rr, bb;
    const uint64_t ir = wg_view_block_incl_u64(keep ? 1u : 0u, sh, rr);
    const uint64_t ib = wg_view_block_incl_u64(mine, sh, bb);
    const uint64_t r_at = rec0 + rec_base[blockIdx.x] + ir - 1;
    if (keep) {
        wg_view_rec r;
        r.off = arena0 + byte_base[blockIdx.x] + ib - mine;
        r.rs = o.rs;
        r.count = (o.flags & 2) ? 1 : 0;
        r.clen = clen;
        r.plen = o.len;
        r.line = 0;
        recs[r_at] = r;
        char* dst = arena + r.off;
        const char* name = a.chroms.arena + a.chroms.off[rank];
        for (uint32_t i = 0; i < clen; i++) dst[i] = name[i];
        dst += clen;
        if (o.src != 2) {
            const wg_sam_read rl = reads[o.src ? j.b : j.a];
            wg_sam_pat_of_line<wg_sam_text> pat = wg_sam_pat_of(a, T, rl);
            for (uint32_t i = 0; i < o.len; i++) dst[i] = pat((int64_t)i);
        } else {
            const int64_t first = o.first, len = o.len;
            const auto put = [&](int64_t i, char c) { if (i >= first && i < first + len) dst[i - first] = c; };
            const wg_sam_read rb = reads[j.b];
            if (j.kind == WG_SAM_JOB_CARRY) {
                const wg_sam_carry c = *carry;
                (void)wg_sam_merge(c.start, c.plen, wg_sam_pat_of_carry(c, recs, arena), rb.start, rb.plen, wg_sam_pat_of(a, T, rb), put);
            } else {
                const wg_sam_read ra = reads[j.a];
                (void)wg_sam_merge(ra.start, ra.plen, wg_sam_pat_of(a, T, ra), rb.start, rb.plen, wg_sam_pat_of(a, T, rb), put);
            }
        }
    }
    if (k < P && (o.flags & 4)) recs[carry->rec].count = 0;         // the carried single found its mate: the merged read (or nothing) stands for both
    if (k < P && k == P - 1) {                                      // the last kept line: what the next chunk's first may be the mate of
        const wg_sam_read rl = reads[part[k]];
        wg_sam_carry c;
        c.rec = j.kind == WG_SAM_JOB_SINGLE && keep ? (int64_t)r_at : -1;
        c.start = rl.start; c.plen = rl.plen; c.rank = rl.rank; c.place = j.place; c.qlen = rl.qlen; c.state = rl.state; c.has = 1;
        carry_out->rec = c.rec; carry_out->start = c.start; carry_out->plen = c.plen; carry_out->rank = c.rank; carry_out->place = c.place;
        carry_out->qlen = c.qlen; carry_out->state = c.state; carry_out->has = 1;
        if (rl.qlen <= WG_SAM_MAX_QNAME)
            for (uint32_t i = 0; i < rl.qlen; i++) carry_out->qname[i] = T.at((int64_t)rl.line + i);
    }
}
