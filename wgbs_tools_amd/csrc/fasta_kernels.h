// fasta_kernels.h — `wgbstools init_genome` on gfx950: FASTA text in, the sequence table and the loci of every CpG out, then the CpG
// dictionary's text.  Every rule is fasta_core.h's; the host side is fasta_plan.h and pat_engines.h (wgbsseg_fasta).
//
// A chunk of text may be cut at ANY byte, so nothing here knows lines: a tile is 4 KB of text, a workgroup per tile, 16 bytes per thread,
// and what a stretch of text does to the walk that enters it — the state it leaves for each of the four states it may be entered in, and
// for each of them the headers, the bases before the first and behind the last header, the sites — composes left to right
// (wg_fa_map_then, wg_fa_sum_then).  Per fed chunk, separate kernels in stream order (no workgroup waits for another):
//
//   k_fa_settle   one thread: a C the chunk before left pending (its next base lay behind the chunk's end) meets its next base
//   k_fa_measure  every thread walks its 16 bytes once per entry state; the workgroup composes the 256 results into the tile's summary
//   k_fa_scan     ONE workgroup, a run of consecutive tiles per thread, seeded with the carry: where the walk stands at every tile's first
//                 byte (wg_fa_entry), the carry of the next chunk, the totals (sequences, sites) that go home: the host makes room
//   k_fa_pack     the scan inside the tile again, then every thread walks its bytes from where the walk really stands: a site's locus to
//                 its place in FASTA order; per header the record (offset, first site, the finished base count of the sequence before)
//                 by the thread that holds the '>', every byte of the name by the thread that holds it, the length by the one that
//                 holds the byte behind the name; refusals by one 64-bit atomicMin of (offset << 8 | reason)
// To decide a C a thread reads on past '\r' and '\n' to the next base, into the tiles behind if need be; a C whose next base lies
// behind the chunk is left to the carry.
//
// finish: k_dict_len -> k_bed_scan -> k_dict_emit write `name \t locus \t site \n` for the selected sites, the chromosome of a site from
// the cumulative table (as k_bed_emit finds it), digits by bed_fmt.h.  Plain C++ only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bed_kernels.h"
#include "fasta_core.h"
#include "fasta_plan.h"

static_assert(WG_FA_DICT_BLOCK == WG_BED_BLOCK, "wg_bed_block_scan scans a workgroup of WG_BED_BLOCK threads");

struct wg_fa_tile {                    // a tile's summary: per entry state its counts, and the map of the states
    wg_fa_sum e[4];
    uint32_t map;
};

struct wg_fa_entry {                   // where the walk stands at a tile's first byte
    uint64_t seqs, bases, hits, hdr_off;
    uint32_t state, pad;
};

struct wg_fa_carry {                   // ... and at the end of the chunks so far
    uint64_t seqs, bases, hits, hdr_off;
    uint32_t state;
    uint32_t pend;                     // the last base was a C: its next base decides
    uint64_t pend_locus;
};
static_assert(sizeof(wg_fa_tile) == 84 && sizeof(wg_fa_entry) == 40 && sizeof(wg_fa_carry) == 48, "the tables the host sizes");

// a tile in LDS in front of the chunk's text: bytes of the tile come from LDS, what a look ahead needs behind it from global memory
struct wg_fa_tile_text {
    const char* lds;
    const char* text;
    int64_t base;
    __device__ __forceinline__ char at(int64_t p) const
    {
        const int64_t r = p - base;
        return r >= 0 && r < WG_FA_TILE ? lds[r] : text[p];
    }
};

struct wg_fa_plain_text {
    const char* p;
    __host__ __device__ __forceinline__ char at(int64_t i) const { return p[i]; }
};

// the tile at `base` into LDS (16 bytes per thread; the chunk's buffer begins at a multiple of 16 and so does every tile).  Ends in a barrier.
__device__ __forceinline__ void wg_fa_load_tile(const char* __restrict__ text, int64_t n, int64_t base, char* lds)
{
    const int64_t at = base + (int64_t)threadIdx.x * WG_FA_THREAD_BYTES;
    if (at + WG_FA_THREAD_BYTES <= n)
        *reinterpret_cast<uint4*>(lds + threadIdx.x * WG_FA_THREAD_BYTES) = *reinterpret_cast<const uint4*>(text + at);
    else
        for (int j = 0; j < WG_FA_THREAD_BYTES; j++) lds[threadIdx.x * WG_FA_THREAD_BYTES + j] = at + j < n ? text[at + j] : '\n';
    __syncthreads();
}

// Inclusive scan of v over the workgroup's threads in thread order by the associative `then`; buf: 2 x WG_FA_BLOCK.  *before: the
// scan of the threads in front (id for thread 0), *all: the whole workgroup's.  Ends in a barrier: buf may be used again.
template <class T, class Then>
__device__ __forceinline__ void wg_fa_block_scan(T v, T* buf, const T& id, Then then, T* before, T* all)
{
    const int t = threadIdx.x;
    int cur = 0;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < WG_FA_BLOCK; d <<= 1, cur ^= 1) {
        T x = buf[cur * WG_FA_BLOCK + t];
        if (t >= d) x = then(buf[cur * WG_FA_BLOCK + t - d], x);
        buf[(cur ^ 1) * WG_FA_BLOCK + t] = x;
        __syncthreads();
    }
    *before = t ? buf[cur * WG_FA_BLOCK + t - 1] : id;
    *all = buf[cur * WG_FA_BLOCK + WG_FA_BLOCK - 1];
    __syncthreads();
}

struct wg_fa_map_op { __device__ __forceinline__ uint32_t operator()(uint32_t a, uint32_t b) const { return wg_fa_map_then(a, b); } };
struct wg_fa_sum_op { __device__ __forceinline__ wg_fa_sum operator()(const wg_fa_sum& a, const wg_fa_sum& b) const { return wg_fa_sum_then(a, b); } };
struct wg_fa_sum64_op { __device__ __forceinline__ wg_fa_sum64 operator()(const wg_fa_sum64& a, const wg_fa_sum64& b) const { return wg_fa_sum_then(a, b); } };

// the state text[p0, p1) leaves for each entry state (no counts, no look ahead)
template <class Text>
__device__ __forceinline__ uint32_t wg_fa_map_of(const Text& T, int64_t p0, int64_t p1)
{
    uint32_t s0 = WG_FA_LS, s1 = WG_FA_SQ, s2 = WG_FA_NM, s3 = WG_FA_HD;
    for (int64_t p = p0; p < p1; p++) {
        const uint8_t b = (uint8_t)T.at(p);
        int ev;
        s0 = (uint32_t)wg_fa_step((int)s0, b, &ev); s1 = (uint32_t)wg_fa_step((int)s1, b, &ev);
        s2 = (uint32_t)wg_fa_step((int)s2, b, &ev); s3 = (uint32_t)wg_fa_step((int)s3, b, &ev);
    }
    return s0 | (s1 << 2) | (s2 << 4) | (s3 << 6);
}

__global__ void k_fa_settle(const char* __restrict__ text, int64_t n, wg_fa_carry* carry, uint32_t* __restrict__ loci)
{
    if (threadIdx.x || blockIdx.x || !carry->pend) return;
    const wg_fa_plain_text T = {text};
    const int g = wg_fa_next_is_g(T, n, 0, carry->state == WG_FA_LS);
    if (g < 0) return;                                             // (a chunk of line breaks: the next one decides)
    if (g > 0) { loci[carry->hits] = (uint32_t)carry->pend_locus; carry->hits += 1; }
    carry->pend = 0;
}

__global__ __launch_bounds__(WG_FA_BLOCK) void k_fa_measure(const char* __restrict__ text, int64_t n, wg_fa_tile* __restrict__ tiles)
{
    __shared__ __attribute__((aligned(16))) char lds[WG_FA_TILE];
    __shared__ uint32_t maps[2 * WG_FA_BLOCK];
    __shared__ wg_fa_sum sums[4][WG_FA_BLOCK];
    const int64_t base = (int64_t)blockIdx.x * WG_FA_TILE;
    wg_fa_load_tile(text, n, base, lds);
    const wg_fa_tile_text T = {lds, text, base};
    const int64_t p0 = base + (int64_t)threadIdx.x * WG_FA_THREAD_BYTES, p1 = p0 + WG_FA_THREAD_BYTES < n ? p0 + WG_FA_THREAD_BYTES : n;
    wg_fa_sum mine[4];
    uint32_t map = 0;
#pragma unroll
    for (uint32_t s = 0; s < 4; s++) {
        uint32_t leaves = s;
        mine[s] = wg_fa_count(T, n, p0, p1, base, s, &leaves);
        map |= leaves << (2 * s);
    }
    uint32_t before, all;
    wg_fa_block_scan(map, maps, WG_FA_MAP_ID, wg_fa_map_op(), &before, &all);
#pragma unroll
    for (uint32_t e = 0; e < 4; e++) {                             // the tile entered in e: this thread is entered in before(e)
        const uint32_t s = wg_fa_map_at(before, e);
        sums[e][threadIdx.x] = s == 0 ? mine[0] : s == 1 ? mine[1] : s == 2 ? mine[2] : mine[3];
    }
    __syncthreads();
    for (int d = 1; d < WG_FA_BLOCK; d <<= 1) {                    // neighbours join in order: then() does not commute
        if ((threadIdx.x & (2 * d - 1)) == 0)
            for (int e = 0; e < 4; e++) sums[e][threadIdx.x] = wg_fa_sum_then(sums[e][threadIdx.x], sums[e][threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x < 4) tiles[blockIdx.x].e[threadIdx.x] = sums[threadIdx.x][0];
    if (threadIdx.x == 0) tiles[blockIdx.x].map = all;
}

// tile i's counts when it is entered in s, its `last` as an offset of the input
__device__ __forceinline__ wg_fa_sum64 wg_fa_tile_sum(const wg_fa_tile* __restrict__ tiles, int64_t i, uint32_t s, uint64_t abs0)
{
    const wg_fa_sum a = tiles[i].e[s];
    return {a.h, a.pre, a.post, a.hits, abs0 + (uint64_t)i * WG_FA_TILE + a.last};
}

// totals: the sequences and the sites of the input so far
__global__ __launch_bounds__(WG_FA_SCAN_BLOCK) void k_fa_scan(const wg_fa_tile* __restrict__ tiles, int64_t n_tiles, uint64_t abs0, wg_fa_carry* carry,
                                                              wg_fa_entry* __restrict__ entries, uint64_t* __restrict__ totals)
{
    __shared__ uint32_t maps[2 * WG_FA_SCAN_BLOCK];
    __shared__ wg_fa_sum64 sums[2 * WG_FA_SCAN_BLOCK];
    static_assert(WG_FA_SCAN_BLOCK == WG_FA_BLOCK, "wg_fa_block_scan scans WG_FA_BLOCK threads");
    const wg_fa_carry in = *carry;
    const int64_t per = (n_tiles + WG_FA_SCAN_BLOCK - 1) / WG_FA_SCAN_BLOCK;
    const int64_t t0 = (int64_t)threadIdx.x * per < n_tiles ? (int64_t)threadIdx.x * per : n_tiles, t1 = t0 + per < n_tiles ? t0 + per : n_tiles;
    uint32_t map = WG_FA_MAP_ID;
    for (int64_t i = t0; i < t1; i++) map = wg_fa_map_then(map, tiles[i].map);
    uint32_t before, all;
    wg_fa_block_scan(map, maps, WG_FA_MAP_ID, wg_fa_map_op(), &before, &all);
    const uint32_t s0 = wg_fa_map_at(before, in.state);
    const wg_fa_sum64 none = {0, 0, 0, 0, 0};
    wg_fa_sum64 mine = none;
    uint32_t s = s0;
    for (int64_t i = t0; i < t1; i++) {
        mine = wg_fa_sum_then(mine, wg_fa_tile_sum(tiles, i, s, abs0));
        s = wg_fa_map_at(tiles[i].map, s);
    }
    wg_fa_sum64 front, whole;
    wg_fa_block_scan(mine, sums, none, wg_fa_sum64_op(), &front, &whole);
    wg_fa_cur c = {in.seqs, in.bases, in.hits, in.hdr_off, 0};
    wg_fa_cur_then(c, front);
    s = s0;
    for (int64_t i = t0; i < t1; i++) {
        entries[i] = {c.seqs, c.bases, c.hits, c.hdr_off, s, 0};
        wg_fa_cur_then(c, wg_fa_tile_sum(tiles, i, s, abs0));
        s = wg_fa_map_at(tiles[i].map, s);
    }
    if (threadIdx.x == 0) {                                        // (every thread has read the carry: the scans above end in barriers)
        wg_fa_cur e = {in.seqs, in.bases, in.hits, in.hdr_off, 0};
        wg_fa_cur_then(e, whole);
        carry->seqs = e.seqs; carry->bases = e.bases; carry->hits = e.hits; carry->hdr_off = e.hdr_off;
        carry->state = wg_fa_map_at(all, in.state);
        totals[0] = e.seqs; totals[1] = e.hits;
    }
}

// what k_fa_pack's walk leaves
struct wg_fa_pack_sink {
    wg_fa_seq* seqs;
    uint32_t* loci;
    unsigned long long* bad;
    wg_fa_carry* carry;
    __device__ __forceinline__ void header(const wg_fa_cur& c, uint64_t at)
    {
        wg_fa_seq* r = seqs + c.seqs;
        r->hdr_off = at; r->first_locus = c.hits; r->prev_bases = (uint32_t)c.bases;
    }
    __device__ __forceinline__ void name_byte(uint64_t seq, uint32_t idx, char b) { seqs[seq].name[idx] = b; }
    __device__ __forceinline__ void name_end(uint64_t seq, uint64_t len) { seqs[seq].name_len = len > WG_FA_MAX_NAME ? WG_FA_MAX_NAME + 1u : (uint32_t)len; }
    __device__ __forceinline__ void hit(uint64_t index, uint64_t locus) { loci[index] = (uint32_t)locus; }
    __device__ __forceinline__ void pending(uint64_t locus) { carry->pend_locus = locus; carry->pend = 1; }
    __device__ __forceinline__ void refuse(uint64_t at, int why) { atomicMin(bad, (unsigned long long)((at << 8) | (uint64_t)why)); }
};

__global__ __launch_bounds__(WG_FA_BLOCK) void k_fa_pack(const char* __restrict__ text, int64_t n, uint64_t abs0, const wg_fa_entry* __restrict__ entries,
                                                         wg_fa_seq* __restrict__ seqs, uint32_t* __restrict__ loci, unsigned long long* bad, wg_fa_carry* carry)
{
    __shared__ __attribute__((aligned(16))) char lds[WG_FA_TILE];
    __shared__ uint32_t maps[2 * WG_FA_BLOCK];
    __shared__ wg_fa_sum sums[2 * WG_FA_BLOCK];
    const int64_t base = (int64_t)blockIdx.x * WG_FA_TILE;
    wg_fa_load_tile(text, n, base, lds);
    const wg_fa_tile_text T = {lds, text, base};
    const wg_fa_entry in = entries[blockIdx.x];
    const int64_t p0 = base + (int64_t)threadIdx.x * WG_FA_THREAD_BYTES, p1 = p0 + WG_FA_THREAD_BYTES < n ? p0 + WG_FA_THREAD_BYTES : n;
    uint32_t before, all;
    wg_fa_block_scan(p0 < p1 ? wg_fa_map_of(T, p0, p1) : WG_FA_MAP_ID, maps, WG_FA_MAP_ID, wg_fa_map_op(), &before, &all);
    const uint32_t s0 = wg_fa_map_at(before, in.state);
    uint32_t leaves;
    const wg_fa_sum mine = wg_fa_count(T, n, p0, p1, base, s0, &leaves);
    const wg_fa_sum none = {0, 0, 0, 0, 0};
    wg_fa_sum front, whole;
    wg_fa_block_scan(mine, sums, none, wg_fa_sum_op(), &front, &whole);
    wg_fa_cur c = {in.seqs, in.bases, in.hits, in.hdr_off, s0};
    wg_fa_cur_then(c, wg_fa_sum64{front.h, front.pre, front.post, front.hits, abs0 + (uint64_t)base + front.last});
    wg_fa_pack_sink k = {seqs, loci, bad, carry};
    wg_fa_walk(T, n, p0, p1, abs0, c, k);
}

// --- the dictionary's text ------------------------------------------------------------------------------------------------------------

struct wg_dict_args {
    const uint32_t* loci;              // the selected sites' loci, in dictionary order
    const int64_t* cum;                // cumulative site counts of the kept chromosomes
    const char* names;                 // WG_FA_MAX_NAME + 1 bytes per chromosome
    const uint32_t* name_len;
    int64_t n;
    int32_t n_chroms;
};

struct wg_dict_site {
    uint32_t len, loc;
    int32_t chrom, name_len;
};

__device__ __forceinline__ wg_dict_site wg_dict_read(const wg_dict_args& a, int64_t i)
{
    wg_dict_site s = {0, 0, 0, 0};
    if (i >= a.n) return s;
    s.loc = a.loci[i];
    int lo = 0, hi = a.n_chroms - 1;                               // the first chromosome with cum > i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.cum[mid] > i) hi = mid; else lo = mid + 1;
    }
    s.chrom = lo;
    s.name_len = (int32_t)a.name_len[lo];
    s.len = (uint32_t)s.name_len + 1u + (uint32_t)wg_dec_len(s.loc) + 1u + (uint32_t)wg_dec_len((uint64_t)i + 1) + 1u;
    return s;
}

template <class P>
__device__ __forceinline__ void wg_dict_put(const wg_dict_args& a, const wg_dict_site& s, int64_t i, P dst)
{
    const char* name = a.names + (int64_t)s.chrom * (WG_FA_MAX_NAME + 1);
    int p = 0;
    for (; p < s.name_len; p++) dst[p] = name[p];
    dst[p++] = '\t';
    p += wg_dec_put(dst + p, s.loc);
    dst[p++] = '\t';
    p += wg_dec_put(dst + p, (uint64_t)i + 1);
    dst[p] = '\n';
}

__global__ __launch_bounds__(WG_FA_DICT_BLOCK) void k_dict_len(wg_dict_args a, uint64_t* __restrict__ wg_bytes, uint64_t* __restrict__ wg_lines)
{
    __shared__ uint32_t waves_b[WG_FA_DICT_BLOCK / 64], waves_l[WG_FA_DICT_BLOCK / 64];
    const wg_dict_site s = wg_dict_read(a, (int64_t)blockIdx.x * WG_FA_DICT_BLOCK + threadIdx.x);
    uint32_t bytes, lines;
    wg_bed_block_scan(s.len, waves_b, bytes);
    wg_bed_block_scan(s.len ? 1u : 0u, waves_l, lines);
    if (threadIdx.x == 0) { wg_bytes[blockIdx.x] = bytes; wg_lines[blockIdx.x] = lines; }
}

__global__ __launch_bounds__(WG_FA_DICT_BLOCK) void k_dict_emit(wg_dict_args a, const uint64_t* __restrict__ wg_base, char* __restrict__ out)
{
    __shared__ uint32_t waves[WG_FA_DICT_BLOCK / 64];
    __shared__ char stage[WG_FA_DICT_STAGE];
    const int64_t i = (int64_t)blockIdx.x * WG_FA_DICT_BLOCK + threadIdx.x;
    const wg_dict_site s = wg_dict_read(a, i);
    uint32_t total;
    const uint32_t off = wg_bed_block_scan(s.len, waves, total);
    char* g = out + wg_base[blockIdx.x];
    if (total <= WG_FA_DICT_STAGE) {                               // (the same in every thread)
        if (s.len) wg_dict_put(a, s, i, stage + off);
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < total; j += WG_FA_DICT_BLOCK) g[j] = stage[j];
    } else if (s.len)
        wg_dict_put(a, s, i, g + off);
}
