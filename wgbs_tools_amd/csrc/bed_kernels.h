// bed_kernels.h — one resident sample as BED text (`wgbstools beta2bed`, wgbsseg_beta2bed): a line per site, formatted on the
// device.  Two passes over a slab of sites, one site per thread, WG_BED_BLOCK sites per workgroup ("Per-site BED text"):
//
//   k_bed_len    the byte length of every site's output (0 when the line is dropped, length x multiplicity with -L), summed per
//                workgroup: one 64-bit total of bytes and one of lines per workgroup
//   k_bed_scan   ONE workgroup turns the totals into every workgroup's first byte in the slab and the slab's totals
//   k_bed_emit   the lengths again (cheaper than keeping 4 bytes per site), a scan inside the workgroup, then every thread formats
//                its line into LDS at its offset, shifted by the low four bits of the workgroup's first byte, so that an LDS
//                address and its global address agree modulo 16: the copy out is aligned 16-byte LDS reads and aligned 16-byte
//                global stores, with byte stores only in the first and the last vector.  A workgroup whose text does not fit
//                the staging area (bed_plan.h, wg_bed_staged) formats each line into its own LDS slot and writes the copies
//                straight to global memory.
//
// The chromosome of a site is the first entry of the cumulative table above it; table and names sit in LDS when they have at
// most WG_BED_LDS_CHROMS entries (any genome's main assembly), else they are read from global memory.  Plain C++ only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "wave_prims.h"
#include "bed_plan.h"

struct wg_bed_args {
    const uint8_t* row;        // the sample's resident row, from resident site 0
    const uint32_t* loci;      // resident loci
    const uint16_t* mult;      // multiplicity of every site of the slab, or nullptr (all 1)
    const int64_t* cum;        // cumulative site counts of the chromosomes
    const char* names;         // WG_BED_NAME_REC bytes per chromosome: the name, byte 31 its length
    int64_t first;             // the slab's first resident site
    int32_t n;                 // ... and its sites
    int32_t n_chroms, min_cov, mean, keep_na;
    uint32_t stage_bytes;
};

// what a thread knows of its site after reading it
struct wg_bed_site {
    uint32_t len;              // bytes of one copy of its line (0: dropped, or no site)
    uint32_t mult;
    uint32_t loc, meth, cov;
    int32_t chrom, name_len;
    uint64_t g3;               // mean: the ratio's text (bed_fmt.h)
    int32_t g3_len;
};

struct wg_bed_table {
    int64_t cum[WG_BED_LDS_CHROMS];
    char names[WG_BED_LDS_CHROMS * WG_BED_NAME_REC];
};

// The chromosome table in LDS, when it fits; -> where the workgroup reads it from.  Ends in a barrier.
__device__ __forceinline__ void wg_bed_load_table(const wg_bed_args& a, wg_bed_table& t, const int64_t*& cum, const char*& names)
{
    const bool fits = a.n_chroms <= WG_BED_LDS_CHROMS;
    if (fits) {
        for (int i = threadIdx.x; i < a.n_chroms; i += WG_BED_BLOCK) t.cum[i] = a.cum[i];
        for (int i = threadIdx.x; i < a.n_chroms * (WG_BED_NAME_REC / 4); i += WG_BED_BLOCK)
            reinterpret_cast<uint32_t*>(t.names)[i] = reinterpret_cast<const uint32_t*>(a.names)[i];
    }
    __syncthreads();
    cum = fits ? t.cum : a.cum;
    names = fits ? t.names : a.names;
}

template <int ELEM>
__device__ __forceinline__ wg_bed_site wg_bed_read(const wg_bed_args& a, int64_t i, const int64_t* cum, const char* names)
{
    wg_bed_site s = {};
    if (i >= a.n) return s;
    const int64_t site = a.first + i;
    s.loc = a.loci[site];
    if (ELEM == 1) {
        const uint32_t w = reinterpret_cast<const uint16_t*>(a.row)[site];
        s.meth = w & 0xffu; s.cov = w >> 8;
    } else {
        const uint32_t w = reinterpret_cast<const uint32_t*>(a.row)[site];
        s.meth = w & 0xffffu; s.cov = w >> 16;
    }
    s.mult = a.mult ? a.mult[i] : 1u;
    if (a.min_cov > 1 && s.cov < (uint32_t)a.min_cov) s.meth = s.cov = 0;
    if ((!a.keep_na && s.cov == 0) || s.mult == 0) { s.mult = 0; return s; }
    int lo = 0, hi = a.n_chroms - 1;                             // the first chromosome with cum > site
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > site) hi = mid; else lo = mid + 1;
    }
    s.chrom = lo;
    s.name_len = (uint8_t)names[lo * WG_BED_NAME_REC + WG_BED_NAME_REC - 1];
    uint32_t len = (uint32_t)s.name_len + 1;
    len += (s.loc == 0 ? 2 : wg_dec_len((uint64_t)s.loc - 1)) + 1;
    len += wg_dec_len((uint64_t)s.loc + 1) + 1;
    if (a.mean) {
        if (s.cov) s.g3 = wg_fmt_g3(s.meth, s.cov, &s.g3_len);
        else { s.g3 = (uint64_t)'-' | ((uint64_t)'1' << 8); s.g3_len = 2; }
        len += s.g3_len;
    } else {
        len += wg_dec_len(s.meth) + 1 + wg_dec_len(s.cov);
    }
    s.len = len + 1;
    return s;
}

// the site's line at dst (LDS): s.len bytes
__device__ __forceinline__ void wg_bed_put(const wg_bed_args& a, const wg_bed_site& s, const char* names, char* dst)
{
    const char* name = names + s.chrom * WG_BED_NAME_REC;
    int p = 0;
    for (; p < s.name_len; p++) dst[p] = name[p];
    dst[p++] = '\t';
    if (s.loc == 0) { dst[p++] = '-'; dst[p++] = '1'; }
    else p += wg_dec_put(dst + p, (uint64_t)s.loc - 1);
    dst[p++] = '\t';
    p += wg_dec_put(dst + p, (uint64_t)s.loc + 1);
    dst[p++] = '\t';
    if (a.mean) {
        for (int j = 0; j < s.g3_len; j++) dst[p++] = (char)(s.g3 >> (8 * j));
    } else {
        p += wg_dec_put(dst + p, s.meth);
        dst[p++] = '\t';
        p += wg_dec_put(dst + p, s.cov);
    }
    dst[p] = '\n';
}

// Exclusive prefix sum of v over the workgroup and its total.  Every thread calls it; ends in a barrier-safe state for one
// further call with ANOTHER `waves` array.
__device__ __forceinline__ uint32_t wg_bed_block_scan(uint32_t v, uint32_t* waves, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t incl = wg_wave_incl_scan_dpp_u32(v);
    if (lane == 63) waves[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WG_BED_BLOCK / 64; w++) {
        const uint32_t t = waves[w];
        if (w < wave) before += t;
        all += t;
    }
    total = all;
    return before + incl - v;
}

template <int ELEM>
__global__ __launch_bounds__(WG_BED_BLOCK) void k_bed_len(wg_bed_args a, uint64_t* __restrict__ wg_bytes, uint64_t* __restrict__ wg_lines)
{
    __shared__ wg_bed_table tab;
    __shared__ uint32_t waves_b[WG_BED_BLOCK / 64], waves_l[WG_BED_BLOCK / 64];
    const int64_t* cum;
    const char* names;
    wg_bed_load_table(a, tab, cum, names);
    const wg_bed_site s = wg_bed_read<ELEM>(a, (int64_t)blockIdx.x * WG_BED_BLOCK + threadIdx.x, cum, names);
    uint32_t bytes, lines;
    wg_bed_block_scan(s.len * s.mult, waves_b, bytes);
    wg_bed_block_scan(s.len ? s.mult : 0u, waves_l, lines);
    if (threadIdx.x == 0) { wg_bytes[blockIdx.x] = bytes; wg_lines[blockIdx.x] = lines; }
}

// one workgroup: wg_base[i] = the bytes of the workgroups before i; totals = {bytes, lines} of the slab
__global__ __launch_bounds__(WG_BED_BLOCK) void k_bed_scan(const uint64_t* __restrict__ wg_bytes, const uint64_t* __restrict__ wg_lines, int64_t n,
                                                           uint64_t* __restrict__ wg_base, uint64_t* __restrict__ totals)
{
    __shared__ uint64_t sb[WG_BED_BLOCK / 64], sl[WG_BED_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0, lines = 0;
    for (int64_t at = 0; at < n; at += WG_BED_BLOCK) {
        const int64_t i = at + threadIdx.x;
        const uint64_t v = i < n ? wg_bytes[i] : 0, l = i < n ? wg_lines[i] : 0;
        const uint64_t incl = wg_wave_incl_scan_u64(v, lane), lsum = wg_wave_sum_u64(l);
        if (lane == 63) { sb[wave] = incl; sl[wave] = lsum; }
        __syncthreads();
        uint64_t before = 0, all = 0, lall = 0;
#pragma unroll
        for (int w = 0; w < WG_BED_BLOCK / 64; w++) {
            if (w < wave) before += sb[w];
            all += sb[w];
            lall += sl[w];
        }
        if (i < n) wg_base[i] = carry + before + incl - v;
        carry += all;
        lines += lall;
        __syncthreads();
    }
    if (threadIdx.x == 0) { totals[0] = carry; totals[1] = lines; }
}

template <int ELEM>
__global__ __launch_bounds__(WG_BED_BLOCK) void k_bed_emit(wg_bed_args a, const uint64_t* __restrict__ wg_base, char* __restrict__ out)
{
    __shared__ wg_bed_table tab;
    __shared__ uint32_t waves[WG_BED_BLOCK / 64];
    __shared__ __attribute__((aligned(16))) char stage[WG_BED_STAGE_BYTES + 16];
    const int64_t* cum;
    const char* names;
    wg_bed_load_table(a, tab, cum, names);
    const wg_bed_site s = wg_bed_read<ELEM>(a, (int64_t)blockIdx.x * WG_BED_BLOCK + threadIdx.x, cum, names);
    uint32_t total;
    const uint32_t off = wg_bed_block_scan(s.len * s.mult, waves, total);
    if (total == 0) return;                                      // (the same in every thread)
    const uint64_t base = wg_base[blockIdx.x];
    if (wg_bed_staged(total, a.stage_bytes)) {
        const uint32_t pad = (uint32_t)(base & 15u);
        if (s.len && s.mult) {
            char* dst = stage + pad + off;
            wg_bed_put(a, s, names, dst);
            for (uint32_t k = 1; k < s.mult; k++)
                for (uint32_t j = 0; j < s.len; j++) dst[k * s.len + j] = dst[j];
        }
        __syncthreads();
        char* g = out + (base - pad);                            // 16-byte aligned, like `out`
        const uint32_t end = pad + total;
        for (uint32_t lo = threadIdx.x * 16u; lo < end; lo += WG_BED_BLOCK * 16u) {
            if (lo >= pad && lo + 16u <= end) {
                *reinterpret_cast<uint4*>(g + lo) = *reinterpret_cast<const uint4*>(stage + lo);
            } else {                                             // the first and the last vector: their bytes inside [pad, end)
                const uint32_t j1 = lo + 16u < end ? lo + 16u : end;
                for (uint32_t j = lo > pad ? lo : pad; j < j1; j++) g[j] = stage[j];
            }
        }
    } else if (s.len && s.mult) {
        char* slot = stage + threadIdx.x * WG_BED_MAX_LINE;
        wg_bed_put(a, s, names, slot);
        char* g = out + base + off;
        for (uint32_t k = 0; k < s.mult; k++)
            for (uint32_t j = 0; j < s.len; j++) g[(uint64_t)k * s.len + j] = slot[j];
    }
}
