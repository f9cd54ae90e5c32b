// block_kernels.h — gfx950 kernels of the block reduction (wgbsseg_block_sums: beta_to_blocks, beta_to_table, find_markers) and of
// the marker statistics over its ratio table (wgbsseg_marker_stats).  The tile constants and the two rules host and device share
// are block_plan.h's; WG_BLOCK and the wave primitives come with seg_kernels.h.
#pragma once
#include "block_plan.h"
#include "seg_kernels.h"

// ------------------------------------------------------------------------------------------------------------
// k_block_sums: (#meth, #cov) of every block of a blocks table in every sample — the reduction of
// beta_to_blocks.py:101-126 (np.add.reduceat over the sample's (meth, cov) rows / the per-row slice sums of its
// slow_method), with its output conversions:
//   mode 0  uint32 pairs (the sums)
//   mode 1  uint8  pairs (.bin):   utils_wgbs.py:277-290 trim_to_uint8: cov > 255   -> meth = trunc(meth / cov * 255), cov = 255
//   mode 2  uint16 pairs (.lbeta): the same with 65535
//   mode 3  double meth/cov, NaN where cov < min_cov (utils_wgbs.py:270-274 beta2vec)
// HBM-bound: a blocks table that tiles the genome reads every beta byte once (2 N n bytes; 4 N n for uint16 .lbeta input).
//
// The blocks arrive SORTED by their first site (the host sorts when the table is not; `perm` then names the row a block
// came from).  One workgroup takes one tile of WG_BS_TILE consecutive sites and 4 x spw samples: every wavefront streams
// its sample's bytes of the tile ONCE with 16-byte loads (coalesced: 1 KB per wave instruction), leaves the tile's
// exclusive prefix sums of (meth, cov) in its own LDS row (two DPP scans per 512 sites), and then every lane takes blocks
// that START in the tile: a block inside the tile is one subtraction of two LDS entries; the part of a block beyond
// the tile's end (a few per cent of the blocks of a segmentation) is summed from memory by the lane.  No byte is fetched
// twice for a table that tiles the genome, whatever the block lengths; a thread per block (the first version of this
// kernel) fetched 2-3 aligned vectors per 20-byte block.
// ------------------------------------------------------------------------------------------------------------

// sums of sites [a, b) of one sample row straight from memory (tails of blocks that leave their tile): 16-byte vectors
template <int ELEM>
__device__ __forceinline__ void wg_direct_sum(const uint8_t* __restrict__ row, int64_t a, int64_t b, int64_t n_total, uint64_t& m, uint64_t& c)
{
    constexpr int SPV = ELEM == 1 ? 8 : 4;                         // sites per 16-byte vector
    for (int64_t v0 = a & ~(int64_t)(SPV - 1); v0 < b; v0 += SPV) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (v0 + SPV <= n_total) {
            const uint4 v = *reinterpret_cast<const uint4*>(row + (size_t)v0 * 2 * ELEM);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
            for (int j = 0; j < SPV; j++) if (v0 + j < n_total) {
                if (ELEM == 1) w[j >> 1] |= ((uint32_t)row[2 * (v0 + j)] | ((uint32_t)row[2 * (v0 + j) + 1] << 8)) << (16 * (j & 1));
                else w[j] = (uint32_t)reinterpret_cast<const uint16_t*>(row)[2 * (v0 + j)] | ((uint32_t)reinterpret_cast<const uint16_t*>(row)[2 * (v0 + j) + 1] << 16);
            }
        }
#pragma unroll
        for (int j = 0; j < SPV; j++) {
            const int64_t x = v0 + j;
            if (x < a || x >= b) continue;
            if (ELEM == 1) { const uint32_t h = w[j >> 1] >> (16 * (j & 1)); m += h & 0xffu; c += (h >> 8) & 0xffu; }
            else { m += w[j] & 0xffffu; c += w[j] >> 16; }
        }
    }
}

__device__ __forceinline__ void wg_block_sum_store(void* __restrict__ out, int64_t o, int mode, uint32_t min_cov, uint64_t m, uint64_t c)
{
    if (mode == 0) {
        reinterpret_cast<uint2*>(out)[o] = make_uint2((uint32_t)m, (uint32_t)c);
    } else if (mode == 1 || mode == 2) {
        const uint64_t maxv = mode == 1 ? 255u : 65535u;
        if (c > maxv) { m = (uint64_t)((double)m / (double)c * (double)maxv); c = maxv; }
        if (mode == 1) reinterpret_cast<uchar2*>(out)[o] = make_uchar2((unsigned char)m, (unsigned char)c);
        else           reinterpret_cast<ushort2*>(out)[o] = make_ushort2((unsigned short)m, (unsigned short)c);
    } else {
        reinterpret_cast<double*>(out)[o] = (c >= (uint64_t)min_cov) ? (double)m / (double)c : __builtin_nan("");
    }
}

template <int ELEM>
__device__ __noinline__ uint4 wg_bs_load_tail(const uint8_t* __restrict__ row, int64_t site, int64_t n_total)
{
    // the last vector of a row: sites beyond n_total read as zero (rare: once per row)
    constexpr int SPL = ELEM == 1 ? 8 : 4;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (int j = 0; j < SPL; j++) if (site + j < n_total) {
        if (ELEM == 1) w[j >> 1] |= ((uint32_t)row[2 * (site + j)] | ((uint32_t)row[2 * (site + j) + 1] << 8)) << (16 * (j & 1));
        else w[j] = (uint32_t)reinterpret_cast<const uint16_t*>(row)[2 * (site + j)] | ((uint32_t)reinterpret_cast<const uint16_t*>(row)[2 * (site + j) + 1] << 16);
    }
    return make_uint4(w[0], w[1], w[2], w[3]);
}

#define WG_BS_EXT 1024         // sites staged per tile = WG_BS_TILE + 128: a block that starts in the tile and ends within 128 sites
                               // of its end (almost every tile's last block) is still served from LDS; no global load sits in the
                               // reduction of the common case, where it would have to wait for the NEXT tile's prefetch as well

template <int ELEM>
struct BsTile {                // one tile's inputs in registers: the sample bytes (32 per lane and pass), and the first 128 block descriptors
    static constexpr int SPL = ELEM == 1 ? 16 : 8;             // sites per lane and pass (two 16-byte vectors)
    static constexpr int SPP = 64 * SPL;                       // sites per pass of the wavefront
    static constexpr int NPASS = WG_BS_EXT / SPP;              // uint8 rows: ONE pass stages the tile; uint16 rows: two
    static constexpr int MAXQ = ELEM == 1 ? 2 : 1;             // samples per wave
    uint4 v[MAXQ][NPASS][2];
    int32_t b0, b1, xa0, xa1, xb0, xb1, ra, rb;
};

template <int ELEM>           // bytes per count: 1 = .beta / .bin (uint8 pairs), 2 = .lbeta (uint16 pairs)
__global__ __launch_bounds__(WG_BLOCK) void k_block_sums(const uint8_t* __restrict__ betas, int64_t pitch, int64_t n_total,
                                                         const int32_t* __restrict__ x0s, const int32_t* __restrict__ x1s,
                                                         const int32_t* __restrict__ perm, const int32_t* __restrict__ tile_first,
                                                         int64_t n_tiles, int64_t n_blocks, int n_samples, int spw, int mode, uint32_t min_cov,
                                                         void* __restrict__ out)
{
    // per wave: exclusive prefixes of the staged sites of the sample it is working on.  Waves never touch each other's row and
    // a wave's LDS instructions execute in program order, so no workgroup barrier is needed anywhere in this kernel.
    // uint8 rows: a lane's 16 sites are summed IN the lane as packed pairs (meth | cov << 16: 16 x 255 fits 16 bits, one add
    // per site for both counts) and stored as such (PK), next to the lane's own base (BASE, from two wave scans per tile): a
    // prefix is BASE[x >> 4] + unpack(PK[x]).  uint16 rows (.lbeta) keep full 32-bit pairs per site (E).
    constexpr int ROW_BYTES = ELEM == 1 ? (WG_BS_EXT + 16) * 4 + (WG_BS_EXT / 16 + 2) * 8 : (WG_BS_EXT + 8) * 8;
    __shared__ __attribute__((aligned(16))) char lds[WG_BLOCK / 64][ROW_BYTES];
    typedef BsTile<ELEM> T;
    constexpr int SPL = T::SPL, SPP = T::SPP, NPASS = T::NPASS, MAXQ = T::MAXQ;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint2* Ew = reinterpret_cast<uint2*>(lds[wv]);                                        // (uint16 rows) [EXT + 1]
    uint32_t* PK = reinterpret_cast<uint32_t*>(lds[wv]);                                  // (uint8 rows) [EXT + 1]
    uint2* BASE = reinterpret_cast<uint2*>(lds[wv] + (WG_BS_EXT + 16) * 4);               // (uint8 rows) [EXT / 16 + 1]
    const int s_first = ((int)blockIdx.y * (WG_BLOCK / 64) + wv) * spw;
    if (s_first >= n_samples) return;
    const int64_t t_first = (int64_t)blockIdx.x * WG_BS_RUN;
    const size_t esz = mode == 0 ? 8 : (mode == 1 ? 2 : (mode == 2 ? 4 : 8));

    // everything a tile needs, requested in one go (nothing is waited for here)
    auto issue = [&](T& R, int64_t tile) {
        R.b0 = R.b1 = 0;
        if (tile >= n_tiles) return;
        R.b0 = tile_first[tile]; R.b1 = tile_first[tile + 1];
        if (R.b0 == R.b1) return;                                  // no block starts in this tile: nothing to read
        const int64_t lo = tile * WG_BS_TILE;
        const int64_t hi = lo + WG_BS_EXT < n_total ? lo + WG_BS_EXT : n_total;          // staged sites [lo, hi)
#pragma unroll
        for (int q = 0; q < MAXQ; q++) {
            const int s = s_first + q;
            const uint8_t* row = betas + (int64_t)(s < n_samples ? s : 0) * pitch;
#pragma unroll
            for (int p = 0; p < NPASS; p++)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int64_t site = lo + p * SPP + (int64_t)lane * SPL + h * (SPL / 2);
                    R.v[q][p][h] = make_uint4(0u, 0u, 0u, 0u);
                    if (q < spw && s < n_samples && site < hi) {
                        if (site + SPL / 2 <= n_total) R.v[q][p][h] = *reinterpret_cast<const uint4*>(row + (size_t)site * 2 * ELEM);
                        else R.v[q][p][h] = wg_bs_load_tail<ELEM>(row, site, n_total);
                    }
                }
        }
        const int ba = R.b0 + lane, bb = R.b0 + 64 + lane;
        R.xa0 = ba < R.b1 ? x0s[ba] : 0; R.xa1 = ba < R.b1 ? x1s[ba] : 0;
        R.xb0 = bb < R.b1 ? x0s[bb] : 0; R.xb1 = bb < R.b1 ? x1s[bb] : 0;
        R.ra = ba < R.b1 ? (perm ? perm[ba] : ba) : 0; R.rb = bb < R.b1 ? (perm ? perm[bb] : bb) : 0;
    };
    auto compute = [&](const T& R, int64_t tile) {
        if (R.b0 == R.b1) return;                                  // wave-uniform
        const int lo = (int)(tile * WG_BS_TILE);
        const int hi = (int64_t)lo + WG_BS_EXT < n_total ? lo + WG_BS_EXT : (int)n_total;   // staged sites [lo, hi)
        const int b0 = R.b0, b1 = R.b1;
#pragma unroll
        for (int q = 0; q < MAXQ; q++) {
            const int s = s_first + q;
            if (q >= spw || s >= n_samples) break;                 // wave-uniform
            const uint8_t* row = betas + (int64_t)s * pitch;
            char* orow = reinterpret_cast<char*>(out) + (size_t)s * (size_t)n_blocks * esz;
            uint32_t run_m = 0, run_c = 0;
#pragma unroll
            for (int p = 0; p < NPASS; p++) {
                const uint32_t w[8] = {R.v[q][p][0].x, R.v[q][p][0].y, R.v[q][p][0].z, R.v[q][p][0].w,
                                       R.v[q][p][1].x, R.v[q][p][1].y, R.v[q][p][1].z, R.v[q][p][1].w};
                if (ELEM == 1) {
                    uint32_t e[16], acc = 0;                       // packed exclusive prefixes inside the lane
#pragma unroll
                    for (int j = 0; j < 16; j++) {
                        e[j] = acc;
                        // site j as (meth | cov << 16): bytes (m, 0, c, 0) picked out of the dword that holds two sites
                        acc += __builtin_amdgcn_perm(0u, w[j >> 1], (j & 1) ? 0x0c030c02u : 0x0c010c00u);
                    }
                    const uint32_t tm = acc & 0xffffu, tc = acc >> 16;
                    const uint32_t im = wg_wave_incl_scan_dpp_u32(tm), ic = wg_wave_incl_scan_dpp_u32(tc);
                    BASE[lane] = make_uint2(im - tm, ic - tc);
                    uint4* dst = reinterpret_cast<uint4*>(PK + lane * 16);
#pragma unroll
                    for (int j = 0; j < 16; j += 4) dst[j >> 2] = make_uint4(e[j], e[j + 1], e[j + 2], e[j + 3]);
                    run_m = (uint32_t)__builtin_amdgcn_readlane((int)im, 63);
                    run_c = (uint32_t)__builtin_amdgcn_readlane((int)ic, 63);
                } else {
                    uint32_t m[SPL], c[SPL], tm = 0, tc = 0;
#pragma unroll
                    for (int j = 0; j < SPL; j++) { m[j] = w[j] & 0xffffu; c[j] = w[j] >> 16; tm += m[j]; tc += c[j]; }
                    const uint32_t im = wg_wave_incl_scan_dpp_u32(tm), ic = wg_wave_incl_scan_dpp_u32(tc);
                    uint32_t em = run_m + (im - tm), ec = run_c + (ic - tc);
                    uint2 e[SPL];
#pragma unroll
                    for (int j = 0; j < SPL; j++) { e[j] = make_uint2(em, ec); em += m[j]; ec += c[j]; }
                    uint4* dst = reinterpret_cast<uint4*>(Ew + p * SPP + lane * SPL);          // 16-byte stores, lane-contiguous
#pragma unroll
                    for (int j = 0; j < SPL; j += 2) dst[j >> 1] = make_uint4(e[j].x, e[j].y, e[j + 1].x, e[j + 1].y);
                    run_m += (uint32_t)__builtin_amdgcn_readlane((int)im, 63);
                    run_c += (uint32_t)__builtin_amdgcn_readlane((int)ic, 63);
                }
            }
            if (lane == 0) {                                       // the entry behind the last staged site (sites past `hi` were read as zeros)
                if (ELEM == 1) { BASE[WG_BS_EXT / 16] = make_uint2(run_m, run_c); PK[WG_BS_EXT] = 0u; }
                else Ew[WG_BS_EXT] = make_uint2(run_m, run_c);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            auto prefix = [&](int x) -> uint2 {                    // sums of the staged sites before x
                if (ELEM == 1) { const uint2 b = BASE[x >> 4]; const uint32_t k = PK[x]; return make_uint2(b.x + (k & 0xffffu), b.y + (k >> 16)); }
                return Ew[x];
            };
            auto one = [&](int x0, int x1, int r) {
                uint32_t m32 = 0, c32 = 0;
                if (x1 > x0) {
                    const int e = x1 < hi ? x1 : hi;
                    const uint2 pe = prefix(e - lo), ps = prefix(x0 - lo);
                    m32 = pe.x - ps.x; c32 = pe.y - ps.y;
                }
                if (x1 > hi) {                                     // rare: a block reaching beyond the staged sites
                    uint64_t m = m32, c = c32;
                    wg_direct_sum<ELEM>(row, hi, x1, n_total, m, c);
                    wg_block_sum_store(orow, r, mode, min_cov, m, c);
                } else {
                    wg_block_sum_store(orow, r, mode, min_cov, (uint64_t)m32, (uint64_t)c32);
                }
            };
            if (b0 + lane < b1) one(R.xa0, R.xa1, R.ra);
            if (b0 + 64 + lane < b1) one(R.xb0, R.xb1, R.rb);
            for (int b = b0 + 128 + lane; b < b1; b += 64) one(x0s[b], x1s[b], perm ? perm[b] : b);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();                                                       // reads done before the next row overwrites
        }
    };
    // stream the run of tiles: the next tile's bytes are in flight while this one is reduced
    T A, B;
    issue(A, t_first);
#pragma unroll 1
    for (int k = 0; k < WG_BS_RUN; k += 2) {
        issue(B, t_first + k + 1);
        compute(A, t_first + k);
        issue(A, t_first + k + 2 < t_first + WG_BS_RUN ? t_first + k + 2 : n_tiles);
        compute(B, t_first + k + 1);
    }
}

// ------------------------------------------------------------------------------------------------------------
// k_block_sums_run: the block reduction for uint8 rows and a table whose blocks are ordered by first AND by last site (every
// table a segmentation wrote; every "nice" table of beta_to_blocks.py:45-60) — the common case, streamed:
// one wavefront takes one sample and a RUN of consecutive 1024-site tiles and walks them in order, keeping running totals,
// so that the prefixes it leaves in LDS (two tiles: a ring) are prefixes of the whole run; after staging tile t it resolves
// the blocks whose LAST site lies in tile t: their first site is in tile t or t-1 (blocks up to 1024 sites), so a block is
// one subtraction of two prefixes whatever tile boundary it crosses.  Every byte is read once (no halo), two tiles are in
// flight while one is reduced, one sample per wavefront keeps it at 60-odd VGPRs.  Blocks that begin before the run or more
// than a tile back are summed from memory by their lane (one or two per run; blocks longer than 1024 sites).
// The general kernel above stays for .lbeta rows and for tables with nested / overlapping blocks.
// ------------------------------------------------------------------------------------------------------------
#define WG_BSR_PK (WG_BSR_TILE + 16)          // packed in-lane prefixes of a tile (+ the entry behind its last site)

// trunc(fl(fl(m / c) * 255)) — utils_wgbs.py:277-290 trim_to_uint8, float64 division, product, truncation — for integers 0 <= m <= c, 255 < c <= 65535 * 255.
// Round 5: it IS floor(255 m / c), always, so it is computed in integers (10 VALU instructions, none of them fp64; rounds 2-4: the reference's own three
// float64 operations, 16 instructions with v_rcp_f64 and the v_div_* family, which nearly every wavefront of the block reduction executes).  Why:
//   * 255 m / c not an integer: it lies at least 1 / c >= 6e-8 from the nearest integer, the two roundings move the product by less than 255 * 2^-52 = 6e-14;
//   * 255 m / c = K an integer: then m / c = K / 255 as a real number, so fl(m / c) = fl(K / 255) whatever m and c are, and trunc(fl(fl(K / 255) * 255)) = K for
//     every K in 0 .. 255 (256 cases: tests/test_blocks_cpu.py::test_trim_rescale_is_an_integer_division walks them, and 65535 likewise).
// The division: q = floor of a float estimate of N / c, N = 255 m < 2^32, pushed DOWN by 1e-4 — Nf and the product carry 2^-24 each, v_rcp_f32 one ulp
// (2^-23): the estimate is within 6.1e-5 of N / c <= 255, so the biased one lies in (N / c - 1.7e-4, N / c) and its floor is K or K - 1 (0 when negative:
// v_cvt_u32_f32 clamps) — then one exact correction from the remainder.  c < 2^24 is exact in float; q * c <= N needs no wider type.
__device__ __forceinline__ uint32_t wg_rescale_255(uint32_t m, uint32_t c)
{
    const uint32_t N = __umul24(m, 255u);            // m < 2^24: the low 32 bits of the 48-bit product are the product
    const float est = __builtin_fmaf((float)N, __builtin_amdgcn_rcpf((float)c), -1.0e-4f);
    uint32_t q = (uint32_t)est;                                           // (negative -> 0)
    const uint32_t r = N - __umul24(q, c);
    return q + (r >= c ? 1u : 0u);
}

// k_block_sums_direct: the blocks the streaming kernel leaves out — those that begin before their run or more than a tile
// before the tile they end in (blocks longer than 1024 sites, and one or two per run boundary): one wavefront per (block,
// sample) reads the block's bytes with 16-byte loads, 512 sites per iteration, and reduces across lanes.  Which blocks these are
// depends on the table alone: the host lists them.
__global__ __launch_bounds__(WG_BLOCK) void k_block_sums_direct(const uint8_t* __restrict__ betas, int64_t pitch, int64_t n_total,
                                                                const int32_t* __restrict__ x0s, const int32_t* __restrict__ x1s,
                                                                const int32_t* __restrict__ perm, const int32_t* __restrict__ list, int64_t n_list,
                                                                int64_t n_blocks, int n_samples, int mode, uint32_t min_cov, void* __restrict__ out)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int s = (int)blockIdx.y * (WG_BLOCK / 64) + wv;
    if (s >= n_samples || (int64_t)blockIdx.x >= n_list) return;
    const int b = list[blockIdx.x];
    const int x0 = x0s[b], x1 = x1s[b];
    const uint8_t* row = betas + (int64_t)s * pitch;
    const int64_t last_vec = ((n_total + 7) >> 3) - 1;
    unsigned long long m = 0, c = 0;
    for (int64_t v0 = (int64_t)(x0 & ~7) + 8 * lane; v0 < x1; v0 += 512) {
        const int64_t vi = v0 >> 3;
        const uint4 v = reinterpret_cast<const uint4*>(row)[vi < last_vec ? vi : last_vec];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int64_t x = v0 + j;
            if (x < x0 || x >= x1) continue;
            const uint32_t hh = w[j >> 1] >> (16 * (j & 1));
            m += hh & 0xffu; c += (hh >> 8) & 0xffu;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { m += __shfl_down(m, o); c += __shfl_down(c, o); }
    if (lane == 0) {
        const size_t esz = mode == 0 ? 8 : (mode == 1 ? 2 : (mode == 2 ? 4 : 8));
        char* orow = reinterpret_cast<char*>(out) + (size_t)s * (size_t)n_blocks * esz;
        wg_block_sum_store(orow, perm ? perm[b] : b, mode, min_cov, (uint64_t)m, (uint64_t)c);
    }
}

#ifndef WG_BSR_PRE
#define WG_BSR_PRE 3                           // rounds of 64 block descriptors fetched a tile ahead (a tile of a segmentation ends ~100 blocks)
#endif
#define WG_BSR_RING (2 * WG_BSR_TILE)
#ifndef WG_BSR_AHEAD
#define WG_BSR_AHEAD 4                         // tiles of sample bytes in flight per wavefront (2 KB each)
#endif

// LDS layout of the prefix ring: ring position q = (half, site x of the tile); the four sites 4 g .. 4 g + 3 of lane L (x = 16 L +
// 4 g + k) sit at dwords (g * 64 + L) * 4 + k of their half: consecutive lanes write consecutive 16-byte slots (no bank
// conflicts; lane-major rows of 16 dwords are 16-way conflicts).
__host__ __device__ __forceinline__ uint32_t wg_bsr_pk_at(uint32_t q)
{
    // x = SPL L + 4 g + k  ->  (g * 64 + L) * 4 + k
    constexpr uint32_t GM = (WG_BSR_SPL / 4 - 1) << 2;           // the bits of g in x
    constexpr int LS = WG_BSR_SPL == 16 ? 4 : 3;                  // log2(SPL)
    return (q & ~(uint32_t)(WG_BSR_TILE - 1)) | ((q & GM) << 6) | (((q & (WG_BSR_TILE - 1)) >> LS) << 2) | (q & 3u);
}

// k_block_sums_prep: what the streaming kernel needs to know about a block depends on the table alone, so it is worked out once
// per call, not once per sample: the LDS addresses of the two prefixes whose difference is the block's sum — INCLUSIVE
// prefixes I(x1 - 1) - I(x0 - 1): the last site x1 - 1 lies in the block's tile, x0 - 1 in it or in the previous one, an
// empty block reads one entry twice, and the position before the run's first site is an entry kept at zero — and the row
// the result goes to (-1: a block the ring cannot serve, k_block_sums_direct's).
//   d1[b] / d0[b] = byte offset of the PK entry | byte offset of the BASE entry << 16
__global__ __launch_bounds__(WG_BLOCK) void k_block_sums_prep(const int32_t* __restrict__ x0s, const int32_t* __restrict__ x1s, const int32_t* __restrict__ perm,
                                                              int64_t n_blocks, int64_t n_tiles, int32_t* __restrict__ d1, int32_t* __restrict__ d0, int32_t* __restrict__ rr)
{
    const int64_t b = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (b >= n_blocks) return;
    const int x0 = x0s[b], x1 = x1s[b];
    int64_t t = wg_bsr_tile_of(x0, x1);                                     // the tile the block is resolved in
    if (t > n_tiles - 1) t = n_tiles - 1;                                   // (an empty block at the very end of a row that fills its last tile: the host's table, which
                                                                            //  ends with n_blocks, puts it into the last tile without a clamp)
    const int h = (int)(t % WG_BSR_RUN) & 1;
    const int lo = (int)(t * WG_BSR_TILE);
    const uint32_t q1 = (uint32_t)(h * WG_BSR_TILE + (x1 - 1 - lo)) & (WG_BSR_RING - 1), q0 = (uint32_t)(h * WG_BSR_TILE + (x0 - 1 - lo)) & (WG_BSR_RING - 1);
    const bool reach = wg_bsr_ring_reaches(x0, x1, t);
    d1[b] = (int32_t)((wg_bsr_pk_at(q1) * 4u) | (((q1 / WG_BSR_SPL) * 8u) << 16));
    d0[b] = (int32_t)((wg_bsr_pk_at(q0) * 4u) | (((q0 / WG_BSR_SPL) * 8u) << 16));
    rr[b] = reach ? (perm ? perm[b] : (int32_t)b) : -1;
}

// Straight-line code on purpose: the tile loop is unrolled (register sets rotate by renaming, not by moves), everything a
// wavefront shares is forced into scalar registers (its sample's row, its LDS rows, the run's tile table), loads that may
// fall outside are clamped instead of predicated, no calls and no per-block address arithmetic (k_block_sums_prep), and the
// output mode is a template parameter.
template <int MODE>
__global__ __launch_bounds__(WG_BLOCK) void k_block_sums_run(const uint8_t* __restrict__ betas, int64_t pitch, int64_t n_total,
                                                             const int32_t* __restrict__ d1s, const int32_t* __restrict__ d0s,
                                                             const int32_t* __restrict__ rrs, const int32_t* __restrict__ end_first,
                                                             int64_t n_tiles, int64_t n_blocks, int n_samples, uint32_t min_cov,
                                                             void* __restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint32_t PKs[WG_BLOCK / 64][WG_BSR_RING];      // packed (meth | cov << 16) INCLUSIVE prefixes inside a lane's 16 sites
    __shared__ uint2 BASEs[WG_BLOCK / 64][WG_BSR_RING / WG_BSR_SPL];                        // the run's totals before each lane's sites
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = (int)blockIdx.y * (WG_BLOCK / 64) + wv;
    if (s >= n_samples) return;
    const int64_t t0 = (int64_t)blockIdx.x * WG_BSR_RUN;
    const int nt = (int)((t0 + WG_BSR_RUN < n_tiles ? t0 + WG_BSR_RUN : n_tiles) - t0);       // tiles of this run
    // the run's slice of the tile table in one register (lane i: first block resolved in tile t0 + i or later)
    const int efv = end_first[t0 + (lane <= nt ? lane : nt)];
    if (__builtin_amdgcn_readlane(efv, 0) == __builtin_amdgcn_readlane(efv, nt)) return;     // no block ends in this run: nothing to read
    const uint8_t* row = betas + (int64_t)s * pitch;
    constexpr uint32_t ESZ = MODE == 0 ? 8u : (MODE == 1 ? 2u : (MODE == 2 ? 4u : 8u));
    char* orow = reinterpret_cast<char*>(out) + (size_t)s * (size_t)n_blocks * ESZ;      // (the host keeps n_blocks * 8 below 2^32: 32-bit offsets)
    uint32_t* PK = PKs[wv];
    uint2* BASE = BASEs[wv];
    const char* PKc = reinterpret_cast<const char*>(PK);
    const char* BASEc = reinterpret_cast<const char*>(BASE);
    const uint32_t site0 = (uint32_t)(t0 * WG_BSR_TILE);           // first site of the run (n_total < 2^31)
    const uint32_t last_vec = (uint32_t)(((n_total + 7) >> 3) - 1);                       // last 16-byte vector that holds a site of the row
    const int nb_all = (int)n_blocks;

    // this lane's 16 sites of the run's tile i: two 16-byte vectors.  A vector beyond the row is clamped onto the row's last
    // one (readable: the pitch is a multiple of 16 bytes) — it only feeds prefixes behind every block's last site.  The last
    // vector itself may hold sites beyond n_total: bytes of the row's padding, which no block reaches either.
    auto load = [&](int i, uint4& a, uint4& b) {                   // (a tile behind the run's last: that one again — no branch, nobody uses it)
        constexpr uint32_t VPL = WG_BSR_SPL / 8;                   // 16-byte vectors per lane
        const uint32_t v = ((site0 + (uint32_t)(i < nt ? i : nt - 1) * WG_BSR_TILE) >> 3) + VPL * (uint32_t)lane;
        const uint4* rv = reinterpret_cast<const uint4*>(row);
        a = rv[v < last_vec ? v : last_vec];
        if (VPL > 1) b = rv[v + 1u < last_vec ? v + 1u : last_vec]; else b = a;
    };
    struct Desc { int32_t d1[WG_BSR_PRE], d0[WG_BSR_PRE], r[WG_BSR_PRE]; };
    auto descriptors = [&](int i, Desc& D) {                       // the first 64 x WG_BSR_PRE blocks resolved in tile i of the run
        const int b0 = __builtin_amdgcn_readlane(efv, i), b1 = __builtin_amdgcn_readlane(efv, i + 1);
#pragma unroll
        for (int k = 0; k < WG_BSR_PRE; k++) {
            const int b = b0 + 64 * k + lane;
            const int bq = b < nb_all ? b : nb_all - 1;            // (clamped, not predicated)
            D.d1[k] = d1s[bq];
            D.d0[k] = d0s[bq];
            const int r = rrs[bq];
            D.r[k] = b < b1 ? r : -1;
        }
    };
    uint32_t run_m = 0, run_c = 0;                                 // totals of the run's sites before the current tile
    auto stage = [&](int h, const uint4& c0, const uint4& c1) {
        const uint32_t w[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
        uint32_t e[WG_BSR_SPL], acc = 0;                          // packed inclusive prefixes inside the lane (16 x 255 fits 16 bits)
#pragma unroll
        for (int j = 0; j < WG_BSR_SPL; j++) {
            acc += __builtin_amdgcn_perm(0u, w[j >> 1], (j & 1) ? 0x0c030c02u : 0x0c010c00u);     // site j as (meth | cov << 16)
            e[j] = acc;
        }
        const uint32_t tm = acc & 0xffffu, tc = acc >> 16;
        const uint32_t im = wg_wave_incl_scan_dpp_u32(tm), ic = wg_wave_incl_scan_dpp_u32(tc);
        BASE[h * 64 + lane] = make_uint2(run_m + (im - tm), run_c + (ic - tc));
        uint4* dst = reinterpret_cast<uint4*>(PK + h * WG_BSR_TILE) + lane;
#pragma unroll
        for (int j = 0; j < WG_BSR_SPL; j += 4) dst[(j >> 2) * 64] = make_uint4(e[j], e[j + 1], e[j + 2], e[j + 3]);
        run_m += (uint32_t)__builtin_amdgcn_readlane((int)im, 63);
        run_c += (uint32_t)__builtin_amdgcn_readlane((int)ic, 63);
    };
    auto one = [&](int d1, int d0, int r) {
        const uint2 be = *reinterpret_cast<const uint2*>(BASEc + ((uint32_t)d1 >> 16)), bs = *reinterpret_cast<const uint2*>(BASEc + ((uint32_t)d0 >> 16));
        const uint32_t ke = *reinterpret_cast<const uint32_t*>(PKc + ((uint32_t)d1 & 0xffffu)), ks = *reinterpret_cast<const uint32_t*>(PKc + ((uint32_t)d0 & 0xffffu));
        uint32_t m32 = (be.x + (ke & 0xffffu)) - (bs.x + (ks & 0xffffu));
        uint32_t c32 = (be.y + (ke >> 16)) - (bs.y + (ks >> 16));
        const uint32_t o = (uint32_t)r * ESZ;
        if (MODE == 0) {
            *reinterpret_cast<uint2*>(orow + o) = make_uint2(m32, c32);
        } else if (MODE == 3) {
            *reinterpret_cast<double*>(orow + o) = (c32 >= min_cov) ? (double)m32 / (double)c32 : __builtin_nan("");
        } else if (MODE == 1) {
            if (c32 > 255u) {
                // the integer form is proved for 0 <= m <= c (tests/test_blocks_cpu.py); a corrupt file with meth > cov — the block reduction, like
                // the reference's (beta_to_blocks.py:101-126), does not check — takes the float64 form every other kernel of the reduction uses
                // (wg_block_sum_store), so that a table's rows do not depend on which kernel produced them
                m32 = m32 <= c32 ? wg_rescale_255(m32, c32) : (uint32_t)(uint64_t)((double)m32 / (double)c32 * 255.0);
                c32 = 255u;
            }
            *reinterpret_cast<uchar2*>(orow + o) = make_uchar2((unsigned char)m32, (unsigned char)c32);
        } else {
            if (c32 > 65535u) { m32 = (uint32_t)(uint64_t)((double)m32 / (double)c32 * 65535.0); c32 = 65535u; }     // (> 257 saturated sites: rare)
            *reinterpret_cast<ushort2*>(orow + o) = make_ushort2((unsigned short)m32, (unsigned short)c32);
        }
    };
    auto resolve = [&](int i, const Desc& D) {
#pragma unroll
        for (int k = 0; k < WG_BSR_PRE; k++)
            if (D.r[k] >= 0) one(D.d1[k], D.d0[k], D.r[k]);
        const int b1 = __builtin_amdgcn_readlane(efv, i + 1);
        for (int b = __builtin_amdgcn_readlane(efv, i) + 64 * WG_BSR_PRE + lane; b < b1; b += 64) { const int r = rrs[b]; if (r >= 0) one(d1s[b], d0s[b], r); }
    };

    if (lane == 0) { PK[WG_BSR_RING - 1] = 0u; BASE[WG_BSR_RING / WG_BSR_SPL - 1] = make_uint2(0u, 0u); }      // I(-1) of the run: the entry "before" tile 0
    constexpr int AHEAD = WG_BSR_AHEAD;                            // tiles in flight behind the one being staged
    uint4 va[AHEAD + 1], vb[AHEAD + 1];                            // tile i in set i mod (AHEAD + 1)
    Desc D[2];                                                     // descriptors of tile i in set i mod 2
    load(0, va[0], vb[0]);
    descriptors(0, D[0]);
#pragma unroll
    for (int a = 1; a < AHEAD; a++) load(a, va[a], vb[a]);
#pragma unroll
    for (int i = 0; i < WG_BSR_RUN; i++) {
        if (i < nt) {                                              // (wave-uniform)
            // (vector memory operations of a wave complete in order: the descriptors, needed one tile from now, go first, so that
            // waiting for them leaves the bytes of the tiles ahead in flight)
            descriptors(i + 1, D[(i + 1) & 1]);                    // (behind the run's last tile: an empty range)
            load(i + AHEAD, va[(i + AHEAD) % (AHEAD + 1)], vb[(i + AHEAD) % (AHEAD + 1)]);
            stage(i & 1, va[i % (AHEAD + 1)], vb[i % (AHEAD + 1)]);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            resolve(i, D[i & 1]);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();                       // (the half written next is the one last read a tile ago)
        }
    }
}

// ------------------------------------------------------------------------------------------------------------
// k_marker_stats: per block, the statistics of a target and a background set of samples that `wgbstools find_markers` filters
// on (find_markers.py:188-196 coverage filter, :318-335 find_X_markers: nanmean / min / max per group), from the
// device-resident table of meth/cov ratios (mode 3 of the block reduction: NaN = below min_cov).  One thread per block;
// the samples of a set are visited in the order given (the column order of the reference's DataFrame): the sum is the
// sequential one numpy takes over that axis.  out[b] = {n_tg, sum_tg, min_tg, max_tg, n_bg, sum_bg, min_bg, max_bg}
// (min / max NaN when the set has no value).
// ------------------------------------------------------------------------------------------------------------
// (round 6: two blocks per thread, a group of four samples' loads in flight before the first of them is used, selects instead of branches —
//  the same operations on the same values in the same order: a thread's one dependent 8-byte load at a time held the pass at 0.50 of the HBM peak)
__device__ __forceinline__ void wg_marker_fold(double v, double& cnt, double& sum, double& mn, double& mx)
{
    const bool num = v == v;
    cnt += num ? 1.0 : 0.0;
    sum += num ? v : 0.0;                                       // numpy's nanmean adds the zero it put in place of the NaN
    const double lo = (mn == mn) ? (v < mn ? v : mn) : v, hi = (mx == mx) ? (v > mx ? v : mx) : v;
    mn = num ? lo : mn;
    mx = num ? hi : mx;
}

// A wavefront's 64 result rows (8 doubles each) are contiguous in `out`: staged in LDS and written as 16-byte vectors, a wavefront store = 1 KB in one
// piece (the direct form — eight 8-byte stores per thread, 64 bytes apart across the lanes — touched 64 cache lines per store instruction).
__device__ __forceinline__ void wg_marker_store(double (*st)[9], double* __restrict__ out, int64_t b, int64_t n_blocks, int lane, const double (&r)[8])
{
    const int64_t wave_b = b - lane;                             // first block of the wavefront
    if (wave_b + 64 <= n_blocks) {
#pragma unroll
        for (int q = 0; q < 8; q++) st[lane][q] = r[q];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        double2* o2 = reinterpret_cast<double2*>(out + wave_b * 8);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int e = 128 * j + 2 * lane;                    // element of the wavefront's 512 doubles
            o2[64 * j + lane] = make_double2(st[e >> 3][e & 7], st[e >> 3][(e & 7) + 1]);
        }
        __builtin_amdgcn_wave_barrier();
    } else if (b < n_blocks) {
        double* o = out + b * 8;
#pragma unroll
        for (int q = 0; q < 8; q++) o[q] = r[q];
    }
}

__global__ __launch_bounds__(WG_BLOCK) void k_marker_stats(const double* __restrict__ V, int64_t n_blocks, const int32_t* __restrict__ tg, int n_tg,
                                                           const int32_t* __restrict__ bg, int n_bg, double* __restrict__ out)
{
    __shared__ double stage[WG_BLOCK / 64][64][9];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t half = (int64_t)gridDim.x * WG_BLOCK;         // the grid covers half of the blocks: thread t takes blocks t and t + half
    const int64_t b0 = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x, b1 = b0 + half;
    // (no early return: the wavefront stores below want all 64 lanes; a lane without a block reads block 0 and drops the result)
    const int64_t c0 = b0 < n_blocks ? b0 : 0, c1 = b1 < n_blocks ? b1 : c0;
    const double nan = __builtin_nan("");
    double r0[8], r1[8];
#pragma unroll
    for (int set = 0; set < 2; set++) {
        const int32_t* idx = set ? bg : tg;
        const int n = set ? n_bg : n_tg;
        double cnt0 = 0.0, sum0 = 0.0, mn0 = nan, mx0 = nan, cnt1 = 0.0, sum1 = 0.0, mn1 = nan, mx1 = nan;
        int k = 0;
        for (; k + 4 <= n; k += 4) {
            double u[4], w[4];
#pragma unroll
            for (int q = 0; q < 4; q++) { const int64_t row = (int64_t)idx[k + q] * n_blocks; u[q] = V[row + c0]; w[q] = V[row + c1]; }
#pragma unroll
            for (int q = 0; q < 4; q++) { wg_marker_fold(u[q], cnt0, sum0, mn0, mx0); wg_marker_fold(w[q], cnt1, sum1, mn1, mx1); }
        }
        for (; k < n; k++) {
            const int64_t row = (int64_t)idx[k] * n_blocks;
            const double u = V[row + c0], w = V[row + c1];
            wg_marker_fold(u, cnt0, sum0, mn0, mx0); wg_marker_fold(w, cnt1, sum1, mn1, mx1);
        }
        r0[4 * set] = cnt0; r0[4 * set + 1] = sum0; r0[4 * set + 2] = mn0; r0[4 * set + 3] = mx0;
        r1[4 * set] = cnt1; r1[4 * set + 1] = sum1; r1[4 * set + 2] = mn1; r1[4 * set + 3] = mx1;
    }
    wg_marker_store(stage[wv], out, b0, n_blocks, lane, r0);
    wg_marker_store(stage[wv], out, b1, n_blocks, lane, r1);
}
