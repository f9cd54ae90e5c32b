// deflate_kernels.h — text deflated into BGZF members on the device (the mirror of inflate_kernels.h):
//   k_bgzf_deflate   one member (at most 65280 bytes of text) per wavefront, three per 192-thread workgroup, each by deflate_core.h's
//                    encoder; the member goes to its slot of WG_DEF_PITCH bytes, its size to a size array
//   (k_bed_scan)     the project's scan, as it is: the sizes become every member's first byte in the packed string, and the total
//   k_bgzf_pack      every member from its slot to its place in the dense byte string, one workgroup per member, 16 bytes per store
//
// How a wave works.  Its 64 lanes run the encoder together (WgDefWaveEx): the loops deflate_core.h shares out take one turn with a lane
// per element — a group's 64 positions find their candidates and compare them with the text in global memory (where the emit pass or the
// upload left it; 4 bytes per read, whatever the alignment), enter the hash table with an LDS atomic max, count their symbols with LDS
// atomic adds, 64 tokens at a time look up their codes, prefix-sum their bit lengths over the wave (DPP) and OR their bits into a ring of
// 256 words in LDS (atomic OR: two tokens may share a word).  What is serial in the rule — the greedy pick over a group's match mask, the
// two-queue Huffman merge, the run-length pass over the code lengths, the block header — every lane computes alike from LDS (one address
// per read, which the LDS broadcasts); the state that steers it (bit position, token count, cursor, table sizes) goes through
// v_readfirstlane and lives in scalar registers, so those branches are the wave's as a whole.  Whenever words of the ring are complete the
// wave stores them to the member's slot, one word per lane; a slot begins at a multiple of 64 bytes, so these stores are aligned whatever
// the text's address is.  CRC32: the lanes take contiguous 1/64 shares of the text, each moves its register to the text's end
// (times x^(8 len) modulo the polynomial) and the wave xors them.  No wave waits for another (no flags); every loop is the encoder's
// (bounded by the member's length, a block's tokens or an alphabet).
//
// LDS: a wave's WgDeflateState is 51.6 KB (32 KB hash table, 10 KB tokens, 9.5 KB counts, codes and the length builder) and its ring
// 1 KB; three waves and the workgroup's CRC table (1 KB) are 158.8 KB, so one workgroup per CU (160 KB) and 3 waves per CU.  A table of
// 16-bit positions would fit a fourth wave, but LDS has no 16-bit atomic max, and the rule needs one: which lane wins a plain conflicting
// store is not defined.
#pragma once
#include <hip/hip_runtime.h>
#include "deflate_core.h"
#include "deflate_plan.h"
#include "wave_prims.h"

#define WG_DEF_WAVES 3                     // members per workgroup
#define WG_DEF_RING 256                    // words of the output ring: 8192 bits, what Out::settle's contract allows between two calls
#define WG_PACK_BLOCK 256

struct WgDefLds {
    WgDeflateState s;
    uint32_t ring[WG_DEF_RING];
};
static_assert(WG_DEF_WAVES * sizeof(WgDefLds) + 1024 <= 160 * 1024, "three waves' encoders and the CRC table fit a CU's LDS");

__device__ __forceinline__ void wg_def_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct WgDefWaveEx {
    int ln;
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int lanes() const { return 64; }
    __device__ __forceinline__ void sync() const { wg_def_wave_sync(); }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ uint64_t mask64(const uint32_t* m) const { return __builtin_amdgcn_ballot_w64(m[ln] != 0); }
    __device__ __forceinline__ void amax(uint32_t* p, uint32_t v) const { (void)__hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ void add(uint32_t* p, uint32_t v) const { (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ uint32_t scan(uint32_t v, uint32_t* total) const
    {
        const uint32_t incl = wg_wave_incl_scan_dpp_u32(v);
        *total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        return incl - v;
    }
    __device__ __forceinline__ uint32_t fold_xor(uint32_t v) const
    {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v ^= (uint32_t)__shfl_xor((int)v, d, 64);
        return v;
    }
};

// the member through the ring into its slot
struct WgDefWaveOut {
    uint32_t* ring;                        // WG_DEF_RING words of LDS, zero wherever nothing has been put
    uint8_t* slot;                         // WG_DEF_PITCH bytes, 64-byte aligned
    int lane;
    uint32_t fw = 0;                       // words stored to the slot so far
    __device__ __forceinline__ void bor(uint32_t w, uint32_t v)
    {
        if (v) (void)__hip_atomic_fetch_or(&ring[w & (WG_DEF_RING - 1)], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ void bits(uint64_t at, uint64_t v, int)
    {
        const uint32_t sh = (uint32_t)at & 31, w = (uint32_t)(at >> 5);
        const uint64_t rest = sh ? v >> (32 - sh) : v >> 32;
        bor(w, (uint32_t)(v << sh));
        bor(w + 1, (uint32_t)rest);
        bor(w + 2, (uint32_t)(rest >> 32));
    }
    __device__ __forceinline__ void settle(uint64_t at)
    {
        wg_def_wave_sync();
        uint32_t end = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(at >> 5));
        if (end > WG_DEF_PITCH / 4) end = WG_DEF_PITCH / 4;                 // (the encoder keeps `at` within the stored form: never taken)
        uint32_t* out = reinterpret_cast<uint32_t*>(slot);
        for (uint32_t w = fw + (uint32_t)lane; w < end; w += 64) {       // end <= (18 + 65280 + 5 + 8) / 4: inside the slot
            out[w] = ring[w & (WG_DEF_RING - 1)];
            ring[w & (WG_DEF_RING - 1)] = 0;
        }
        fw = end;
        wg_def_wave_sync();
    }
    __device__ __forceinline__ void finish(uint64_t at)
    {
        settle(at);
        const uint32_t rem = (uint32_t)(at >> 3) - 4 * fw;              // 0 .. 3 bytes of the last word
        if ((uint32_t)lane < rem) slot[4 * fw + (uint32_t)lane] = (uint8_t)(ring[fw & (WG_DEF_RING - 1)] >> (8 * lane));
    }
    // (behind stores of other lanes to the same bytes: the fence orders them)
    __device__ __forceinline__ void patch16(uint32_t byte, uint32_t v)
    {
        __threadfence();
        wg_def_wave_sync();
        if (lane < 2) slot[byte + (uint32_t)lane] = (uint8_t)(v >> (8 * lane));
    }
    __device__ __forceinline__ void stored(const uint8_t* text, uint32_t n, uint32_t crc)
    {
        __threadfence();
        wg_def_wave_sync();
        const uint32_t bsize = WG_DEF_HEAD + n + 5 + WG_DEF_TAIL - 1;
        const uint8_t head[WG_DEF_HEAD + 5] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bsize, (uint8_t)(bsize >> 8),
                                               1, (uint8_t)n, (uint8_t)(n >> 8), (uint8_t)~n, (uint8_t)~(n >> 8)};
        for (int i = 0; i < WG_DEF_HEAD + 5; i++)
            if (lane == i) slot[i] = head[i];
        for (uint32_t i = (uint32_t)lane; i < n; i += 64) slot[WG_DEF_HEAD + 5 + i] = text[i];
        if (lane < 4) slot[WG_DEF_HEAD + 5 + n + (uint32_t)lane] = (uint8_t)(crc >> (8 * lane));
        else if (lane < 8) slot[WG_DEF_HEAD + 5 + n + (uint32_t)lane] = (uint8_t)(n >> (8 * (lane - 4)));
    }
};

// text[0 .. n) as members of WG_DEF_MEMBER bytes: member m into slots + m * WG_DEF_PITCH, its size into sizes[m]
__global__ __launch_bounds__(64 * WG_DEF_WAVES) void k_bgzf_deflate(const uint8_t* __restrict__ text, int64_t n, int64_t n_members, uint8_t* __restrict__ slots,
                                                                    uint64_t* __restrict__ sizes)
{
    __shared__ WgDefLds lds[WG_DEF_WAVES];
    __shared__ uint32_t crctab[256];
    for (uint32_t i = threadIdx.x; i < 256; i += 64 * WG_DEF_WAVES) crctab[i] = wg_def_crc_entry(i);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    const int64_t m = (int64_t)blockIdx.x * WG_DEF_WAVES + wave;
    if (m >= n_members) return;                                   // (whole waves: the encoder below runs with all 64 lanes)
    const int64_t off = m * WG_DEF_MEMBER;
    const uint32_t len = (uint32_t)(n - off < WG_DEF_MEMBER ? n - off : WG_DEF_MEMBER);
    for (int i = lane; i < WG_DEF_RING; i += 64) lds[wave].ring[i] = 0;
    wg_def_wave_sync();
    WgDefWaveEx ex{lane};
    WgDefWaveOut out{lds[wave].ring, slots + m * WG_DEF_PITCH, lane};
    const uint32_t size = wg_deflate_member(ex, text + off, len, out, lds[wave].s, crctab);
    if (lane == 0) sizes[m] = size;
}

// member m: slots[m * WG_DEF_PITCH ..)[0 .. sizes[m]) -> dense[first[m] ..).  The destination is misaligned against the slot by whatever the
// members before add up to: the bytes up to its first 16-byte boundary and the last ones go singly, the rest as 16-byte stores put together
// from five aligned words of the slot (the fifth may lie behind the member: inside the slot's pitch, and its bytes are not used).
__global__ __launch_bounds__(WG_PACK_BLOCK) void k_bgzf_pack(const uint8_t* __restrict__ slots, const uint64_t* __restrict__ sizes, const uint64_t* __restrict__ first,
                                                             uint8_t* __restrict__ dense)
{
    const int64_t m = blockIdx.x;
    const uint32_t n = (uint32_t)sizes[m];
    const uint8_t* src = slots + m * WG_DEF_PITCH;
    uint8_t* dst = dense + first[m];
    uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > n) head = n;
    const uint32_t body = (n - head) & ~15u, tail0 = head + body;
    if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
    for (uint32_t v = threadIdx.x; v < body / 16; v += WG_PACK_BLOCK) {
        const uint32_t s = head + 16 * v, a = s & 3, wi = s >> 2;
        uint32_t w[5];
        for (int k = 0; k < 5; k++) w[k] = s32[wi + k];
        uint4 o;
        o.x = __builtin_amdgcn_alignbyte(w[1], w[0], a); o.y = __builtin_amdgcn_alignbyte(w[2], w[1], a);
        o.z = __builtin_amdgcn_alignbyte(w[3], w[2], a); o.w = __builtin_amdgcn_alignbyte(w[4], w[3], a);
        *reinterpret_cast<uint4*>(dst + s) = o;
    }
    for (uint32_t i = tail0 + threadIdx.x; i < n; i += WG_PACK_BLOCK) dst[i] = src[i];
}
