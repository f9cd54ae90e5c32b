// inflate_kernels.h — k_bgzf_inflate: the members of a BGZF byte string inflated on the device, one member per wavefront (four per
// 256-thread workgroup), each by inflate_core.h's decoder.
//
// How a wave works.  Its 64 lanes run the decoder with the same state: the bit reader, the table builds and the symbol decode are wave-
// uniform, and what is read back from a table goes through v_readfirstlane so that the decoder's state lives in scalar registers and
// its branches are scalar ones (the tables are in LDS; every lane reads the same address, which the LDS broadcasts), so there is no hand-over of symbols
// from one lane to the others and no branch that splits the wave inside the decoder.  The lanes differ where bytes move, and in the
// fill of a block's lookup tables (each lane walks the code for its share of the table's indexes):
//   input    the wave keeps 64 words (256 bytes) of the payload in registers, one per lane, loaded coalesced; a word reaches the bit
//            reader by v_readlane.  Lanes whose word lies at or behind the payload's end load nothing.
//   window   a 32 KB ring in LDS per wave holds the last 32768 bytes of text.  A literal is one lane's byte store.  A match is
//            copied by the wave, lane i taking byte i: in steps of at most `d` bytes with d = dist at first, so that a step never reads
//            what it writes; while d < 64, a finished step doubles d (the text from p - dist on has period dist by then, so 2 d reaches
//            the same bytes), which turns dist < len (a run: dist 1, len 258) into a few wide steps instead of len narrow ones.
//   output   whenever 16 KB of the ring are complete the wave stores them to the member's slot of the text buffer, 16 bytes per lane
//            (the bytes up to the slot's first 16-byte boundary and the last ones singly); a wave's text is written once, never read.
// Lanes exchange bytes through the ring only: LDS operations of one wave complete in order, and wave_sync() keeps the compiler from
// moving a read across the write it depends on.  No lane reads text another lane stored to global memory, no wave waits for another
// (no flags), and every loop is the decoder's (bounded by the payload's bits and ISIZE) or counts bytes of one copy.
//
// Occupancy: 4 x (32768 B ring + 7200 B tables) = 159872 B of LDS per workgroup, so one workgroup per CU (160 KB), 4 waves per CU,
// one per SIMD.  The whole <= 64 KB text of a member in LDS would halve that (2 waves per CU); reading matches back from global memory
// would lift the LDS limit but pays an L2 round trip per match on the decoder's serial path.
//
// A member that is refused: the wave stores what it decoded, fills the rest of the member's slot with '\n' (the engine's kernel behind
// reads defined bytes), and lowers *bad_member to (file offset << 8 | reason) with atomicMin: the first bad member of the file wins.
#pragma once
#include <hip/hip_runtime.h>
#include "inflate_core.h"

#define WG_INF_WAVES 4                     // members per workgroup
#define WG_INF_RING 32768                  // bytes of the window ring (a power of two, >= DEFLATE's longest distance)
#define WG_INF_FLUSH 16384                 // bytes stored to the text buffer at a time

struct WgInfLds {
    uint32_t ring[WG_INF_RING / 4];
    WgInflateTables t;
};

__device__ __forceinline__ void wg_inf_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the payload through a 64-word register window
struct WgWaveIn {
    const uint8_t* p;
    int64_t n;
    int ln;                                // this lane
    int64_t base = -64;                    // the window holds the words [base, base + 64)
    uint32_t win = 0;
    __device__ __forceinline__ uint32_t load(int64_t w) const
    {
        const int64_t at = 4 * w;
        uint32_t v = 0;
        if (at + 4 <= n) { __builtin_memcpy(&v, p + at, 4); return v; }
        for (int k = 0; k < 4; k++)
            if (at + k < n) v |= (uint32_t)p[at + k] << (8 * k);
        return v;
    }
    __device__ __forceinline__ uint32_t word(int64_t w)
    {
        if (w < base || w >= base + 64) { base = w; win = load(w + ln); }
        return (uint32_t)__builtin_amdgcn_readlane((int)win, (int)(w - base));
    }
    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ uint8_t byte(int64_t i) const { return p[i]; }
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int lanes() const { return 64; }
    __device__ __forceinline__ void sync() const { wg_inf_wave_sync(); }
};

// the text through the ring
struct WgWaveOut {
    uint8_t* ring;                         // WG_INF_RING bytes of LDS
    uint8_t* slot;                         // the member's text in the text buffer
    uint32_t isize;
    int lane;
    uint32_t at = 0, flushed = 0;          // bytes decoded, bytes stored to the slot
    static constexpr uint32_t M = WG_INF_RING - 1;
    __device__ __forceinline__ uint32_t pos() const { return at; }
    // ring bytes [lo, hi) -> slot[lo .. hi)
    __device__ __forceinline__ void store(uint32_t lo, uint32_t hi)
    {
        wg_inf_wave_sync();
        const uint32_t n = hi - lo;
        uint32_t head = (uint32_t)((16 - ((uintptr_t)(slot + lo) & 15)) & 15);
        if (head > n) head = n;
        const uint32_t body = (n - head) & ~15u, tail0 = head + body;
        if ((uint32_t)lane < head) slot[lo + lane] = ring[(lo + lane) & M];
        const uint32_t* r32 = reinterpret_cast<const uint32_t*>(ring);
        for (uint32_t v = (uint32_t)lane; v < body / 16; v += 64) {
            const uint32_t s = lo + head + 16 * v, a = s & 3, wi = (s & M) >> 2;
            uint32_t w[5];
            for (int k = 0; k < 5; k++) w[k] = r32[(wi + k) & (M >> 2)];
            uint4 o;
            o.x = __builtin_amdgcn_alignbyte(w[1], w[0], a); o.y = __builtin_amdgcn_alignbyte(w[2], w[1], a);
            o.z = __builtin_amdgcn_alignbyte(w[3], w[2], a); o.w = __builtin_amdgcn_alignbyte(w[4], w[3], a);
            *reinterpret_cast<uint4*>(slot + s) = o;
        }
        for (uint32_t i = tail0 + (uint32_t)lane; i < n; i += 64) slot[lo + i] = ring[(lo + i) & M];
        wg_inf_wave_sync();
    }
    __device__ __forceinline__ void settle()                      // after every symbol: at - flushed stays below WG_INF_FLUSH + 258
    {
        while (at - flushed >= WG_INF_FLUSH) { store(flushed, flushed + WG_INF_FLUSH); flushed += WG_INF_FLUSH; }
    }
    __device__ __forceinline__ void finish()
    {
        if (at > flushed) store(flushed, at);
        flushed = at;
    }
    __device__ __forceinline__ int lit(uint8_t b)
    {
        if (at >= isize) return WG_INF_OUT_BIG;
        if (lane == 0) ring[at & M] = b;
        at += 1;
        settle();
        return 0;
    }
    __device__ __forceinline__ int copy(uint32_t dist, uint32_t len)
    {
        if (len > isize - at) return WG_INF_OUT_BIG;
        wg_inf_wave_sync();
        uint32_t d = dist, done = 0;
        while (done < len) {                                      // at most 7 doubling steps and len / 64 + 1 others
            const uint32_t n = len - done < d ? len - done : d;
            for (uint32_t i = (uint32_t)lane; i < n; i += 64) ring[(at + done + i) & M] = ring[(at + done + i - d) & M];
            wg_inf_wave_sync();
            done += n;
            if (d < 64) d <<= 1;
        }
        at += len;
        settle();
        return 0;
    }
    __device__ __forceinline__ int stored(const WgWaveIn& in, int64_t off, uint32_t len)
    {
        if (len > isize - at) return WG_INF_OUT_BIG;
        for (uint32_t c = 0; c < len; c += 256) {
            const uint32_t n = len - c < 256 ? len - c : 256;
            for (uint32_t i = (uint32_t)lane; i < n; i += 64) ring[(at + i) & M] = in.byte(off + c + i);
            at += n;
            settle();
        }
        return 0;
    }
};

__global__ __launch_bounds__(64 * WG_INF_WAVES) void k_bgzf_inflate(const uint8_t* __restrict__ comp, const wg_bgzf_member* __restrict__ members, int64_t n_members,
                                                                    uint8_t* __restrict__ text, unsigned long long* __restrict__ bad_member)
{
    __shared__ WgInfLds lds[WG_INF_WAVES];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63);
    const int64_t m = (int64_t)blockIdx.x * WG_INF_WAVES + wave;
    if (m >= n_members) return;                                   // (whole waves: the decoder below runs with all 64 lanes)
    const wg_bgzf_member mem = members[m];
    WgWaveIn in{comp + mem.in_off, (int64_t)mem.in_len, lane};
    WgWaveOut out{reinterpret_cast<uint8_t*>(lds[wave].ring), text + mem.out_off, mem.isize, lane};
    const int why = wg_inflate_member(in, (int64_t)mem.in_len, out, mem.isize, lds[wave].t);
    out.finish();
    if (why != WG_INF_OK) {
        for (uint32_t i = out.at + (uint32_t)lane; i < mem.isize; i += 64) out.slot[i] = '\n';
        if (lane == 0) atomicMin(bad_member, ((unsigned long long)mem.file_off << 8) | (unsigned long long)why);
    }
}
