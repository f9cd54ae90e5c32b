// pat_kernels.h — the pat text format on gfx950: the staging of a tile of pat text in LDS, its line finding and the parsing of a
// line, shared by every kernel that reads a pat file (k_pat_count here, k_homog_count in homog_kernels.h, k_frag_hist in frag_kernels.h, k_bim_tile_count /
// k_bim_fill in bimodal_kernels.h), and the pat -> beta kernels k_pat_count / k_pat_trim.  Includes block_kernels.h for the
// wg_block_sum_store that k_pat_trim uses (and, through it, seg_kernels.h for WG_BLOCK and wg_wave_incl_scan_dpp_u32).
#pragma once
#include "block_kernels.h"

// ------------------------------------------------------------------------------------------------------------
// k_pat_count / k_pat_trim: a pat file -> (#meth, #cov) per CpG, the producer of the path's input (src/pat2beta/
// stdin2beta.cpp:59-93 proc_line, :95-123 parse; utils_wgbs.py:277-290 trim_to_uint8).  A pat line is
//     chr \t first CpG index \t pattern over {C, T, H, .} \t number of reads with that pattern [\t ...]
// Every line adds `count` to the coverage of every site under a C / T / H and to the methylated count under C / H
// (atomics on int32: reads overlap).  Reads that end before `start` or begin at or after `end` are skipped, sites outside
// are ignored, empty lines are skipped (stdin2beta.cpp:75-78,:100).  A line with fewer than four fields or a non-numeric
// site / count makes the reference give up ("failed calculating beta"): its offset is reported through `bad`.
// ------------------------------------------------------------------------------------------------------------
// Round 5: the text is parsed out of LDS, one LINE per thread.  (Rounds 3-4: one thread per BYTE, the thread on a line's first byte parsing
// it alone with byte loads from global memory — 1 lane in ~25 at work, each a chain of dependent loads.)  A workgroup takes WG_PAT_TILE
// bytes of the chunk + WG_PAT_OVER bytes behind them (a line that begins in the tile may end there) into LDS with 16-byte loads, finds
// the line starts of its tile (16 bytes per thread, a workgroup-wide prefix count), and thread l then parses line l: ~160 lines of ~25
// bytes per tile.  A line that runs past the staged bytes (a read of hundreds of CpGs) reads the rest from global memory.
#define WG_PAT_TILE 4096
#define WG_PAT_OVER 1024
struct PatText {
    const char* lds; const char* __restrict__ g; int64_t base, n;          // staged bytes [base, base + WG_PAT_TILE + WG_PAT_OVER) of g[0, n)
    __device__ __forceinline__ char at(int64_t i) const { const int64_t r = i - base; return r < WG_PAT_TILE + WG_PAT_OVER ? lds[r] : g[i]; }
};

// The LDS of one tile, declared __shared__ once per kernel that stages pat text.
struct PatTile {
    __attribute__((aligned(16))) char tx[16 + WG_PAT_TILE + WG_PAT_OVER];   // tx[15] = the byte before the tile; the tile from tx[16] (uint4 stores)
    uint16_t lstart[WG_PAT_TILE / 2 + 1];     // tile-relative first bytes of the lines that begin in the tile (at most every other byte)
    uint32_t wtot[WG_BLOCK / 64];             // lines per wavefront (the workgroup-wide prefix count)
    // the staged tile at byte `base` of g[0, n)
    __device__ __forceinline__ PatText text(const char* __restrict__ g, int64_t base, int64_t n) const { return {tx + 16, g, base, n}; }
};

__device__ __forceinline__ bool wg_parse_int(const PatText& t, int64_t& i, int64_t n, int64_t& val)
{
    // std::stoi: leading white space, an optional sign, at least one digit; anything after the digits is ignored
    char ch;
    while (i < n && ((ch = t.at(i)) == ' ' || (ch >= 9 && ch <= 13 && ch != '\n' && ch != '\t'))) i++;
    bool neg = false;
    if (i < n && ((ch = t.at(i)) == '-' || ch == '+')) { neg = ch == '-'; i++; }
    if (!(i < n && (ch = t.at(i)) >= '0' && ch <= '9')) return false;
    int64_t v = 0;
    while (i < n && (ch = t.at(i)) >= '0' && ch <= '9') { v = v * 10 + (ch - '0'); if (v > 0x7fffffffLL) return false; i++; }
    val = neg ? -v : v;
    return true;
}

// The staging and line finding of the tile at byte `base`: t.tx receives the bytes, t.lstart the tile-relative first bytes of the lines
// that begin in the tile; returns their number.  Every thread of the workgroup calls it (it synchronises).
__device__ __forceinline__ uint32_t wg_pat_tile_lines(const char* __restrict__ text, int64_t n, int64_t base, PatTile& t)
{
    char* tx = t.tx;
    uint16_t* lstart = t.lstart;
    uint32_t* wtot = t.wtot;
    static_assert(WG_PAT_TILE == 16 * WG_BLOCK && WG_PAT_OVER % 16 == 0 && WG_PAT_OVER / 16 <= WG_BLOCK, "16 bytes per thread");
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // ---- stage: 16 bytes per thread (the chunk's buffer is 16-byte aligned and so is base), bytes at or past n as '\n'
    auto stage16 = [&](int64_t off) {                        // off: tile-relative, multiple of 16
        const int64_t a = base + off;
        uint4 v;
        if (a + 16 <= n) v = *reinterpret_cast<const uint4*>(text + a);
        else {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int j = 0; j < 16; j++) w[j >> 2] |= (uint32_t)(unsigned char)(a + j < n ? text[a + j] : '\n') << (8 * (j & 3));
            v.x = w[0]; v.y = w[1]; v.z = w[2]; v.w = w[3];
        }
        *reinterpret_cast<uint4*>(tx + 16 + off) = v;
    };
    stage16((int64_t)tid * 16);
    if (tid < WG_PAT_OVER / 16) stage16(WG_PAT_TILE + (int64_t)tid * 16);
    if (tid == 0) tx[15] = base > 0 ? text[base - 1] : '\n';
    __syncthreads();
    // ---- line starts of the tile: byte x begins a line when the byte before it is a newline and it is not one itself (empty lines: skipped,
    // stdin2beta.cpp:100)
    uint32_t mask = 0;
    {
        const char* q = tx + 16 + tid * 16;
        char prev = q[-1];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const char c = q[j];
            if (prev == '\n' && c != '\n' && base + tid * 16 + j < n) mask |= 1u << j;
            prev = c;
        }
    }
    const uint32_t cnt = (uint32_t)__popc(mask);
    const uint32_t incl = wg_wave_incl_scan_dpp_u32(cnt);
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    uint32_t before = incl - cnt, total = 0;
#pragma unroll
    for (int w = 0; w < WG_BLOCK / 64; w++) { if (w < wv) before += wtot[w]; total += wtot[w]; }
    while (mask) {
        const int j = __ffs((int)mask) - 1;
        mask &= mask - 1;
        lstart[before++] = (uint16_t)(tid * 16 + j);
    }
    __syncthreads();
    return total;
}

// The four fields of the pat line that begins at byte p: site, the pattern's first byte ps and length plen, count; false when the line
// has fewer than four fields or its site / count is not a number (what makes the reference's std::stoi throw).
__device__ __forceinline__ bool wg_pat_parse_line(const PatText& T, int64_t p, int64_t n, int64_t& site, int64_t& ps, int64_t& plen, int64_t& count)
{
    int64_t i = p;
    char ch = 0;
    bool ok = true;
    while (i < n && (ch = T.at(i)) != '\t' && ch != '\n') i++;   // field 1: chromosome
    ok = i < n && ch == '\t';
    if (ok) {
        i++;
        ok = wg_parse_int(T, i, n, site);                           // field 2: index of the read's first CpG
    }
    if (ok) {
        while (i < n && (ch = T.at(i)) != '\t' && ch != '\n') i++;
        ok = i < n && ch == '\t';
    }
    if (ok) {
        i++;
        ps = i;                                                     // field 3: the pattern
        while (i < n && (ch = T.at(i)) != '\t' && ch != '\n') i++;
        ok = i < n && ch == '\t';
        plen = i - ps;
    }
    if (ok) {
        i++;
        ok = i < n && T.at(i) != '\n' && wg_parse_int(T, i, n, count);   // field 4: how many reads (an empty one: stoi throws)
    }
    return ok;
}

// The two ends of the sortedness check of a kernel that walks a chunk tile by tile (k_frag_hist in frag_kernels.h; k_homog_count has
// the same two steps written out in its body).  WG_PAT_NO_SITE: no read (none yet, or a malformed line: nothing to compare with).
#define WG_PAT_NO_SITE ((long long)INT64_MIN)

// The start of the read before the first line of the tile at byte `base`: back over empty lines to the line that holds byte base - 1,
// parsed from global memory; *prev_in (the last read of the chunks before) when the tile's first line is the chunk's first.  One thread.
__device__ __forceinline__ long long wg_pat_site_before(const char* __restrict__ text, int64_t n, int64_t base, const long long* prev_in)
{
    int64_t i = base - 1;
    while (i >= 0 && text[i] == '\n') i--;
    if (i < 0) return *prev_in;
    while (i > 0 && text[i - 1] != '\n') i--;
    const PatText G = {text, text, INT64_MIN / 4, n};               // (base far below: every byte from g)
    int64_t site = 0, ps = 0, plen = 0, count = 0;
    return wg_pat_parse_line(G, i, n, site, ps, plen, count) ? (long long)site : WG_PAT_NO_SITE;
}

// Is the line whose pattern is [ps, ps + plen) the chunk's last read (only newlines behind its end)?  Its start is then what the next
// chunk's first read is checked against (prev_out).
__device__ __forceinline__ bool wg_pat_is_last_read(const PatText& T, int64_t ps, int64_t plen, int64_t n)
{
    int64_t i = ps + plen;
    while (i < n && T.at(i) != '\n') i++;
    while (i < n && T.at(i) == '\n') i++;
    return i == n;
}

__global__ __launch_bounds__(WG_BLOCK) void k_pat_count(const char* __restrict__ text, int64_t n, int64_t start, int64_t end,
                                                        int32_t* __restrict__ meth, int32_t* __restrict__ cov, unsigned long long* bad,
                                                        unsigned long long chunk_off)
{
    __shared__ PatTile tile;
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * WG_PAT_TILE;
    const uint32_t total = wg_pat_tile_lines(text, n, base, tile);
    // ---- one line per thread
    const PatText T = tile.text(text, base, n);
    const int64_t nr = end - start;
    for (uint32_t l = (uint32_t)tid; l < total; l += WG_BLOCK) {
        const int64_t p = base + tile.lstart[l];
        int64_t site = 0, count = 0, ps = 0, plen = 0;
        const bool ok = wg_pat_parse_line(T, p, n, site, ps, plen, count);
        if (!ok) { atomicMin(bad, chunk_off + (unsigned long long)p); continue; }
        if (site + plen - 1 < start || site >= end) continue;           // stdin2beta.cpp:75-78
        for (int64_t k = 0; k < plen; k++) {
            const int64_t x = site - start + k;
            if (x < 0 || x >= nr) continue;
            const char c = T.at(ps + k);
            if (!(c == 'T' || c == 'C' || c == 'H')) continue;
            atomicAdd(&cov[x], (int32_t)count);
            if (c != 'T') atomicAdd(&meth[x], (int32_t)count);
        }
    }
}

// counts -> .beta (uint8 pairs) or .lbeta (uint16 pairs): rows whose coverage exceeds the type's maximum M become
// (trunc(meth / cov * M), M) (utils_wgbs.py:277-290; the same rule as modes 1 / 2 of the block reduction)
__global__ __launch_bounds__(WG_BLOCK) void k_pat_trim(const int32_t* __restrict__ meth, const int32_t* __restrict__ cov, int64_t n, int lbeta, void* __restrict__ out)
{
    const int64_t x = (int64_t)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (x >= n) return;
    wg_block_sum_store(out, x, lbeta ? 2 : 1, 0u, (uint64_t)(uint32_t)meth[x], (uint64_t)(uint32_t)cov[x]);
}
