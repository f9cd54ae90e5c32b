// bimodal_kernels.h — `wgbstools test_bimodal` on gfx950: per block, the reference's two-allele hard-assignment EM over the
// reads of the block and the one-allele likelihood it is tested against.  The pat text format comes from pat_kernels.h (WG_PAT_TILE,
// PatTile, PatText, wg_pat_tile_lines, wg_pat_parse_line); WG_BLOCK and wg_log2 with g_wg_tables through its seg_kernels.h.
//
// The reference (src/python/test_bimodal.py:25-176) asks tabix, per block [s1, s2), for the reads starting in
// [max(1, s1 - 150), s2 - 1], builds a dense matrix with one row per read copy and runs its EM in numpy.  Here the pat text
// streams through the device once:
//   feed    k_bim_tile_count / k_bim_tile_scan / k_bim_fill parse each chunk (the tile staging and line parser of
//           k_pat_count) into a compact READ TABLE: start, length, count (int32) and the pattern at 2 bits per site
//           (0 unobserved, 1 C, 2 T) in 32-bit words; k_bim_order checks that starts never descend.  The text does not stay.
//   retire  the host keeps the blocks sorted by s2; once a read starting at or after s2 has been seen, every read the block
//           can use is in the table, so its EM runs right away (k_bim_gather, then k_bim_em) while the host inflates the
//           next chunk.  Reads starting before the lowest max(1, s1 - 150) of the blocks still pending are then dropped
//           (k_bim_drop_find / k_bim_drop_copy), so the table holds the live window, not the file.
//   EM      k_bim_em: one wavefront per block.  The four log2 tables of the block's columns (32 B per column) and the
//           per-cluster C / T column counts (16 B per column; WG_BIM_COL_BYTES in all) live in LDS up to WG_BIM_LDS_COLS columns,
//           in global scratch beyond (the host sizes it from k_bim_gather's column counts: wg_bim_scratch_layout).  Lanes take one pat line each; a line stands for
//           `count` identical rows, so its log-likelihoods are computed once.  The column counts are integer atomics
//           (exact in any order).  Every sum the stopping test depends on is taken in the reference's order by the whole
//           wavefront in lock-step from shuffled values: ll0 over columns left to right, each cluster's new_ll over rows in
//           file order, one addition per row copy.  No float atomics, no trees.
//
// The arithmetic (tests/bimodal_ref.py restates it in Python; the build keeps -ffp-contract=off, divisions are IEEE):
//   ll0      c = 1e-3 + #C, t = 1e-3 + #T per column; sum over columns from 0.0 of #C * log2(c / (c + t)) + #T * log2(t / (c + t))
//   row ll   (-1.0 + sum of l_p_c[z] over the row's C columns, left to right) + sum of l_p_t[z] over its T columns
//   assign   z = 1 only when ll_1 > ll_0 (argmax: a tie goes to cluster 0)
//   new_ll   (sum of cluster-0 rows) + (sum of cluster-1 rows); the loop runs while new_ll - ll > 0 from ll = -inf and
//            returns the last new_ll; between passes p_c[z] = 1e-3 + C counts of cluster z, p_t likewise,
//            l_p = log2(p / (p_c + p_t)); the first pass uses p_c = {0.9, 0.1}, p_t = 1 - p_c.
#pragma once
#include "pat_kernels.h"
#include "bimodal_plan.h"      // WG_BIM_LDS_COLS, WG_BIM_COL_BYTES, WG_BIM_MAX_ITERS, WG_BIM_CTX, WG_BIM_NONE, wg_bim_state, wg_bim_meta

#define WG_BIM_WAVE 64
static_assert(WG_BIM_COL_BYTES == 4 * sizeof(double) + 4 * sizeof(uint32_t), "k_bim_em's lp | cn tables per column are what the host lays out in scratch");

// the reference's acceptance of a read for block [s1, s2) (read_pat_vis :35-56): false when skipped; else its clipped start / length
__device__ __forceinline__ bool wg_bim_accept(long long st, long long len, long long s1, long long s2, int strict, int min_len,
                                              long long& cs, long long& cl)
{
    if (st + len <= s1) return false;
    cs = st; cl = len;
    if (strict) {
        if (cs < s1) { cl -= s1 - cs; cs = s1; }
        if (cs + cl > s2) cl = s2 - cs;
    }
    return cl >= min_len;
}

// first index in [lo, hi) with a[i] >= v (a ascending)
__device__ __forceinline__ long long wg_bim_lower(const int32_t* a, long long lo, long long hi, long long v)
{
    while (lo < hi) {
        const long long m = (lo + hi) >> 1;
        if ((long long)a[m] < v) lo = m + 1; else hi = m;
    }
    return lo;
}

__device__ __forceinline__ uint32_t wg_bim_code(char c) { return c == 'C' ? 1u : (c == 'T' ? 2u : 0u); }

// What k_bim_em computes from a pair of column counts (a, b) = (#C, #T): pa = 1e-3 + a, pb = 1e-3 + b, n = pa + pb, the IEEE
// quotients pa / n and pb / n and their log2 (the between-pass tables l_p_c / l_p_t), and the column's ll0 term a * la + b * lb.
// k_bim_debug_terms (the test hook) evaluates the same function; tests/native/exact_host.cpp carries its host twin.
struct wg_bim_terms { double n, qa, qb, la, lb; };
__device__ __forceinline__ wg_bim_terms wg_bim_pair(uint32_t a, uint32_t b, const wg_d2* __restrict__ dt, const wg_d2* __restrict__ dt2)
{
    wg_bim_terms r;
    const double pa = 1e-3 + (double)a, pb = 1e-3 + (double)b;
    r.n = pa + pb;
    r.qa = pa / r.n;
    r.qb = pb / r.n;
    r.la = wg_log2(r.qa, dt, dt2);
    r.lb = wg_log2(r.qb, dt, dt2);
    return r;
}
__device__ __forceinline__ double wg_bim_ll0_term(uint32_t a, uint32_t b, const wg_bim_terms& r) { return (double)a * r.la + (double)b * r.lb; }

// Pass 1 over a chunk: per tile, the number of good lines and of their pattern words.  Malformed lines and negative counts
// are reported (lowest byte offset) and left out of the table (both kernels skip the same lines).
__global__ __launch_bounds__(WG_BLOCK) void k_bim_tile_count(const char* __restrict__ text, int64_t n, uint32_t* __restrict__ tile_cnt,
                                                             wg_bim_state* st, unsigned long long chunk_off)
{
    __shared__ PatTile tile;
    __shared__ uint32_t s_lines, s_words;
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * WG_PAT_TILE;
    if (tid == 0) { s_lines = 0; s_words = 0; }
    const uint32_t total = wg_pat_tile_lines(text, n, base, tile);    // (synchronises)
    const PatText T = tile.text(text, base, n);
    uint32_t lines = 0, words = 0;
    for (uint32_t l = (uint32_t)tid; l < total; l += WG_BLOCK) {
        const int64_t p = base + tile.lstart[l];
        int64_t site = 0, ps = 0, plen = 0, count = 0;
        if (!wg_pat_parse_line(T, p, n, site, ps, plen, count)) { atomicMin(&st->bad, chunk_off + (unsigned long long)p); continue; }
        if (count < 0) { atomicMin(&st->neg, chunk_off + (unsigned long long)p); continue; }
        lines += 1;
        words += (uint32_t)((plen + 15) >> 4);
    }
    lines = wg_wave_sum_u32(lines);
    words = wg_wave_sum_u32(words);
    if ((tid & 63) == 0) { atomicAdd(&s_lines, lines); atomicAdd(&s_words, words); }
    __syncthreads();
    if (tid == 0) { tile_cnt[2 * blockIdx.x] = s_lines; tile_cnt[2 * blockIdx.x + 1] = s_words; }
}

// Pass 2 (one workgroup): exclusive prefix of the tiles' counts on top of the table's R / W -> each tile's first row and word;
// the state's R / W then include the chunk.
__global__ __launch_bounds__(WG_BLOCK) void k_bim_tile_scan(const uint32_t* __restrict__ tile_cnt, int64_t n_tiles, long long* __restrict__ tile_base,
                                                            wg_bim_state* st)
{
    __shared__ unsigned long long wl[WG_BLOCK / 64], ww[WG_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long R = st->R, W = st->W;
    unsigned long long cl = (unsigned long long)R, cw = (unsigned long long)W;
    for (int64_t t0 = 0; t0 < n_tiles; t0 += WG_BLOCK) {
        const int64_t t = t0 + tid;
        const uint64_t a = t < n_tiles ? tile_cnt[2 * t] : 0u, b = t < n_tiles ? tile_cnt[2 * t + 1] : 0u;
        const uint64_t ia = wg_wave_incl_scan_u64(a, lane), ib = wg_wave_incl_scan_u64(b, lane);
        if (lane == 63) { wl[wv] = ia; ww[wv] = ib; }
        __syncthreads();
        unsigned long long pa = cl + ia - a, pb = cw + ib - b, ta = 0, tb = 0;
        for (int w = 0; w < WG_BLOCK / 64; w++) {
            if (w < wv) { pa += wl[w]; pb += ww[w]; }
            ta += wl[w]; tb += ww[w];
        }
        if (t < n_tiles) { tile_base[2 * t] = (long long)pa; tile_base[2 * t + 1] = (long long)pb; }
        cl += ta; cw += tb;
        __syncthreads();
    }
    if (tid == 0) { st->R0 = R; st->R = (long long)cl; st->W = (long long)cw; }
}

// Pass 3: the good lines of each tile into the table at the tile's rows / words (file order); pos[row - R0] = the line's byte offset
__global__ __launch_bounds__(WG_BLOCK) void k_bim_fill(const char* __restrict__ text, int64_t n, const long long* __restrict__ tile_base,
                                                       int32_t* __restrict__ r_start, int32_t* __restrict__ r_len, int32_t* __restrict__ r_cnt,
                                                       long long* __restrict__ r_woff, uint32_t* __restrict__ words, long long* __restrict__ pos,
                                                       const wg_bim_state* st, unsigned long long chunk_off)
{
    __shared__ PatTile tile;
    __shared__ uint32_t wl[WG_BLOCK / 64], ww[WG_BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t base = (int64_t)blockIdx.x * WG_PAT_TILE;
    const uint32_t total = wg_pat_tile_lines(text, n, base, tile);
    const PatText T = tile.text(text, base, n);
    const long long R0 = st->R0;
    long long row = tile_base[2 * blockIdx.x], word = tile_base[2 * blockIdx.x + 1];
    for (uint32_t r0 = 0; r0 < total; r0 += WG_BLOCK) {
        const uint32_t l = r0 + (uint32_t)tid;
        int64_t p = 0, site = 0, ps = 0, plen = 0, count = 0;
        bool ok = false;
        if (l < total) {
            p = base + tile.lstart[l];
            ok = wg_pat_parse_line(T, p, n, site, ps, plen, count) && count >= 0;
        }
        const uint32_t a = ok ? 1u : 0u, b = ok ? (uint32_t)((plen + 15) >> 4) : 0u;
        const uint32_t ia = wg_wave_incl_scan_dpp_u32(a), ib = wg_wave_incl_scan_dpp_u32(b);
        if (lane == 63) { wl[wv] = ia; ww[wv] = ib; }
        __syncthreads();
        uint32_t pa = ia - a, pb = ib - b, ta = 0, tb = 0;
        for (int w = 0; w < WG_BLOCK / 64; w++) {
            if (w < wv) { pa += wl[w]; pb += ww[w]; }
            ta += wl[w]; tb += ww[w];
        }
        if (ok) {
            const long long i = row + pa, w0 = word + pb;
            r_start[i] = (int32_t)site;
            r_len[i] = (int32_t)plen;
            r_cnt[i] = (int32_t)count;
            r_woff[i] = w0;
            pos[i - R0] = (long long)(chunk_off + (unsigned long long)p);
            for (int64_t k0 = 0; k0 < plen; k0 += 16) {
                uint32_t v = 0;
                const int64_t k1 = plen - k0 < 16 ? plen - k0 : 16;
                for (int64_t k = 0; k < k1; k++) v |= wg_bim_code(T.at(ps + k0 + k)) << (2 * k);
                words[w0 + (k0 >> 4)] = v;
            }
        }
        row += ta; word += tb;
        __syncthreads();                                          // (wl / ww reused by the next round)
    }
}

// Pass 4: starts never descend, within the chunk and from the previous chunk's last read; then the state's last start
__global__ __launch_bounds__(WG_BLOCK) void k_bim_order(const int32_t* __restrict__ r_start, const long long* __restrict__ pos, wg_bim_state* st,
                                                        long long prev_last, int64_t cap)
{
    const long long R0 = st->R0, R = st->R;
    const long long i = R0 + (long long)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (i - R0 >= cap || i >= R) return;
    const long long pv = i == R0 ? prev_last : (long long)r_start[i - 1];
    if (pv != WG_BIM_NONE && (long long)r_start[i] < pv) atomicMin(&st->desc, (unsigned long long)pos[i - R0]);
    if (i == R - 1) st->last_start = r_start[i];
}

// Per retired block (one wavefront each): its table rows, the reference's first_ind / max_ind, its column and row counts.
__global__ __launch_bounds__(WG_BIM_WAVE) void k_bim_gather(const int32_t* __restrict__ r_start, const int32_t* __restrict__ r_len,
                                                            const int32_t* __restrict__ r_cnt, const wg_bim_state* st,
                                                            const int32_t* __restrict__ bs1, const int32_t* __restrict__ bs2,
                                                            const int32_t* __restrict__ ids, int strict, int min_len, wg_bim_meta* __restrict__ meta)
{
    const int lane = threadIdx.x;
    const int32_t b = ids[blockIdx.x];
    const long long s1 = bs1[b], s2 = bs2[b], R = st->R;
    const long long lo_s = s1 - WG_BIM_CTX > 1 ? s1 - WG_BIM_CTX : 1;
    const long long ra = wg_bim_lower(r_start, 0, R, lo_s), rb = wg_bim_lower(r_start, ra, R, s2);     // start <= s2 - 1
    long long first = INT64_MAX, first_cs = 0, mx = 0;
    unsigned long long rows = 0, lines = 0;
    for (long long i = ra + lane; i < rb; i += WG_BIM_WAVE) {
        long long cs, cl;
        const long long s = r_start[i], len = r_len[i];
        if (!wg_bim_accept(s, len, s1, s2, strict, min_len, cs, cl)) continue;
        if (first == INT64_MAX) { first = i; first_cs = cs; }
        if (s + len > mx) mx = s + len;                           // max_ind: the end BEFORE clipping
        rows += (unsigned long long)r_cnt[i];
        lines += 1;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const long long of = __shfl_xor(first, o), ofc = __shfl_xor(first_cs, o), om = __shfl_xor(mx, o);
        if (of < first) { first = of; first_cs = ofc; }
        if (om > mx) mx = om;
        rows += __shfl_xor(rows, o);
        lines += __shfl_xor(lines, o);
    }
    if (lane == 0) {
        wg_bim_meta m;
        m.ra = ra; m.rb = rb; m.rows = (long long)rows; m.lines = (long long)lines;
        m.first_ind = first == INT64_MAX ? 0 : first_cs;
        m.ncols = first == INT64_MAX ? 0 : mx - first_cs;
        meta[blockIdx.x] = m;
    }
}

// the EM of one retired block per wavefront: res_f[b] = {ll0, ll_em, sum of n_per_col}, res_i[b] = {ncols, rows, iterations}
__global__ __launch_bounds__(WG_BIM_WAVE) void k_bim_em(const int32_t* __restrict__ r_start, const int32_t* __restrict__ r_len,
                                                        const int32_t* __restrict__ r_cnt, const long long* __restrict__ r_woff,
                                                        const uint32_t* __restrict__ words, const int32_t* __restrict__ bs1,
                                                        const int32_t* __restrict__ bs2, const int32_t* __restrict__ ids,
                                                        const wg_bim_meta* __restrict__ meta, const long long* __restrict__ scr_off,
                                                        unsigned char* __restrict__ scratch, int lds_cols, int strict, int min_len,
                                                        double* __restrict__ res_f, long long* __restrict__ res_i, wg_bim_state* st)
{
    __shared__ double s_lp[4 * WG_BIM_LDS_COLS];
    __shared__ uint32_t s_cn[4 * WG_BIM_LDS_COLS];
    const int lane = threadIdx.x;
    const int32_t b = ids[blockIdx.x];
    const long long ra = meta[blockIdx.x].ra, rb = meta[blockIdx.x].rb, first_ind = meta[blockIdx.x].first_ind;
    const long long nc = meta[blockIdx.x].ncols, rows = meta[blockIdx.x].rows;
    const long long s1 = bs1[b], s2 = bs2[b];
    if (rows == 0) {                                              // test_single_region: no rows -> p = 1, nothing computed
        if (lane == 0) {
            res_f[3 * b] = 0.0; res_f[3 * b + 1] = 0.0; res_f[3 * b + 2] = 0.0;
            res_i[3 * b] = nc; res_i[3 * b + 1] = 0; res_i[3 * b + 2] = 0;
        }
        return;
    }
    // tables: lp = {l_p_c[0], l_p_c[1], l_p_t[0], l_p_t[1]} x nc doubles, cn = {C[0], C[1], T[0], T[1]} x nc counts
    double* lp;
    uint32_t* cn;
    if (nc <= lds_cols) { lp = s_lp; cn = s_cn; }
    else {
        lp = reinterpret_cast<double*>(scratch + scr_off[blockIdx.x]);
        cn = reinterpret_cast<uint32_t*>(lp + 4 * nc);
    }
    const wg_d2* dt = g_wg_tables.d_tab;
    const wg_d2* dt2 = g_wg_tables.d_tab2;
    for (long long j = lane; j < 4 * nc; j += WG_BIM_WAVE) cn[j] = 0u;
    __syncthreads();
    // ---- column counts of all rows -> ll0 (calc_initial_liklihood :132-146).  A line's observations: the C / T sites of its
    // clipped pattern, left to right (site kk of the pattern: 2 bits at word kk / 16, slot kk % 16)
    for (long long i = ra + lane; i < rb; i += WG_BIM_WAVE) {
        long long cs, cl;
        if (!wg_bim_accept(r_start[i], r_len[i], s1, s2, strict, min_len, cs, cl)) continue;
        const uint32_t cnt = (uint32_t)r_cnt[i];
        if (cnt == 0u) continue;
        const long long k0 = cs - r_start[i], col0 = cs - first_ind, w0 = r_woff[i];
        for (long long k = 0; k < cl; k++) {
            const long long kk = k0 + k, col = col0 + k;
            const uint32_t c = (words[w0 + (kk >> 4)] >> (2 * (kk & 15))) & 3u;
            if (c && col >= 0 && col < nc) atomicAdd(&cn[(c == 1u ? 0 : 2) * nc + col], cnt);      // (always inside on an ordered table)
        }
    }
    __syncthreads();
    for (long long j = lane; j < nc; j += WG_BIM_WAVE) {
        const uint32_t C = cn[j], Tn = cn[2 * nc + j];
        const wg_bim_terms r = wg_bim_pair(C, Tn, dt, dt2);
        lp[j] = wg_bim_ll0_term(C, Tn, r);
        lp[nc + j] = r.n;
        cn[j] = 0u; cn[2 * nc + j] = 0u;
    }
    __syncthreads();
    double ll0 = 0.0, sum_n = 0.0;                                 // Python's sum from int 0, column by column (every lane alike)
    for (long long j = 0; j < nc; j++) { ll0 = ll0 + lp[j]; sum_n = sum_n + lp[nc + j]; }
    __syncthreads();
    // ---- EM (em_pat_matrix :72-130)
    {
        const double l09 = wg_log2(0.9, dt, dt2), l01 = wg_log2(0.1, dt, dt2);
        const double lt0 = wg_log2(1.0 - 0.9, dt, dt2), lt1 = wg_log2(1.0 - 0.1, dt, dt2);
        for (long long j = lane; j < nc; j += WG_BIM_WAVE) { lp[j] = l09; lp[nc + j] = l01; lp[2 * nc + j] = lt0; lp[3 * nc + j] = lt1; }
    }
    __syncthreads();
    double ll = -__builtin_inf();
    long long iters = 0;
    bool more = true;
    while (more) {
        iters += 1;
        double S0 = 0.0, S1 = 0.0;
        for (long long g = ra; g < rb; g += WG_BIM_WAVE) {
            const long long i = g + lane;
            long long cs = 0, cl = 0;
            uint32_t cnt = 0u;
            int z = 0;
            double lz = 0.0;
            if (i < rb && wg_bim_accept(r_start[i], r_len[i], s1, s2, strict, min_len, cs, cl)) {
                cnt = (uint32_t)r_cnt[i];
                const long long k0 = cs - r_start[i], col0 = cs - first_ind, w0 = r_woff[i];
                double c0 = 0.0, c1 = 0.0, t0 = 0.0, t1 = 0.0;
                for (long long k = 0; k < cl; k++) {
                    const long long kk = k0 + k, col = col0 + k;
                    const uint32_t c = (words[w0 + (kk >> 4)] >> (2 * (kk & 15))) & 3u;
                    if (!c || col < 0 || col >= nc) continue;
                    if (c == 1u) { c0 = c0 + lp[col]; c1 = c1 + lp[nc + col]; }
                    else { t0 = t0 + lp[2 * nc + col]; t1 = t1 + lp[3 * nc + col]; }
                }
                const double l0 = (-1.0 + c0) + t0, l1 = (-1.0 + c1) + t1;
                z = l1 > l0 ? 1 : 0;
                lz = z ? l1 : l0;
                if (cnt) {
                    for (long long k = 0; k < cl; k++) {
                        const long long kk = k0 + k, col = col0 + k;
                        const uint32_t c = (words[w0 + (kk >> 4)] >> (2 * (kk & 15))) & 3u;
                        if (c && col >= 0 && col < nc) atomicAdd(&cn[((c == 1u ? 0 : 2) + z) * nc + col], cnt);
                    }
                }
            }
            // the rows of these 64 lines in file order: every lane adds the same values in the same order
            const int nl = rb - g < WG_BIM_WAVE ? (int)(rb - g) : WG_BIM_WAVE;
            for (int k = 0; k < nl; k++) {
                const double v = __shfl(lz, k);
                const uint32_t c = (uint32_t)__shfl((int)cnt, k);
                if (__shfl(z, k)) { for (uint32_t q = 0; q < c; q++) S1 = S1 + v; }
                else { for (uint32_t q = 0; q < c; q++) S0 = S0 + v; }
            }
        }
        __syncthreads();
        const double nll = S0 + S1;
        more = nll - ll > 0.0;
        ll = nll;
        for (long long j = lane; j < nc; j += WG_BIM_WAVE) {
            for (int z = 0; z < 2; z++) {
                const wg_bim_terms r = wg_bim_pair(cn[z * nc + j], cn[(2 + z) * nc + j], dt, dt2);
                lp[z * nc + j] = r.la;
                lp[(2 + z) * nc + j] = r.lb;
                cn[z * nc + j] = 0u; cn[(2 + z) * nc + j] = 0u;
            }
        }
        __syncthreads();
        if (more && iters >= WG_BIM_MAX_ITERS) {
            if (lane == 0) atomicMax(&st->em_cap, (unsigned long long)b + 1ull);
            break;
        }
    }
    if (lane == 0) {
        res_f[3 * b] = ll0; res_f[3 * b + 1] = ll; res_f[3 * b + 2] = sum_n;
        res_i[3 * b] = nc; res_i[3 * b + 1] = rows; res_i[3 * b + 2] = iters;
    }
}

// test hook: wg_bim_pair / wg_bim_ll0_term on arrays of (a, b); out = six rows of `count` bit patterns: qa, qb, la, lb, n, the ll0 term
__global__ __launch_bounds__(WG_BLOCK) void k_bim_debug_terms(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, int64_t count,
                                                              uint64_t* __restrict__ out)
{
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < count; q += (int64_t)gridDim.x * blockDim.x) {
        const wg_bim_terms r = wg_bim_pair(a[q], b[q], g_wg_tables.d_tab, g_wg_tables.d_tab2);
        out[q] = wg_d2u(r.qa);
        out[count + q] = wg_d2u(r.qb);
        out[2 * count + q] = wg_d2u(r.la);
        out[3 * count + q] = wg_d2u(r.lb);
        out[4 * count + q] = wg_d2u(r.n);
        out[5 * count + q] = wg_d2u(wg_bim_ll0_term(a[q], b[q], r));
    }
}

// Dropping reads no pending block can reach: head = first row with start >= lo (one thread), then the live rows and their
// words move to the other table (k_bim_drop_copy, grid over the rows / words known before the drop), then the counts shrink.
__global__ void k_bim_drop_find(const int32_t* __restrict__ r_start, const long long* __restrict__ r_woff, wg_bim_state* st, long long lo)
{
    const long long R = st->R;
    const long long h = wg_bim_lower(r_start, 0, R, lo);
    st->head = h;
    st->whead = h < R ? r_woff[h] : st->W;
}

__global__ __launch_bounds__(WG_BLOCK) void k_bim_drop_copy(const int32_t* __restrict__ a_start, const int32_t* __restrict__ a_len,
                                                            const int32_t* __restrict__ a_cnt, const long long* __restrict__ a_woff,
                                                            const uint32_t* __restrict__ a_words, int32_t* __restrict__ b_start,
                                                            int32_t* __restrict__ b_len, int32_t* __restrict__ b_cnt,
                                                            long long* __restrict__ b_woff, uint32_t* __restrict__ b_words,
                                                            const wg_bim_state* st, long long rows_cap, long long words_cap)
{
    const long long R = st->R, W = st->W, h = st->head, wh = st->whead;
    const long long i = (long long)blockIdx.x * WG_BLOCK + threadIdx.x;
    if (i < rows_cap && h + i < R) {
        b_start[i] = a_start[h + i]; b_len[i] = a_len[h + i]; b_cnt[i] = a_cnt[h + i]; b_woff[i] = a_woff[h + i] - wh;
    }
    if (i < words_cap && wh + i < W) b_words[i] = a_words[wh + i];
}

__global__ void k_bim_drop_done(wg_bim_state* st)
{
    st->R -= st->head;
    st->W -= st->whead;
}
