// array_kernels.h — the probe table (`wgbstools beta_to_450k`, wgbsseg_site_counts, wgbsseg_site_table): chosen sites of chosen
// resident samples as counts or as CSV text, formatted on the device ("Probe table").  Per slab of rows:
//
//   k_site_gather  one thread per cell (row, column): reads the counts of sample samples[column] at site site0[row] — one scattered
//                  read of 2 or 4 bytes, the only pass that touches the resident rows — and stores them as one packed 32-bit cell
//                  (meth | cov << 16) of the compact [rows][n_cols] table: consecutive threads store consecutive cells
//   k_site_len     one thread per FIELD (array_plan.h: n_cols + 1 per row, row-major): the field's byte length from the label table or
//                  the cell, summed per workgroup — 64-bit totals of bytes and of line ends
//   k_bed_scan     (bed_kernels.h, as it is) ONE workgroup turns the totals into every workgroup's first byte and the slab's totals
//   k_site_emit    the lengths again, a scan inside the workgroup, every thread formats its field into LDS at its offset, shifted by
//                  the low four bits of the workgroup's first byte; the copy out is aligned 16-byte LDS reads and global stores, byte
//                  stores only in the first and the last vector.  A field is at most WG_SITE_MAX_FIELD bytes, so every workgroup's
//                  text fits the stage: there is no other path.
//
// Plain C++ only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "bed_kernels.h"
#include "array_plan.h"

struct wg_gather_args {
    const uint8_t* betas;      // the resident rows
    int64_t pitch;             // bytes from one sample's row to the next
    const int64_t* site0;      // the site of every row of the launch
    const int32_t* samples;    // the sample of every column
    int64_t n_cells;           // rows x n_cols
    int32_t n_cols;
};

template <int ELEM>
__global__ __launch_bounds__(WG_SITE_BLOCK) void k_site_gather(wg_gather_args a, uint32_t* __restrict__ cells)
{
    const int64_t i = (int64_t)blockIdx.x * WG_SITE_BLOCK + threadIdx.x;
    if (i >= a.n_cells) return;
    int64_t row;
    if (a.n_cells <= 0x7fffffff) row = (int64_t)((uint32_t)i / (uint32_t)a.n_cols);       // (the same in every thread)
    else row = i / a.n_cols;
    const int32_t col = (int32_t)(i - row * a.n_cols);
    const int64_t site = a.site0[row];
    const uint8_t* r = a.betas + (int64_t)a.samples[col] * a.pitch;
    if (ELEM == 1) {
        const uint32_t w = reinterpret_cast<const uint16_t*>(r)[site];
        cells[i] = (w & 0xffu) | ((w >> 8) << 16);
    } else {
        cells[i] = reinterpret_cast<const uint32_t*>(r)[site];
    }
}

struct wg_site_args {
    const uint32_t* cells;     // the slab's cells, [rows][n_cols]
    const char* labels;        // the call's label bytes, from byte label_base of the caller's on
    const int64_t* label_off;  // the call's n_rows + 1 offsets, as the caller gave them
    int64_t label_base;
    int64_t first_row;         // the slab's first row
    int32_t n_fields;          // ... and its fields: rows x (n_cols + 1)
    int32_t n_cols;
    uint32_t min_cov;
};

// what a thread knows of its field
struct wg_site_field {
    uint32_t len;              // its bytes, separator included (0: no field)
    int32_t text_len;          // ... without the separator
    uint32_t q;                // a "%.3f" value: its thousandths
    int64_t label;             // field 0: where its bytes begin in `labels`; -1: a value
    uint32_t line_end;         // 1: the row's last field
};

__device__ __forceinline__ wg_site_field wg_site_read(const wg_site_args& a, uint32_t i)
{
    wg_site_field s = {};
    if (i >= (uint32_t)a.n_fields) return s;
    const uint32_t per = (uint32_t)a.n_cols + 1u;
    const uint32_t row = i / per, f = i - row * per;
    if (f == 0) {
        const int64_t lo = a.label_off[a.first_row + row], hi = a.label_off[a.first_row + row + 1];
        s.label = lo - a.label_base;
        s.text_len = (int32_t)(hi - lo);
    } else {
        const uint32_t w = a.cells[i - row - 1u];
        s.label = -1;
        s.text_len = wg_site_value(w & 0xffffu, w >> 16, a.min_cov, &s.q);
        s.line_end = f == (uint32_t)a.n_cols;
    }
    s.len = (uint32_t)s.text_len + 1u;
    return s;
}

// the field at dst (LDS): s.len bytes
__device__ __forceinline__ void wg_site_put(const wg_site_args& a, const wg_site_field& s, char* dst)
{
    if (s.label >= 0) {
        const char* src = a.labels + s.label;
        for (int j = 0; j < s.text_len; j++) dst[j] = src[j];
    } else {
        wg_site_value_put(dst, s.text_len, s.q);
    }
    dst[s.text_len] = s.line_end ? '\n' : ',';
}

__global__ __launch_bounds__(WG_SITE_BLOCK) void k_site_len(wg_site_args a, uint64_t* __restrict__ wg_bytes, uint64_t* __restrict__ wg_lines)
{
    __shared__ uint32_t waves_b[WG_SITE_BLOCK / 64], waves_l[WG_SITE_BLOCK / 64];
    const wg_site_field s = wg_site_read(a, blockIdx.x * WG_SITE_BLOCK + threadIdx.x);
    uint32_t bytes, lines;
    wg_bed_block_scan(s.len, waves_b, bytes);
    wg_bed_block_scan(s.line_end, waves_l, lines);
    if (threadIdx.x == 0) { wg_bytes[blockIdx.x] = bytes; wg_lines[blockIdx.x] = lines; }
}

__global__ __launch_bounds__(WG_SITE_BLOCK) void k_site_emit(wg_site_args a, const uint64_t* __restrict__ wg_base, char* __restrict__ out)
{
    __shared__ uint32_t waves[WG_SITE_BLOCK / 64];
    __shared__ __attribute__((aligned(16))) char stage[WG_SITE_STAGE_BYTES + 16];
    const wg_site_field s = wg_site_read(a, blockIdx.x * WG_SITE_BLOCK + threadIdx.x);
    uint32_t total;
    const uint32_t off = wg_bed_block_scan(s.len, waves, total);           // total <= WG_SITE_STAGE_BYTES: array_plan.h
    const uint64_t base = wg_base[blockIdx.x];
    const uint32_t pad = (uint32_t)(base & 15u);
    if (s.len) wg_site_put(a, s, stage + pad + off);
    __syncthreads();
    char* g = out + (base - pad);                                          // 16-byte aligned, like `out`
    const uint32_t end = pad + total;
    for (uint32_t lo = threadIdx.x * 16u; lo < end; lo += WG_SITE_BLOCK * 16u) {
        if (lo >= pad && lo + 16u <= end) {
            *reinterpret_cast<uint4*>(g + lo) = *reinterpret_cast<const uint4*>(stage + lo);
        } else {                                                           // the first and the last vector: their bytes inside [pad, end)
            const uint32_t j1 = lo + 16u < end ? lo + 16u : end;
            for (uint32_t j = lo > pad ? lo : pad; j < j1; j++) g[j] = stage[j];
        }
    }
}
