// vmp_hmm_diag_dev.h -- shapes, splits and workspace of the diagonal-Gaussian-emission pass of the
// fused hidden-Markov-model block (csrc/vmp_hmm_diag.hip): every time step carries D real numbers
// with one precision per dimension, y (B T, D) doubles, R = B T rows.
//
// The recursion, the chain kernel and its partial are those of vmp_hmm_wide_dev.h (kernel 2, used
// as it is, through vmp_hmmw_chain).  What this pass brings are the products over the flattened
// (b, t) plate on either side of it, with the tables of the diagonal-Gaussian mixture block
// (vmp_dgmm_tables): h = <tau><mu>, q = -1/2 <tau> (D x K), g[k] = sum_d (1/2 <log tau> - 1/2 <tau><mu^2>).
//
//   emission    E[(b, t), k] = g[k] + sum_d (y_d h[d, k] + y_d^2 q[d, k]): ONE contraction of length
//               2 D on the fp64 matrix cores (v_mfma_f64_16x16x4f64).  A workgroup of four
//               wavefronts owns 64 rows, a wavefront a tile of 16; dimensions go through LDS in
//               chunks of c = VMP_HMMD_D_CHUNK: the stacked table [h; q] of the chunk (2 c rows,
//               row stride hmmw_stride(NT)) and the y of the 64 rows.  A lane reads its 8 values of
//               a row and chunk once, squares them in registers and feeds y, then y^2, as
//               successive k-slices.  NT = ceil(KP / 16) accumulator tiles cover the
//               KP = vmp_hmmf_kpad(K) columns of E.  Order of the additions of an element: chunks
//               ascending; within a chunk the slices q = 0 .. c/4 - 1 of y (slice q holds the
//               dimensions 4 q .. 4 q + 3 of the chunk, added by the instruction), then the same
//               slices of y^2; g[k] last.  A masked row and a row past the plate have zeros for y
//               before any product (their y is never loaded) and E = 0; a padded state k >= K has
//               E = -inf.  A row of E is stored less its largest element over k < K (the terms
//               1/2 tau y^2 reach 1e5 for data far from 0, and the recursion would round there);
//               the sums of the shifts, one per wavefront, are added back to sum log Z and
//               sum gamma . e in a fixed order.
//   statistics  S1[d, k] = sum over the observed rows of y_d gamma_k, S2 the same with y_d^2,
//               Nk[k] = sum of gamma_k: workgroup (w, s) owns rows [w R_w, (w + 1) R_w) and
//               dimension slab s (VMP_HMMD_SLAB_TILES tiles of 16 dimensions, two per wavefront);
//               it stages VMP_HMMD_ROWS rows of y and of gamma per step (zeros for masked rows and
//               past the end), reads y once for both products (the square is formed in registers),
//               multiplies the transposed tile (16 dimensions x 4 rows) with gamma (4 rows x 16
//               states), adds its rows in ascending order and leaves one partial
//               [S1 (D x K), S2 (D x K), Nk (K)]; Nk comes from the slab 0 workgroups, one
//               thread per state, rows ascending.
//   combine     adds the chain partials and the partials of the statistics in workgroup order.
// No atomics anywhere: the bits of every output depend on the inputs and (B, T, D, K) alone.
#pragma once

#include "vmp_hmm_wide_dev.h"

#define VMP_HMMD_MAX_K 64
#define VMP_HMMD_MAX_D 1024
#define VMP_HMMD_D_CHUNK 32       // dimensions resident in LDS at a time (emission kernel)
#define VMP_HMMD_ROWS 16          // rows staged per step of the statistics kernel
#define VMP_HMMD_SLAB_TILES 8     // 16-dimension tiles of a slab: 4 wavefronts x 2 tiles
#define VMP_HMMD_MAX_ROW_WGS 1024
#define VMP_HMMD_MAX_EMIT_WGS 4096

// accumulator tiles of 16 states: every column of E is written, so KP and not K sets the number
__host__ __device__ inline int vmp_hmmd_state_tiles(int K) { return (vmp_hmmf_kpad(K) + 15) / 16; }

// workgroups of the emission kernel: one per block of 64 rows up to VMP_HMMD_MAX_EMIT_WGS, beyond
// that a workgroup takes every VMP_HMMD_MAX_EMIT_WGS-th block; a function of R alone
__host__ __device__ inline int64_t vmp_hmmd_emit_wgs(int64_t R)
{
    const int64_t nblk = (R + 63) / 64;
    return nblk < VMP_HMMD_MAX_EMIT_WGS ? nblk : VMP_HMMD_MAX_EMIT_WGS;
}

// dimension slabs of the statistics kernel
__host__ __device__ inline int vmp_hmmd_slabs(int D)
{
    const int tiles = (D + 15) / 16;
    return (tiles + VMP_HMMD_SLAB_TILES - 1) / VMP_HMMD_SLAB_TILES;
}

// doubles of one partial of the statistics kernel: S1, S2 (D x K each) and Nk (K)
__host__ __device__ inline int64_t vmp_hmmd_stat_doubles(int D, int K)
{
    return 2 * (int64_t)D * K + K;
}

// rows of a workgroup of the statistics kernel: a multiple of VMP_HMMD_ROWS, at most
// VMP_HMMD_MAX_ROW_WGS row ranges and 2^24 doubles of partials
__host__ __device__ inline int64_t vmp_hmmd_rows_per_wg(int64_t R, int D, int K)
{
    int64_t maxw = ((int64_t)1 << 24) / vmp_hmmd_stat_doubles(D, K);
    if (maxw > VMP_HMMD_MAX_ROW_WGS) maxw = VMP_HMMD_MAX_ROW_WGS;
    if (maxw < 1) maxw = 1;
    int64_t r = (R + maxw - 1) / maxw;
    r = (r + VMP_HMMD_ROWS - 1) / VMP_HMMD_ROWS * VMP_HMMD_ROWS;
    if (r < VMP_HMMD_ROWS) r = VMP_HMMD_ROWS;
    return r;
}

__host__ __device__ inline int64_t vmp_hmmd_row_wgs(int64_t R, int D, int K)
{
    const int64_t r = vmp_hmmd_rows_per_wg(R, D, K);
    return R > 0 ? (R + r - 1) / r : 0;
}

// workspace of the pass, in this order: E (B T KP), the forward state that becomes gamma (B T K),
// the partials of the chain kernel, the partials of the statistics kernel, the sums of the row
// shifts of E (4 per workgroup of the emission kernel), 1024 doubles for the dot products
__host__ __device__ inline int64_t vmp_hmmd_workspace_doubles(int64_t B, int T, int D, int K)
{
    const int64_t R = B * (int64_t)T;
    return R * vmp_hmmf_kpad(K) + R * K
           + vmp_hmmw_chain_wgs(B, K) * vmp_hmmw_chain_partial_doubles(K)
           + vmp_hmmd_row_wgs(R, D, K) * vmp_hmmd_stat_doubles(D, K) + 4 * vmp_hmmd_emit_wgs(R)
           + 1024;
}
