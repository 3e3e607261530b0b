// vmp_hmm_mult_dev.h -- shapes, splits and workspace of the multinomial-emission pass of the fused
// hidden-Markov-model block (csrc/vmp_hmm_mult.hip): every time step carries a vector of counts
// over M categories, kept as one uint16 per entry (the pack of vmp_mmm_pack), R = B T rows.
//
// The recursion, the chain kernel and its partial are those of vmp_hmm_wide_dev.h (kernel 2, used
// as it is).  What this pass brings are the two products over the flattened (b, t) plate:
//
//   emission    E[(b, t), k] = sum_m x_{bt,m} <log P>[m, k] on the fp64 matrix cores
//               (v_mfma_f64_16x16x4f64).  A workgroup of four wavefronts owns 64 rows, a wavefront
//               a tile of 16; words go through LDS in chunks of VMP_HMMM_W_CHUNK: the rows' counts
//               as uint16 (widened to double on the way into the instruction, which is exact) and
//               the word-major table with row stride hmmw_stride(NT).  NT = ceil(KP / 16)
//               accumulator tiles cover the KP = vmp_hmmf_kpad(K) columns of E.  A masked row has
//               zeros for counts before any product and E = 0; a padded state k >= K has E = -inf.
//               A row of E is stored less its largest element c over the states, which keeps the
//               sums of the chain recursion near 0 where states compete (e itself is of the order
//               of -1000 for counts in the hundreds); the sums of c, one per wavefront, are added
//               back to sum log Z and sum gamma . e in a fixed order.
//   statistics  S[m, k] = sum over the observed rows of x_m gamma_k: workgroup (w, s) owns rows
//               [w R_w, (w + 1) R_w) and word slab s (VMP_HMMM_SLAB_TILES tiles of 16 words, two
//               per wavefront); it stages VMP_HMMM_ROWS rows of counts and of gamma per step
//               (zeros for masked rows and past the end), multiplies the transposed count tile
//               (16 words x 4 rows) with gamma (4 rows x 16 states), adds its rows in ascending
//               order and leaves one partial of its slab, word-major like S.
//   combine     adds the chain partials and the partials of S in workgroup order.
// No atomics anywhere: the bits of every output depend on the inputs and (B, T, M, K) alone.
#pragma once

#include "vmp_hmm_wide_dev.h"

#define VMP_HMMM_MAX_K 64
#define VMP_HMMM_MAX_M 1024
#define VMP_HMMM_MAX_COUNT 65534
#define VMP_HMMM_W_CHUNK 64       // words resident in LDS at a time (emission kernel)
#define VMP_HMMM_ROWS 32          // rows staged per step of the statistics kernel
#define VMP_HMMM_SLAB_TILES 8     // 16-word tiles of a slab: 4 wavefronts x 2 tiles
#define VMP_HMMM_MAX_ROW_WGS 1024
#define VMP_HMMM_MAX_EMIT_WGS 4096

// accumulator tiles of 16 states: every column of E is written, so KP and not K sets the number
__host__ __device__ inline int vmp_hmmm_state_tiles(int K) { return (vmp_hmmf_kpad(K) + 15) / 16; }

// workgroups of the emission kernel: one per block of 64 rows up to VMP_HMMM_MAX_EMIT_WGS, beyond
// that a workgroup takes every VMP_HMMM_MAX_EMIT_WGS-th block; a function of R alone
__host__ __device__ inline int64_t vmp_hmmm_emit_wgs(int64_t R)
{
    const int64_t nblk = (R + 63) / 64;
    return nblk < VMP_HMMM_MAX_EMIT_WGS ? nblk : VMP_HMMM_MAX_EMIT_WGS;
}

// word slabs of the statistics kernel
__host__ __device__ inline int vmp_hmmm_slabs(int M)
{
    const int tiles = (M + 15) / 16;
    return (tiles + VMP_HMMM_SLAB_TILES - 1) / VMP_HMMM_SLAB_TILES;
}

// rows of a workgroup of the statistics kernel: a multiple of VMP_HMMM_ROWS, at most
// VMP_HMMM_MAX_ROW_WGS row ranges and 2^24 doubles of partials (M x K per row range)
__host__ __device__ inline int64_t vmp_hmmm_rows_per_wg(int64_t R, int M, int K)
{
    int64_t maxw = ((int64_t)1 << 24) / ((int64_t)M * K);
    if (maxw > VMP_HMMM_MAX_ROW_WGS) maxw = VMP_HMMM_MAX_ROW_WGS;
    if (maxw < 1) maxw = 1;
    int64_t r = (R + maxw - 1) / maxw;
    r = (r + VMP_HMMM_ROWS - 1) / VMP_HMMM_ROWS * VMP_HMMM_ROWS;
    if (r < VMP_HMMM_ROWS) r = VMP_HMMM_ROWS;
    return r;
}

__host__ __device__ inline int64_t vmp_hmmm_row_wgs(int64_t R, int M, int K)
{
    const int64_t r = vmp_hmmm_rows_per_wg(R, M, K);
    return R > 0 ? (R + r - 1) / r : 0;
}

// workspace of the pass: E (B T KP), the forward state that becomes gamma (B T K), the partials
// of the chain kernel and of the statistics kernel, the sums of the row shifts of E (4 per
// workgroup of the emission kernel), 1024 doubles for the dot products
__host__ __device__ inline int64_t vmp_hmmm_workspace_doubles(int64_t B, int T, int M, int K)
{
    const int64_t R = B * (int64_t)T;
    return R * vmp_hmmf_kpad(K) + R * K
           + vmp_hmmw_chain_wgs(B, K) * vmp_hmmw_chain_partial_doubles(K)
           + vmp_hmmm_row_wgs(R, M, K) * (int64_t)M * K + 4 * vmp_hmmm_emit_wgs(R) + 1024;
}

#ifdef __HIPCC__
// The stages of the pass as one host call (defined in vmp_hmm_mult.hip) around a chain stage with
// the arguments of vmp_hmmw_chain that leaves nwc partials: vmp_hmm_mult_pass gives
// vmp_hmmw_chain, the wide-state pass (vmp_hmm_states.hip, K <= 128) its own.  The arguments are
// checked by the caller; ws is laid out as E (R KP), gamma (R K), nwc chain partials, the
// partials of S, the shifts, 1024 doubles.
typedef int32_t (*vmp_hmmm_chain_fn)(vmp_ctx *, int64_t, int, int, const double *, const double *,
                                     const double *, const int32_t *, const uint8_t *, double *,
                                     double *, double *, double *, double *);
int32_t vmp_hmmm_stages(vmp_ctx *ctx, int64_t B, int T, int M, int K, int64_t nwc,
                        vmp_hmmm_chain_fn chain, const uint16_t *x_packed, const double *elogPt,
                        const double *elog_a0, const double *elog_A, const int32_t *labels,
                        const uint8_t *mask, double *ws, double *z0sum, double *xisum, double *S,
                        double *scal, double *gamma, double *z0, double *zz);
#endif
