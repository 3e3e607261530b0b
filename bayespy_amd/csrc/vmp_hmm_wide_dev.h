// vmp_hmm_wide_dev.h -- shapes, splits and workspace of the wide-emission pass of the fused
// hidden-Markov-model block (csrc/vmp_hmm_wide.hip): Gaussian emissions with up to 32 dimensions.
// Host and device share these functions; g++ compiles this header for the host side of the C ABI
// (vmp_hmm_wide_plan) and for any host restatement.
//
// The recursion, its log-domain form and the order of its additions are those of
// vmp_hmm_fused_dev.h; its per-step functions are called from there, not restated.  What differs
// is where the emission term and the emission statistics are formed:
//
//   kernel 1  E[(b, t), k] = C_k . phi(y_bt) for every row of the flattened (b, t) plate, on the
//             fp64 matrix cores (v_mfma_f64_16x16x4f64): a wavefront owns a tile of 16 rows, the
//             compact features [y_a y_b (a <= b), y_d, 1] are expanded four at a time from the
//             rows' y in LDS as the A operand, C streams through LDS in chunks of
//             VMP_HMMW_C_CHUNK features.  A masked row has y = 0 before any product and E = 0;
//             a padded state k >= K has E = -inf.  E has row stride KP = vmp_hmmf_kpad(K).
//   kernel 2  the chain: KP lanes per chain, lane j owns column j; e_t[j] is one load from E.
//             gamma_t overwrites the forward state la_t in place.  A workgroup (one wavefront)
//             owns vmp_hmmw_chains_per_wg(B, K) consecutive chains and leaves one partial
//             [sum gamma_0 (K), sum xi (K x K), sum log Z, sum gamma . e].
//   kernel 3  T = Gamma^T [phi(y)] on the matrix cores, contracted over the rows.  Workgroup
//             (w, s) owns rows [w R_w, (w + 1) R_w) and feature slab s (VMP_HMMW_SLAB_TILES tiles
//             of 16 compact features); it adds its rows in ascending order, four per matrix
//             instruction, and leaves one partial.  Only the a <= b half of y y^T is formed.
//   combine   adds the partials of kernel 2 and kernel 3 in workgroup order and mirrors the
//             a <= b half into T_k = [sum gamma, sum gamma y, sum gamma y y^T].
// No atomics anywhere: the bits of every output depend on the inputs and (B, T, D, K) alone.
#pragma once

#include "vmp_hmm_fused_dev.h"

#define VMP_HMMW_MAX_K 64
#define VMP_HMMW_MAX_D 32
#define VMP_HMMW_C_CHUNK 32       // features of C resident in LDS at a time (kernel 1)
#define VMP_HMMW_ROWS 32          // rows staged per step of kernel 3
#define VMP_HMMW_SLAB_TILES 12    // 16-feature tiles of a slab: 4 wavefronts x 3 tiles
#define VMP_HMMW_MAX_ROW_WGS 1024

// LDS row stride of a 16 NT wide operand: rows 4 q + l4 of one matrix instruction in distinct banks
__host__ __device__ constexpr int hmmw_stride(int NT) { return (NT * 16) % 32 == 0 ? NT * 16 + 16 : NT * 16; }

// doubles the chain kernel leaves per workgroup: sum gamma_0, sum xi, sum log Z, sum gamma . e
__host__ __device__ inline int64_t vmp_hmmw_chain_partial_doubles(int K)
{
    return (int64_t)K + (int64_t)K * K + 2;
}

// chains of a workgroup of the chain kernel: a function of (B, K) alone; a multiple of the
// 64 / KP chains that share the wavefront, at most VMP_HMMF_MAX_WGS workgroups
__host__ __device__ inline int64_t vmp_hmmw_chains_per_wg(int64_t B, int K)
{
    const int64_t groups = 64 / vmp_hmmf_kpad(K);
    int64_t c = (B + VMP_HMMF_MAX_WGS - 1) / VMP_HMMF_MAX_WGS;
    c = (c + groups - 1) / groups * groups;
    if (c < groups) c = groups;
    return c;
}

__host__ __device__ inline int64_t vmp_hmmw_chain_wgs(int64_t B, int K)
{
    const int64_t c = vmp_hmmw_chains_per_wg(B, K);
    return B > 0 ? (B + c - 1) / c : 0;
}

// feature slabs of kernel 3
__host__ __device__ inline int vmp_hmmw_slabs(int D)
{
    const int tiles = (vmp_hmmf_nfeat(D) + 15) / 16;
    return (tiles + VMP_HMMW_SLAB_TILES - 1) / VMP_HMMW_SLAB_TILES;
}

// rows of a workgroup of kernel 3: a multiple of VMP_HMMW_ROWS, at most VMP_HMMW_MAX_ROW_WGS
// row ranges and 2^24 doubles of partials (K x NF per row range)
__host__ __device__ inline int64_t vmp_hmmw_rows_per_wg(int64_t R, int D, int K)
{
    int64_t maxw = ((int64_t)1 << 24) / ((int64_t)K * vmp_hmmf_nfeat(D));
    if (maxw > VMP_HMMW_MAX_ROW_WGS) maxw = VMP_HMMW_MAX_ROW_WGS;
    if (maxw < 1) maxw = 1;
    int64_t r = (R + maxw - 1) / maxw;
    r = (r + VMP_HMMW_ROWS - 1) / VMP_HMMW_ROWS * VMP_HMMW_ROWS;
    if (r < VMP_HMMW_ROWS) r = VMP_HMMW_ROWS;
    return r;
}

__host__ __device__ inline int64_t vmp_hmmw_row_wgs(int64_t R, int D, int K)
{
    const int64_t r = vmp_hmmw_rows_per_wg(R, D, K);
    return R > 0 ? (R + r - 1) / r : 0;
}

// workspace of the pass: E (B T KP), the forward state that becomes gamma (B T K), the partials
// of the chain kernel and of kernel 3, 1024 doubles for the dot products
__host__ __device__ inline int64_t vmp_hmmw_workspace_doubles(int64_t B, int T, int D, int K)
{
    const int64_t R = B * (int64_t)T;
    return R * vmp_hmmf_kpad(K) + R * K
           + vmp_hmmw_chain_wgs(B, K) * vmp_hmmw_chain_partial_doubles(K)
           + vmp_hmmw_row_wgs(R, D, K) * (int64_t)K * vmp_hmmf_nfeat(D) + 1024;
}

#ifdef __HIPCC__
// The plate-parallel stages as host calls (defined in vmp_hmm_wide.hip), for the passes that keep
// kernel 1, kernel 3 and the combine kernel and bring a chain stage of their own
// (vmp_hmm_seg.hip).  emit: E (R x KP) from Y, C and the mask; stats: vmp_hmmw_row_wgs(R, D, K)
// partials from the in-place gamma; combine: adds nwc chain partials of
// vmp_hmmw_chain_partial_doubles(K) doubles and the partials of stats in workgroup order, then
// forms scal[2] and scal[3] with dot_ws (1024 doubles).  chain: the chain stage (kernel 2) alone,
// for a pass with emission and statistics kernels of its own (vmp_hmm_mult.hip): E (B T x KP) or
// null, gamma left in aw (B T x K), vmp_hmmw_chain_wgs(B, K) partials in cpart.
struct vmp_ctx;
int32_t vmp_hmmw_emit(vmp_ctx *ctx, int64_t R, int D, int K, const double *Y, const double *C,
                      int ldc, const uint8_t *mask, double *E);
int32_t vmp_hmmw_chain(vmp_ctx *ctx, int64_t B, int T, int K, const double *E, const double *la0,
                       const double *lA, const int32_t *labels, const uint8_t *mask, double *aw,
                       double *cpart, double *gamma, double *z0, double *zz);
int32_t vmp_hmmw_stats(vmp_ctx *ctx, int64_t R, int D, int K, const double *Y, const double *gam,
                       const uint8_t *mask, double *spart);
int32_t vmp_hmmw_combine(vmp_ctx *ctx, int64_t nwc, int64_t nwr, int D, int K, const double *cpart,
                         const double *spart, const double *elog_a0, const double *elog_A,
                         double *dot_ws, double *z0sum, double *xisum, double *Tstat, double *scal);
#endif
