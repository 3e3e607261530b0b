// vmp_hmm_seg_cat_dev.h -- sizes, splits and workspace of the segmented (time-parallel) chain pass
// of the fused hidden-Markov-model block with categorical emissions (csrc/vmp_hmm_seg_cat.hip).
// Host and device share these functions; g++ compiles this header for the host side of the C ABI
// (vmp_hmm_seg_cat_plan).
//
// The segments, the formulas, the ownership of the boundary steps and the order of the additions
// of the transfer, the scan and the sweep are those of vmp_hmm_seg_dev.h, with
// e_t[j] = <log P>[y_t][j] at an observed step whose word lies in [0, M) and 0 at every other step
// (vmp_hmm_fused_dev.h), and b_t = max_j e_t[j] read from a table of M maxima.  What the discrete
// form adds is the count
//
//   S[m][k] = sum over the observed (b, t) with y_bt = m of gamma_bt[k]
//
// which the sweep cannot hold (its four wavefronts would need 4 x 64 M doubles of LDS), so it is a
// kernel of its own over the flattened (b, t) plate, after the sweep has left gamma in place of
// la:
//   count     a workgroup (one wavefront) owns vmp_hmmsc_rows_per_wg(B, T, M, K) consecutive rows;
//             lane group g of its 64 / KP takes the rows g, g + 64 / KP, ... of the range in
//             ascending order; lane (g, k) adds gamma[row][k] to its private histogram
//             sacc[m * 64 + lane].  A chain without an observed step has no observed row, so the
//             chain weight does not enter.  The groups are added from zero in group order into
//             one M x K partial.
//   combine   one thread per output element adds the partials of the sweep (sum gamma_0, sum xi,
//             sum log Z, sum gamma . e) and of the count kernel in workgroup order.
// No atomics: the bits of every output depend on the inputs and (B, T, M, K, L) alone.
#pragma once

#include "vmp_hmm_seg_dev.h"

#define VMP_HMMSC_MAX_K VMP_HMMF_MAX_K
#define VMP_HMMSC_MAX_M VMP_HMMF_MAX_M
#define VMP_HMMSC_MAX_COUNT_WGS 512
#define VMP_HMMSC_MIN_ROWS 64             // rows of a workgroup of the count kernel, at least

// dynamic LDS in doubles: <log A>, one vector per lane, the table (M x KP), the maxima (M)
__host__ __device__ inline int64_t vmp_hmmsc_transfer_lds_doubles(int KP, int M)
{
    return (int64_t)KP * KP + 256 + (int64_t)M * KP + M;
}

// <log A>, its transpose, the la / u vectors of the four wavefronts, the table
__host__ __device__ inline int64_t vmp_hmmsc_sweep_lds_doubles(int KP, int M)
{
    return (int64_t)2 * KP * KP + 128 * VMP_HMMS_WAVES + (int64_t)M * KP;
}

// rows of a workgroup of the count kernel: a function of (B, T, M, K) alone; a multiple of the
// 64 / KP rows of a round, at most VMP_HMMSC_MAX_COUNT_WGS workgroups and 2^23 doubles of partials
__host__ __device__ inline int64_t vmp_hmmsc_rows_per_wg(int64_t B, int T, int M, int K)
{
    const int64_t groups = 64 / vmp_hmmf_kpad(K), R = B * (int64_t)T;
    int64_t maxw = ((int64_t)1 << 23) / ((int64_t)M * K);
    if (maxw > VMP_HMMSC_MAX_COUNT_WGS) maxw = VMP_HMMSC_MAX_COUNT_WGS;
    int64_t r = (R + maxw - 1) / maxw;
    if (r < VMP_HMMSC_MIN_ROWS) r = VMP_HMMSC_MIN_ROWS;
    return (r + groups - 1) / groups * groups;
}

__host__ __device__ inline int64_t vmp_hmmsc_count_wgs(int64_t B, int T, int M, int K)
{
    const int64_t r = vmp_hmmsc_rows_per_wg(B, T, M, K), R = B * (int64_t)T;
    return R > 0 ? (R + r - 1) / r : 0;
}

// workspace of the pass: the forward state that becomes gamma (B T K), the partials of the sweep
// and of the count kernel, 1024 doubles for the dot products, then log W (B S K KP), la at the
// segment starts and lb at the segment ends (B S KP each), the flag and the sum b of every segment
// (B S 2), the weight and log Z of every chain (B 2).  Not below the workspace of the sequential
// pass, which serves fixed labels.
__host__ __device__ inline int64_t vmp_hmmsc_workspace_doubles(int64_t B, int T, int M, int K, int L)
{
    const int64_t R = B * (int64_t)T, KP = vmp_hmmf_kpad(K), BS = B * vmp_hmms_segments(T, L);
    const int64_t n = R * K + vmp_hmms_sweep_wgs(B, T, K, L) * vmp_hmmw_chain_partial_doubles(K)
                      + vmp_hmmsc_count_wgs(B, T, M, K) * (int64_t)M * K + 1024
                      + BS * K * KP + 2 * BS * KP + 2 * BS + 2 * B;
    const int64_t seq = vmp_hmmf_cat_workspace_doubles(B, T, M, K);
    return n > seq ? n : seq;
}
