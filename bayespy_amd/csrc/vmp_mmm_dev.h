// vmp_mmm_dev.h -- arithmetic of the multinomial-mixture block (csrc/vmp_mmm.hip), shared with the
// host build of the CPU tests (tests/host/mmm_host.cpp).  vmp_digamma, vmp_lgamma and vmp_lgamma_dd
// (vmp_common.h) are declared before this header is included.
//
//     R = Dirichlet(a);  Z = Categorical(R, plates=(N,))
//     P = Dirichlet(a0, plates=(K,)) over M words;  X = Mixture(Z, Multinomial, n, P);  X.observe(x)
//
// A row of counts x_n (M entries that add up to n_n) has the logits
//     l_k = c[k] + sum_m x_nm L[m, k],      L[m, k] = <log p_km> - <log p_0m>,  c = <log pi> - max
// The multinomial coefficient lgamma(n_n + 1) - sum_m lgamma(x_nm + 1) is the same for every k and
// never enters the logits; the pack sums it once (lcoef).  There is no rate term: where the Poisson
// block has c = <log pi> - sum_d <lam>, c is <log pi> alone here, and the parameter table is K
// Dirichlet rows of M entries, not D K Gammas.  The statistics are S[k, m] = sum_n r_nk x_nm, ROW
// PER CLUSTER so that one strided Dirichlet call (rows K, row stride M, column stride 1) updates P,
// and N_k.
//
// x IS KEPT AS 16 BITS PER ENTRY (vmp_pmm_dev.h: vmp_pmm_pack_f64 / vmp_pmm_pack_i64, the largest
// count VMP_PMM_MAX_COUNT).  Nothing is hidden in this block: an entry that fails a check is packed
// as zero and raises a flag, and the caller does not run the pass on such data.
//
// THE TABLE OF THE PASS IS CENTRED: cluster 0 is taken out of every word's row.  That moves every
// logit of a row n by sum_m x_nm <log p_0m>, so r does not change, and sum lse and scal[2] = S . L
// move by the same sum, so the entropy sum lse - N_k . c - scal[2] does not change either; the
// logits are sums of differences between clusters instead of n_n log-probabilities.  c needs no
// term of the table for that and is <log pi> less its largest element.  The bound term of X needs
// the table as it is: the plan takes S . <log p> from its own (K x M) table.
//
// ORDER OF THE ADDITIONS (what the host build restates):
//   * logit: starts at zero; the words are walked in steps of 4, the four x L of a step in
//     ascending m, one matrix instruction; c[k] last;
//   * softmax, slots, tiles of 64 rows and chunks as in vmp_pmm_dev.h: K is padded to a multiple of
//     16 with -inf logits, lane j of a 16-lane group adds its columns j, j + 16, ... in ascending
//     order and the butterfly follows; N_k and sum lse per slot in row order, the 16 slots in slot
//     order at the end of a chunk; r_k = exp(l_k - m) / s with the very exponentials of the sum s;
//   * S in two levels: within a tile of 64 rows from zero in ascending row order, the tiles' sums
//     in tile order to the running sum of the chunk;
//   * a workgroup owns one chunk of vmp_pmm_chunk_rows(N, M, K) consecutive rows; the partials are
//     added in chunk order by a second kernel;
//   * scal[1] = N_k . c in ascending k; scal[2] = S . L: element e = k M + m belongs to thread
//     e % 256, which adds its products in ascending e; the 256 sums are halved eight times;
//   * pack: block b of vmp_pmm_pack_blocks(N) owns the ROWS [b span, (b + 1) span),
//     span = vmp_pmm_pack_span(N); thread t takes its rows b span + t + 256 i in ascending i and adds,
//     per row, lgamma(n + 1) and then -lgamma(x_m + 1) in ascending m, keeping the rounding errors
//     of the additions (vmp_pmm_sum_add); the 256 sums are halved eight times; the blocks'
//     partials are added in block order, again with their rounding errors kept.
// The bits of every output therefore depend on the packed x, n, the tables and (N, M, K) only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vmp_pmm_dev.h"

#define VMP_MMM_MAX_K VMP_PMM_MAX_K
#define VMP_MMM_MAX_M VMP_PMM_MAX_D
#define VMP_MMM_MAX_COUNT VMP_PMM_MAX_COUNT
#define VMP_MMM_TILE VMP_PMM_TILE
#define VMP_MMM_NT VMP_PMM_NT
#define VMP_MMM_MBLOCK VMP_PMM_DBLOCK  // words a workgroup holds at a time

// flags of the pack (four int32): the three of vmp_pmm_dev.h, then a row whose counts do not add
// up to its number of trials
#define VMP_MMM_BAD_SUM 8

// doubles one chunk leaves behind: S (K x M), N_k (K), sum lse (1)
__host__ __device__ inline int64_t vmp_mmm_partial_doubles(int M, int K)
{
    return (int64_t)M * K + K + 1;
}

// rows of a chunk and their number: those of the Poisson block at the same shape
__host__ __device__ inline int64_t vmp_mmm_chunk_rows(int64_t N, int M, int K)
{
    return vmp_pmm_chunk_rows(N, M, K);
}

__host__ __device__ inline int64_t vmp_mmm_chunks(int64_t N, int M, int K)
{
    return vmp_pmm_chunks(N, M, K);
}

// doubles of workspace: the partials; never less than the pack needs
__host__ __device__ inline int64_t vmp_mmm_workspace_doubles(int64_t N, int M, int K)
{
    const int64_t w = vmp_mmm_chunks(N, M, K) * vmp_mmm_partial_doubles(M, K);
    return w > VMP_PMM_PACK_BLOCKS ? w : VMP_PMM_PACK_BLOCKS;
}

// lgamma(n + 1) of a number of trials (at most M counts of VMP_MMM_MAX_COUNT); exactly zero for
// 0 and 1, the rule of vmp_pmm_lgamma1 above
__host__ __device__ inline double vmp_mmm_lgamma1_trials(int64_t n)
{
    if (n < 2) return 0.0;
    if (n <= 20) {
        uint64_t f = 2;
        for (int64_t i = 3; i <= n; ++i) f *= (uint64_t)i;
        return log((double)f);
    }
    double lo;
    return vmp_lgamma_dd((double)n + 1.0, 0.0, &lo);
}

// the 16 bits of one entry: one that fails a check becomes zero and sets bits of *bad
__host__ __device__ inline uint16_t vmp_mmm_entry(uint16_t packed)
{
    return packed == VMP_PMM_HIDDEN ? (uint16_t)0 : packed;
}

// whether a row's counts, all of them valid, miss its number of trials
__host__ __device__ inline bool vmp_mmm_sum_mismatch(int64_t sum, int64_t trials, int bad_row)
{
    return bad_row == 0 && sum != trials;
}

// an entry of the table of the pass: cluster 0 of the word taken out
__host__ __device__ inline double vmp_mmm_table(double v, double v0) { return v - v0; }
