// vmp_bmm_dev.h -- per-row arithmetic of the Bernoulli-mixture pass (csrc/vmp_bmm.hip), shared
// with the host build of the CPU tests (tests/host/bmm_host.cpp).
//
// A row n of binary observations x_n (D bits, packed into ceil(D / 64) words, bit d of the row in
// bit d & 63 of word d >> 6, unused high bits zero) has the logits
//     l_k = c[k] + sum_d x_nd w[d, k],            k = 0 .. K-1,
// with w[d, k] = <log p_dk> - <log(1 - p_dk)> and c[k] = <log pi_k> + sum_d <log(1 - p_dk)>
// (mixture.py: the (N, D, K) broadcast of x <log p> + (1 - x) <log(1 - p)> summed over D plus the
// message of the Categorical parent).  Its responsibilities are r_k = exp(l_k - lse) with
// lse = m + log(sum_k exp(l_k - m)), m = max_k l_k (categorical.py: normalised exponential).
//
// A CONSTANT IS TAKEN OUT OF c.  r, and with it S, N_k and the entropy sum_n (lse_n - sum_k r_nk
// l_nk), do not change when the same number is added to every c[k]; vmp_bmm_tables subtracts
// max_k c[k].  A Dirichlet prior of 1e-5 (bmm.rst) has <log pi> near -1e5: left in, every lse
// would be rounded at that size (1.5e-11), sum_k r_nk would miss 1 by as much, and the entropy
// formed from sum lse - sum N_k c - sum S w would be off by 1e5 times that per row.  The reference
// subtracts <log pi> from the logits element by element before it multiplies by r and does not
// have the problem.  lse and sum lse are therefore relative to the constant taken out.
//
// ORDER OF THE ADDITIONS (what the host build restates):
//   * logit: starts at zero, adds w[d, k] for the set bits in ascending d (the matrix instruction
//     multiplies by the exact 0 / 1, so every step is one addition), and c[k] last: the order of
//     the reference, which sums over D and then adds the message of the Categorical parent;
//   * K is padded to KP = a multiple of 16 with -inf logits; the KP values of a row sit 16 to a
//     lane group, lane j holding columns j, j + 16, ...: the sum under the logarithm adds a lane's
//     columns in ascending order, then runs the butterfly (partner j ^ off, off = 8, 4, 2, 1);
//   * rows are walked in TILES of 64; row t of a tile belongs to SLOT (t / 16) * 4 + (t % 16) % 4
//     (wavefront, lane quarter).  N_k and sum lse are kept per slot in row order and the 16 slots
//     are added in slot order at the end of a CHUNK;
//   * S[k, d] adds r_k of the rows with bit d set in ascending row order through the chunk;
//   * a workgroup owns one chunk of vmp_bmm_chunk_rows(N, D, K) consecutive rows; the chunks'
//     partial S, N_k and sum lse are added in chunk order by a second kernel.
// The bits of every output therefore depend on the inputs and (N, D, K) only.
//
// Non-finite tables (a point mass at p0 = 0 or 1 gives w = +-inf and c = -inf) are OUTSIDE the
// contract: the reference forms 0 * (-inf) = NaN for them as well.  A logit of -inf (padding) gives
// r = 0 exactly.
//
// MISSING OBSERVATIONS (the *_masked entries).  A row carries two bit planes, 2 W words with
// W = ceil(D / 64): plane 0 = x & m in words 0 .. W-1, plane 1 = the mask m (1 = observed) in words
// W .. 2W-1, the unused high bits of both zero.  With xm = x & m
//     l_k = c[k] + sum_d xm_nd w[d, k] + sum_d m_nd l0[d, k],    l0[d, k] = <log(1 - p_dk)>,
//     c[k] = <log pi_k> - max_k <log pi_k>                       (sum_d l0 is no longer in c),
//     S_dk = sum_n r_nk xm_nd,  M_dk = sum_n r_nk m_nd,  counts = (S, M - S),
// the masked broadcast of mixture.py summed over D.  A hidden position is never interpreted: any
// value, NaN included, may stand there (the reference checks hidden values as well and raises for
// them).  A ROW WITH NO OBSERVED BIT has r = softmax(c), which is written to r_out when asked for
// (with labels: the one-hot row), and adds exactly nothing to N_k, sum lse, S and M: the reference
// masks the row out of the message of Z to R and out of the bound term of Z.
// Order of the additions of the masked pass:
//   * logit: starts at zero, adds w[d, k] for the set bits of plane 0 in ascending d, then l0[d, k]
//     for the set bits of plane 1 in ascending d, and c[k] last;
//   * the sum under the logarithm, the slots of N_k and sum lse (observed rows only) and the chunks
//     as above;
//   * S[k, d] adds r_k of the rows with bit d of plane 0 set, M[k, d] of those with bit d of plane
//     1 set, in two levels: within a tile of 64 rows from zero in ascending row order, and the
//     tiles' sums in tile order to the running sum of the chunk.  (The unmasked pass adds row by
//     row through the chunk; with few distinct rows, as a small D gives, the equal terms of such
//     a sum round the same way hundreds of times in a row.  At (N, D, K) = (300, 1, 5) that put
//     S . w + M . l0 at 1.27 times its allowance; in two levels it is at 0.23 of it.);
//   * the chunks' partial S, M, N_k and sum lse are added in chunk order by a second kernel.
#pragma once

#include <stdint.h>

#define VMP_BMM_MAX_K 64
#define VMP_BMM_MAX_D 1024
#define VMP_BMM_MASKED_MAX_K 64   // the masked pass: the same limits
#define VMP_BMM_MASKED_MAX_D 1024
#define VMP_BMM_TILE 64           // rows per tile: 16 per wavefront of a four-wavefront workgroup
#define VMP_BMM_MIN_CHUNK 256
#define VMP_BMM_MAX_CHUNKS 1024
#define VMP_BMM_DBLOCK 256        // columns of S one workgroup holds in accumulators at a time

__host__ __device__ inline int vmp_bmm_kpad(int K) { return (K + 15) & ~15; }

__host__ __device__ inline int vmp_bmm_words(int D) { return (D + 63) >> 6; }

// doubles one chunk leaves behind: S (K x D), N_k (K), sum lse (1)
__host__ __device__ inline int64_t vmp_bmm_partial_doubles(int D, int K)
{
    return (int64_t)D * K + K + 1;
}

// rows of a chunk: a function of (N, D, K) alone.  At most VMP_BMM_MAX_CHUNKS chunks and at most
// 2^25 doubles (256 MB) of partials; a multiple of the tile, at least VMP_BMM_MIN_CHUNK.
__host__ __device__ inline int64_t vmp_bmm_chunk_rows(int64_t N, int D, int K)
{
    int64_t maxc = ((int64_t)1 << 25) / vmp_bmm_partial_doubles(D, K);
    if (maxc > VMP_BMM_MAX_CHUNKS) maxc = VMP_BMM_MAX_CHUNKS;
    if (maxc < 1) maxc = 1;
    int64_t rows = (N + maxc - 1) / maxc;
    rows = (rows + VMP_BMM_TILE - 1) / VMP_BMM_TILE * VMP_BMM_TILE;
    if (rows < VMP_BMM_MIN_CHUNK) rows = VMP_BMM_MIN_CHUNK;
    return rows;
}

__host__ __device__ inline int64_t vmp_bmm_chunks(int64_t N, int D, int K)
{
    const int64_t rows = vmp_bmm_chunk_rows(N, D, K);
    return N > 0 ? (N + rows - 1) / rows : 0;
}

// the masked pass: S (K x D), M (K x D), N_k (K), sum lse (1) per chunk, under the same caps
__host__ __device__ inline int64_t vmp_bmm_partial_doubles_masked(int D, int K)
{
    return 2 * (int64_t)D * K + K + 1;
}

__host__ __device__ inline int64_t vmp_bmm_chunk_rows_masked(int64_t N, int D, int K)
{
    int64_t maxc = ((int64_t)1 << 25) / vmp_bmm_partial_doubles_masked(D, K);
    if (maxc > VMP_BMM_MAX_CHUNKS) maxc = VMP_BMM_MAX_CHUNKS;
    if (maxc < 1) maxc = 1;
    int64_t rows = (N + maxc - 1) / maxc;
    rows = (rows + VMP_BMM_TILE - 1) / VMP_BMM_TILE * VMP_BMM_TILE;
    if (rows < VMP_BMM_MIN_CHUNK) rows = VMP_BMM_MIN_CHUNK;
    return rows;
}

__host__ __device__ inline int64_t vmp_bmm_chunks_masked(int64_t N, int D, int K)
{
    const int64_t rows = vmp_bmm_chunk_rows_masked(N, D, K);
    return N > 0 ? (N + rows - 1) / rows : 0;
}

// whether any bit of the mask plane (W words) of a row is set
__host__ __device__ inline bool vmp_bmm_row_observed(const uint64_t *mask_words, int W)
{
    uint64_t any = 0;
    for (int i = 0; i < W; ++i) any |= mask_words[i];
    return any != 0;
}

// slot of row t (0 .. 63) of a tile
__host__ __device__ inline int vmp_bmm_slot(int t) { return (t >> 4) * 4 + (t & 3); }

// bit d of a packed row as the 0 / 1 operand of the products
__host__ __device__ inline double vmp_bmm_bit(const uint64_t *row_words, int d)
{
    return (double)((row_words[d >> 6] >> (d & 63)) & 1u);
}

// one step of the logit: x is exactly 0 or 1
__host__ __device__ inline double vmp_bmm_logit_step(double logit, double x, double w_dk)
{
    return logit + x * w_dk;
}

// the column's constant, added last
__host__ __device__ inline double vmp_bmm_logit_finish(double sum_xw, double c_k)
{
    return sum_xw + c_k;
}

// exp(l - m) of the sum under the logarithm; m is the row's maximum, so the argument is <= 0
__host__ __device__ inline double vmp_bmm_shifted_exp(double logit, double m)
{
    return exp(logit - m);
}

__host__ __device__ inline double vmp_bmm_lse(double m, double s) { return m + log(s); }

__host__ __device__ inline double vmp_bmm_resp(double logit, double lse) { return exp(logit - lse); }

#ifndef __HIPCC__
// the butterfly of a 16-lane group over v[0 .. 15]; every element ends with the result
inline void vmp_bmm_group_sum_host(double *v)
{
    double t[16];
    for (int off = 8; off > 0; off >>= 1) {
        for (int l = 0; l < 16; ++l) t[l] = v[l] + v[l ^ off];
        for (int l = 0; l < 16; ++l) v[l] = t[l];
    }
}
#endif
