// vmp_lda_hyper_dev.h -- layout, element arithmetic and order of additions of the statistics pass
// that the latent-Dirichlet-allocation block runs for a learnt concentration
// (csrc/vmp_lda_hyper.hip), shared with the host build of the CPU tests
// (tests/host/lda_hyper_host.cpp).  Include after vmp_common.h (vmp_two_sum, vmp_lgamma_dd,
// vmp_digamma).
//
// For rows x cols Dirichlet rows with parameters alpha and moments elog = <log p> the pass forms
//     S[c]  = sum_rows elog[r, c]                                        (cols doubles)
//     qterm = sum_rows ( lgamma(sum_c alpha_rc) - sum_c lgamma(alpha_rc) + sum_c (alpha_rc - 1) elog_rc )
// S is the Dirichlets' message to their concentration; qterm is the part of the node's lower-bound
// term that does not depend on the prior.
//
// qterm is a small number left over by terms that can be 1e7 each (lgamma of a large alpha and of
// the row sum), so everything that enters it is kept as an unevaluated sum hi + lo (vmp_dd): the
// product alpha * elog with its rounding error (fma), lgamma as vmp_lgamma_dd from 10 upwards (the
// math library's below, where the value is small), the row sums of alpha, and every accumulation
// (vmp_dd_add: Knuth's two-sum, the errors collected in lo).  Only the last addition rounds.
//
// Both memory forms of the block are M memory rows of W <= 1024 contiguous doubles:
//   tall        element (r, c) at r * cols + c       M = rows, W = cols   (p_topic, D x K)
//   transposed  element (r, c) at r + c * rows       M = cols, W = rows   (p_word kept as V x K)
// One wavefront owns a CHUNK of consecutive memory rows; lane j holds the positions w = j + 64 i,
// i = 0 .. R-1, R = the smallest of {1, 2, 4, 8, 16} with 64 R >= W.  Per memory row one quantity
// is summed ALONG the row (in lane over i ascending, then a 64-lane butterfly, partner lane ^ 32,
// ^ 16, .. ^ 1) and one is added DOWN the chunk per (lane, i), in row order:
//   tall        along: alpha (hi + lo) -> lgamma of the row sum;   down: elog (plain) -> S
//   transposed  along: elog (plain) -> S[c], complete;             down: alpha (hi + lo) -> row sums
// Every lane also adds the terms of its elements (vmp_lda_hyper_q_add) in the order i ascending.
// Tall: the 64 sums of one row go through the butterfly, lgamma of the row sum joins them, and the
// row terms add up in row order to the chunk's scalar.  Transposed: the lanes keep adding down the
// chunk and the chunk's scalar is the butterfly of the 64 sums; lgamma of the row sums joins in the
// combine.
//
// The combine adds the chunks' `down` partials per position: VMP_LDA_HYPER_GROUPS slices of
// consecutive chunks, each added in chunk order, then the slices in slice order.  The scalars are
// added by one workgroup: 1024 strided sums, the 64 of a wavefront folded by halves (lane l += lane
// l + off, off = 32 .. 1), the 16 wavefronts in order; qterm = hi + lo of that total.  The chunk size
// is a function of M alone, so the bits of both outputs depend on the inputs and the shape only.
#pragma once
#include "vmp_lda_dev.h"

#define VMP_LDA_HYPER_MAX_W 1024
#define VMP_LDA_HYPER_LANES 64
#define VMP_LDA_HYPER_GROUPS 16
#define VMP_LDA_HYPER_RED_NT 1024

// registers per lane: the smallest of {1, 2, 4, 8, 16} with 64 R >= W (W <= 1024)
__host__ __device__ inline int vmp_lda_hyper_regs(int W)
{
    int r = 1;
    while (r < 16 && VMP_LDA_HYPER_LANES * r < W) r <<= 1;
    return r;
}

// memory rows one wavefront walks in order: a function of M alone (vmp_lda_chunk_tokens with 64
// lanes per chunk: the smallest power of two from 16 to 256 that keeps M / chunk * 64 <= 2^17)
__host__ __device__ inline int vmp_lda_hyper_chunk_rows(int64_t M)
{
    return vmp_lda_chunk_tokens(M, VMP_LDA_HYPER_LANES);
}

__host__ __device__ inline int64_t vmp_lda_hyper_chunks(int64_t M)
{
    const int T = vmp_lda_hyper_chunk_rows(M);
    return M > 0 ? (M + T - 1) / T : 0;
}

// chunks per slice of the combine
__host__ __device__ inline int64_t vmp_lda_hyper_slice(int64_t nchunks)
{
    return (nchunks + VMP_LDA_HYPER_GROUPS - 1) / VMP_LDA_HYPER_GROUPS;
}

// doubles of the workspace: the scalars ([nchunks] chunk scalars and [W] lgamma of the row sums of
// the transposed form) as a hi array and a lo array, then the `down` partials [nchunks x W], twice
// (hi, lo; the tall form uses the first)
__host__ __device__ inline int64_t vmp_lda_hyper_ws_doubles(int64_t M, int W)
{
    const int64_t nc = vmp_lda_hyper_chunks(M);
    return 2 * (nc + W) + 2 * nc * W;
}

// an unevaluated sum hi + lo
struct vmp_dd {
    double hi, lo;
};

// a += x: the rounding error of the addition joins lo
__host__ __device__ inline void vmp_dd_add(vmp_dd &a, double x)
{
    double e;
    a.hi = vmp_two_sum(a.hi, x, &e);
    a.lo += e;
}

// a += b, the same bits whichever of the two is `a` (the butterflies rely on it)
__host__ __device__ inline void vmp_dd_add_dd(vmp_dd &a, const vmp_dd &b)
{
    double e;
    a.hi = vmp_two_sum(a.hi, b.hi, &e);
    a.lo = (a.lo + b.lo) + e;
}

// ln Gamma(x + dx) as hi + *lo: vmp_lgamma_dd from 10 upwards, where the value is large; below, the
// math library's (ocml on the device, libm on the host), whose error is relative to a small value
__host__ __device__ inline double vmp_lda_hyper_lgamma(double x, double dx, double *lo)
{
    if (x >= 10.0 && x < 4e15) return vmp_lgamma_dd(x, dx, lo);
    *lo = dx == 0.0 ? 0.0 : dx * vmp_digamma(x);
    return lgamma(x);
}

// what one element adds to qterm besides lgamma of its row sum: alpha elog - elog - lgamma(alpha)
__host__ __device__ inline void vmp_lda_hyper_q_add(vmp_dd &q, double alpha, double elog)
{
    const double p = alpha * elog, pe = fma(alpha, elog, -p);
    double lo;
    const double lg = vmp_lda_hyper_lgamma(alpha, 0.0, &lo);
    vmp_dd_add(q, p);
    vmp_dd_add(q, -elog);
    vmp_dd_add(q, -lg);
    q.lo += pe - lo;
}

#ifndef __HIPCC__
// the 64-lane butterfly of unevaluated sums; every element ends with the result
inline void vmp_lda_hyper_bfly_dd_host(vmp_dd *v)
{
    vmp_dd t[VMP_LDA_HYPER_LANES];
    for (int off = VMP_LDA_HYPER_LANES >> 1; off > 0; off >>= 1) {
        for (int l = 0; l < VMP_LDA_HYPER_LANES; ++l) {
            t[l] = v[l];
            vmp_dd_add_dd(t[l], v[l ^ off]);
        }
        for (int l = 0; l < VMP_LDA_HYPER_LANES; ++l) v[l] = t[l];
    }
}

// in lane over i ascending, then the plain butterfly: x[0 .. 64 R - 1] in position order, 0 beyond W
inline double vmp_lda_hyper_along_host(const double *x, int R)
{
    double v[VMP_LDA_HYPER_LANES];
    for (int j = 0; j < VMP_LDA_HYPER_LANES; ++j) {
        double s = x[j];
        for (int i = 1; i < R; ++i) s += x[j + VMP_LDA_HYPER_LANES * i];
        v[j] = s;
    }
    vmp_lda_group_sum_host(v, VMP_LDA_HYPER_LANES);
    return v[0];
}

// the single-workgroup sum of `cnt` unevaluated sums hi[i] + lo[i]
inline vmp_dd vmp_lda_hyper_strided_sum_host(const double *hi, const double *lo, int64_t cnt)
{
    vmp_dd total = {0.0, 0.0};
    for (int w = 0; w < VMP_LDA_HYPER_RED_NT / 64; ++w) {
        vmp_dd v[64];
        for (int l = 0; l < 64; ++l) {
            vmp_dd s = {0.0, 0.0};
            for (int64_t i = w * 64 + l; i < cnt; i += VMP_LDA_HYPER_RED_NT) {
                const vmp_dd x = {hi[i], lo[i]};
                vmp_dd_add_dd(s, x);
            }
            v[l] = s;
        }
        for (int off = 32; off > 0; off >>= 1)
            for (int l = 0; l < off; ++l) vmp_dd_add_dd(v[l], v[l + off]);
        if (w == 0) total = v[0]; else vmp_dd_add_dd(total, v[0]);
    }
    return total;
}
#endif
