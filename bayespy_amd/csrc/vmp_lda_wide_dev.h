// vmp_lda_wide_dev.h -- layout and order of operations of the wide-topic token pass of the
// latent-Dirichlet-allocation block (csrc/vmp_lda_wide.hip, 65 <= K <= 1024), shared with the host
// build of the CPU tests (tests/host/lda_wide_host.cpp).  The per-token arithmetic is that of
// vmp_lda_dev.h (vmp_lda_logit, vmp_lda_shifted_exp, vmp_lda_lse, vmp_lda_phi), unchanged.
//
// One wavefront of 64 lanes owns a CHUNK of consecutive tokens.  Lane j holds the topics
//     k = j + 64 r,   r = 0 .. R-1,
// R = the smallest of {2, 4, 8, 16} with 64 R >= K; a (lane, register) with k >= K holds a logit
// of -inf and contributes 0 to every sum.  A row of K contiguous doubles is then read as R
// wave-wide loads of 512 contiguous bytes each.
//
// Order of operations per token:
//   1. m_j = l[j], then m_j = fmax(m_j, l[j + 64 r]) for r = 1 .. R-1           (in lane, r ascending)
//   2. m   = the 64-lane butterfly of m_j, partner lane ^ 32, ^ 16, .. ^ 1      (vmp_lda_dev.h)
//   3. s_j = e[j], then s_j += e[j + 64 r] for r = 1 .. R-1,  e = exp(l - m), 0 for k >= K
//   4. s   = the 64-lane butterfly of s_j, the same partners
//   5. lse = m + log s;  phi_k = exp(l_k - lse), 0 for k >= K
// Every lane ends 2. and 4. with the same bits.  Counts add phi in token order per (lane, r).
//
// -inf: as in vmp_lda_dev.h -- a topic with l_k = -inf gets phi_k = 0 exactly; a token whose logits
// are ALL -inf has m = -inf, and its lse and the phi of its K topics are NaN.
#pragma once
#include "vmp_lda_dev.h"

#define VMP_LDA_WIDE_MIN_K 65
#define VMP_LDA_WIDE_MAX_K 1024
#define VMP_LDA_WIDE_LANES 64

// registers per lane: the smallest of {2, 4, 8, 16} with 64 R >= K (K <= 1024)
__host__ __device__ inline int vmp_lda_wide_regs(int K)
{
    int r = 2;
    while (r < 16 && VMP_LDA_WIDE_LANES * r < K) r <<= 1;
    return r;
}

// tokens one wavefront walks in order.  A function of n alone: vmp_lda_chunk_tokens with 64 lanes
// per chunk -- the smallest power of two from 16 to 256 that keeps n / chunk * 64 at or below 2^17
__host__ __device__ inline int vmp_lda_wide_chunk_tokens(int64_t n)
{
    return vmp_lda_chunk_tokens(n, VMP_LDA_WIDE_LANES);
}

#ifndef __HIPCC__
// steps 1-2 over l[0 .. 64 R - 1] (topic order, -inf beyond K)
inline double vmp_lda_wide_max_host(const double *l, int R)
{
    double v[VMP_LDA_WIDE_LANES];
    for (int j = 0; j < VMP_LDA_WIDE_LANES; ++j) {
        double m = l[j];
        for (int r = 1; r < R; ++r) m = fmax(m, l[j + VMP_LDA_WIDE_LANES * r]);
        v[j] = m;
    }
    vmp_lda_group_max_host(v, VMP_LDA_WIDE_LANES);
    return v[0];
}

// steps 3-4 over e[0 .. 64 R - 1] (topic order, 0 beyond K)
inline double vmp_lda_wide_sum_host(const double *e, int R)
{
    double v[VMP_LDA_WIDE_LANES];
    for (int j = 0; j < VMP_LDA_WIDE_LANES; ++j) {
        double s = e[j];
        for (int r = 1; r < R; ++r) s += e[j + VMP_LDA_WIDE_LANES * r];
        v[j] = s;
    }
    vmp_lda_group_sum_host(v, VMP_LDA_WIDE_LANES);
    return v[0];
}
#endif
