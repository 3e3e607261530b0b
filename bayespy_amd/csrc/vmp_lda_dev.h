// vmp_lda_dev.h -- per-token arithmetic of the latent-Dirichlet-allocation token pass
// (csrc/vmp_lda.hip), shared with the host build of the CPU tests (tests/host/lda_host.cpp).
//
// A token n with document d and vocabulary index w has the logits
//     l_k = <log theta>[d, k] + <log beta>[k, w],            k = 0 .. K-1,
// its responsibilities are phi_k = exp(l_k - lse) with lse = m + log(sum_k exp(l_k - m)),
// m = max_k l_k (categorical.py:117-124 / multinomial.py:118-140: normalised exponential).
//
// The K logits of a token sit in a GROUP of G lanes, G = the power of two >= K; lanes k >= K
// hold -inf.  Maximum and sum over the group are butterflies (partner lane ^ off, off = G/2 ..
// 1): every lane ends with the same bits, and the order of the additions depends on G alone.
// The host build runs the same butterfly over an array of G values.
//
// Logits of -inf: a topic with l_k = -inf gets phi_k = 0 exactly.  A token whose logits are ALL
// -inf has m = -inf; l_k - m is then NaN, and lse and every phi_k of that token are NaN, as in
// the reference (exp(-inf - (-inf))).  Nothing else turns into NaN.
#pragma once

// lane group of K topics: the power of two >= K (1 for K = 1)
__host__ __device__ inline int vmp_lda_group(int K)
{
    int g = 1;
    while (g < K) g <<= 1;
    return g;
}

// tokens one lane group walks in order (a CHUNK).  A function of (n, K) alone: the smallest power
// of two from 16 to 256 that keeps the number of busy lanes n / chunk * G at or below 2^17 (about
// eight wavefronts on each of the 256 compute units).
__host__ __device__ inline int vmp_lda_chunk_tokens(int64_t n, int K)
{
    const int64_t lanes = n * (int64_t)vmp_lda_group(K);
    int t = 16;
    while (t < 256 && lanes / t > ((int64_t)1 << 17)) t <<= 1;
    return t;
}

__host__ __device__ inline double vmp_lda_logit(double elog_theta_dk, double elog_beta_kw)
{
    return elog_theta_dk + elog_beta_kw;
}

// exp(l - m) of the sum under the logarithm; m is the group's maximum, so the argument is <= 0
__host__ __device__ inline double vmp_lda_shifted_exp(double logit, double m)
{
    return exp(logit - m);
}

__host__ __device__ inline double vmp_lda_lse(double m, double s) { return m + log(s); }

__host__ __device__ inline double vmp_lda_phi(double logit, double lse) { return exp(logit - lse); }

#ifndef __HIPCC__
// the butterflies of a lane group over an array v[0 .. G-1]; every element ends with the result
inline void vmp_lda_group_max_host(double *v, int G)
{
    double t[64];
    for (int off = G >> 1; off > 0; off >>= 1) {
        for (int l = 0; l < G; ++l) t[l] = fmax(v[l], v[l ^ off]);
        for (int l = 0; l < G; ++l) v[l] = t[l];
    }
}

inline void vmp_lda_group_sum_host(double *v, int G)
{
    double t[64];
    for (int off = G >> 1; off > 0; off >>= 1) {
        for (int l = 0; l < G; ++l) t[l] = v[l] + v[l ^ off];
        for (int l = 0; l < G; ++l) v[l] = t[l];
    }
}
#endif
