// vmp_hmm_fused_dev.h -- per-step arithmetic of the chain pass of the fused hidden-Markov-model
// block (csrc/vmp_hmm_fused.hip), shared with the host build of the CPU tests
// (tests/host/hmm_fused_host.cpp).
//
// A chain b has T time instances with observations y_t (D doubles) and K states.  With the
// emission log-likelihoods e_t[j] = sum_f C[j][f] phi_f(y_t) (features phi in the compact order of
// vmp_gmm_prepare_z: y_a y_b for a <= b, then y_d, then 1) the reference builds
//     logp0[j] = <log a0_j> + e_0[j],    logP[n, i, j] = <log A_ij> + e_{n+1}[j],   n = 0 .. T-2,
// and runs random.alpha_beta_recursion on it.  Here nothing of size K x K exists per step:
//
//   forward   la_0 = logp0 (not normalised, as in the reference); for n = 0 .. T-2
//                 m_j = max_i (la_n[i] + A_ij),  s_j = sum_i exp(la_n[i] + A_ij - m_j)
//                 q_j = m_j + log s_j + e_{n+1}[j]        (log of column j's sum)
//                 c_n = lse_j q_j,  la_{n+1} = q - c_n,   log Z_b = sum_n c_n
//             la_n (K doubles) goes to the workspace: the only thing kept per step.
//   backward  lb_{T-1} = 0; for n = T-2 .. 0, with u_j = e_{n+1}[j] + lb_{n+1}[j]
//                 gamma_{n+1} = softmax_j (la_{n+1}[j] + lb_{n+1}[j])
//                 xi_n[i, j]  = gamma_{n+1}[j] exp(la_n[i] + A_ij - m_j) / s_j   (m, s as above)
//                 lb_n[i]     = lse_j (A_ij + u_j), less its largest element
//             and gamma_0 = softmax_i (la_0[i] + lb_0[i]) (= the normalised row sums of xi_0).
//
// Everything is a logarithm until the last exponential, whose argument is <= 0: tables such as
// <log A_ij> = -985 everywhere (Dirichlet(1e-3) rows at K = 64) or one row near 0 and the others
// near -670 never pass through exp(<log A>).  exp(-inf - m) counts as 0, so a state with -inf in
// <log a0> or in a column of <log A> gets 0; a step whose logits are ALL -inf gives
// c = -inf and la = -inf - (-inf) = NaN, as in the reference.
//
// ORDER OF THE ADDITIONS (what the host build restates):
//   * K is padded to KP = 2, 4, ..., 64 lanes per chain, lane j owns column j (forward, xi,
//     gamma, the statistics of state j) and row j (lb);  64 / KP chains share a wavefront;
//   * sums over i (or over j for lb) run in ascending order inside the lane; maxima and sums over
//     the lanes of a chain are butterflies with partner j ^ 1, j ^ 2, ..., j ^ (KP / 2);
//   * e = sum over the features in compact order, starting from zero;
//   * a workgroup (one wavefront) owns vmp_hmmf_chains_per_wg(B, D, K) consecutive chains;
//     chain c of its range belongs to lane group c % (64 / KP), which walks its chains in
//     ascending order and adds each chain's steps in the order of the backward sweep
//     (t = T-1 ... 1, then t = 0);  the groups are added in group order, then the workgroups'
//     partials in workgroup order by a second kernel;
//   * categorical emissions (csrc/vmp_hmm_cat.hip; y_t a word in [0, M), e_t[j] = <log P>[y_t][j]
//     read from the word-major table, nothing to add up): everything above but the feature line,
//     with vmp_hmmf_cat_chains_per_wg(B, M, K) chains per workgroup; the count S[m][j] of lane
//     (group g, column j) takes gamma_t[j] times the chain weight at the observed steps with
//     y_t = m, in the order in which that lane meets them (its chains ascending, each in the
//     order of the backward sweep); a workgroup's partial adds the groups from zero in group
//     order, the second kernel the workgroups in workgroup order and writes S word-major (M, K).
// The bits of every output therefore depend on the inputs and (B, T, D, K) only ((B, T, M, K) with
// categorical emissions).
//
// MASKS (vmp_hmm_fused_pass_masked; mask[b, t] = 1 where y_{b,t} is observed).  A masked step
// sends a zero message: e_t = 0 for every state.  The step stays in the chain: the recursion above
// runs over all T steps with that e, trailing masked steps propagate through <log A> and their xi
// counts.  y_t of a masked step is never read (the pass selects, it does not multiply by zero), so
// NaN may stand there.  Chain b has the weight o_b = "any step of b observed"; the sums are
//     sum gamma_0 = sum_b o_b gamma_{b,0},   sum xi = sum_b o_b sum_n xi_{b,n},
//     sum log Z = sum_b o_b log Z_b,   T_k and sum gamma . e over the observed (b, t) only.
// The order of the additions is the one above with the masked steps absent from the feature sums
// and from sum gamma . e, and with the terms of a chain that has o_b = 0 multiplied by 0 (as those
// of the chains past the end of a workgroup's range are).  A mask of ones gives the bits of the
// unmasked pass.  gamma, z0 and zz of a chain with o_b = 0 are what the recursion gives with
// e = 0 throughout (the reference leaves the moments of such a chain at their initial values).
#pragma once

#include <math.h>
#include <stdint.h>

#define VMP_HMMF_MAX_K 64
#define VMP_HMMF_MAX_D 8
#define VMP_HMMF_MAX_WGS 4096
#define VMP_HMMF_MAX_NF 45        // features of D = 8
#define VMP_HMMF_MAX_M 128        // categorical emissions: 512 M bytes of count accumulators in LDS

__host__ __device__ inline int vmp_hmmf_kpad(int K)
{
    int p = 2;
    while (p < K) p <<= 1;
    return p;
}

// compact features: y_a y_b (a <= b), y_d, 1
__host__ __device__ inline int vmp_hmmf_nfeat(int D) { return D * (D + 1) / 2 + D + 1; }

// doubles one workgroup leaves behind: sum gamma_0 (K), sum xi (K x K), the feature sums
// (K x NF, compact), sum log Z, sum gamma . e
__host__ __device__ inline int64_t vmp_hmmf_partial_doubles(int D, int K)
{
    return (int64_t)K + (int64_t)K * K + (int64_t)K * vmp_hmmf_nfeat(D) + 2;
}

// chains of a workgroup: a function of the shape alone; a multiple of the 64 / KP chains that
// share the wavefront, at most VMP_HMMF_MAX_WGS workgroups and 2^24 doubles of partials
__host__ __device__ inline int64_t vmp_hmmf_chains_per_wg(int64_t B, int D, int K)
{
    const int64_t groups = 64 / vmp_hmmf_kpad(K);
    int64_t maxw = ((int64_t)1 << 24) / vmp_hmmf_partial_doubles(D, K);
    if (maxw > VMP_HMMF_MAX_WGS) maxw = VMP_HMMF_MAX_WGS;
    if (maxw < 1) maxw = 1;
    int64_t c = (B + maxw - 1) / maxw;
    c = (c + groups - 1) / groups * groups;
    if (c < groups) c = groups;
    return c;
}

__host__ __device__ inline int64_t vmp_hmmf_wgs(int64_t B, int D, int K)
{
    const int64_t c = vmp_hmmf_chains_per_wg(B, D, K);
    return B > 0 ? (B + c - 1) / c : 0;
}

// workspace of the pass: la (B T K), the partials, 1024 doubles for the dot products
__host__ __device__ inline int64_t vmp_hmmf_workspace_doubles(int64_t B, int T, int D, int K)
{
    return B * (int64_t)T * K + vmp_hmmf_wgs(B, D, K) * vmp_hmmf_partial_doubles(D, K) + 1024;
}

// the two factors of feature f as indices into (y_0 .. y_{D-1}, 1)
__host__ __device__ inline void vmp_hmmf_feature(int D, int f, int *pa, int *pb)
{
    const int npair = D * (D + 1) / 2;
    if (f < npair) {
        int rem = f, a = 0;
        while (rem >= D - a) { rem -= D - a; ++a; }
        *pa = a;
        *pb = a + rem;
    } else {
        *pa = f - npair;          // y_d, and D for the constant
        *pb = D;
    }
}

// exp(x - m) with the conventions of a masked softmax: -inf gives 0 whatever m is
__host__ __device__ inline double vmp_hmmf_exp_shift(double x, double m)
{
    return (x == -INFINITY) ? 0.0 : exp(x - m);
}

// e = sum_f C[f * ldc] phi[f], from zero in ascending f
__host__ __device__ inline double vmp_hmmf_emit(const double *C, int ldc, const double *phi, int NF)
{
    double e = 0.0;
    for (int f = 0; f < NF; ++f) e += C[f * ldc] * phi[f];
    return e;
}

// the emission term of a step: 0 where it is masked, whatever e holds (NaN included)
__host__ __device__ inline double vmp_hmmf_observed_or_zero(bool observed, double e)
{
    return observed ? e : 0.0;
}

// categorical emissions: a step counts as observed when its mask says so AND its word lies in
// [0, M) (one unsigned compare); any other word indexes nothing and the step sends a zero message.
// The caller validates the words; this only keeps a bad one from becoming an address.
__host__ __device__ inline bool vmp_hmmf_cat_observed(bool unmasked, int32_t word, int M)
{
    return unmasked && (uint32_t)word < (uint32_t)M;
}

// doubles one workgroup leaves behind: sum gamma_0 (K), sum xi (K x K), the counts (M x K,
// word-major), sum log Z, sum gamma . e
__host__ __device__ inline int64_t vmp_hmmf_cat_partial_doubles(int M, int K)
{
    return (int64_t)K + (int64_t)K * K + (int64_t)M * K + 2;
}

// as vmp_hmmf_chains_per_wg, with the partial of the categorical pass
__host__ __device__ inline int64_t vmp_hmmf_cat_chains_per_wg(int64_t B, int M, int K)
{
    const int64_t groups = 64 / vmp_hmmf_kpad(K);
    int64_t maxw = ((int64_t)1 << 24) / vmp_hmmf_cat_partial_doubles(M, K);
    if (maxw > VMP_HMMF_MAX_WGS) maxw = VMP_HMMF_MAX_WGS;
    if (maxw < 1) maxw = 1;
    int64_t c = (B + maxw - 1) / maxw;
    c = (c + groups - 1) / groups * groups;
    if (c < groups) c = groups;
    return c;
}

__host__ __device__ inline int64_t vmp_hmmf_cat_wgs(int64_t B, int M, int K)
{
    const int64_t c = vmp_hmmf_cat_chains_per_wg(B, M, K);
    return B > 0 ? (B + c - 1) / c : 0;
}

// workspace of the categorical pass: la (B T K), the partials, 1024 doubles for the dot products
__host__ __device__ inline int64_t vmp_hmmf_cat_workspace_doubles(int64_t B, int T, int M, int K)
{
    return B * (int64_t)T * K + vmp_hmmf_cat_wgs(B, M, K) * vmp_hmmf_cat_partial_doubles(M, K)
           + 1024;
}

// the weight of a chain: 1 if any of its T steps is observed
__host__ __device__ inline int vmp_hmmf_chain_observed(const uint8_t *row, int T)
{
    int any = 0;
    for (int t = 0; t < T; ++t) any |= row[t];
    return any != 0;
}

// column (or row) j of the recursion: m = max_i (v[i] + a[i * lda]), s = sum_i exp(. - m)
__host__ __device__ inline void vmp_hmmf_column(const double *v, const double *a, int lda, int K,
                                                double *m, double *s)
{
    double mm = -INFINITY;
    for (int i = 0; i < K; ++i) mm = fmax(mm, v[i] + a[i * lda]);
    double ss = 0.0;
    for (int i = 0; i < K; ++i) ss += vmp_hmmf_exp_shift(v[i] + a[i * lda], mm);
    *m = mm;
    *s = ss;
}

// xi = gamma p / s; a state that cannot be reached (gamma == 0) contributes exact zeros
__host__ __device__ inline double vmp_hmmf_ratio(double gamma, double s)
{
    return gamma == 0.0 ? 0.0 : gamma / s;
}

#ifndef __HIPCC__
// butterflies over the KP lanes of a chain; every element ends with the result
inline void vmp_hmmf_group_max_host(double *v, int KP)
{
    double t[VMP_HMMF_MAX_K];
    for (int off = 1; off < KP; off <<= 1) {
        for (int l = 0; l < KP; ++l) t[l] = fmax(v[l], v[l ^ off]);
        for (int l = 0; l < KP; ++l) v[l] = t[l];
    }
}

inline void vmp_hmmf_group_sum_host(double *v, int KP)
{
    double t[VMP_HMMF_MAX_K];
    for (int off = 1; off < KP; off <<= 1) {
        for (int l = 0; l < KP; ++l) t[l] = v[l] + v[l ^ off];
        for (int l = 0; l < KP; ++l) v[l] = t[l];
    }
}
#endif
