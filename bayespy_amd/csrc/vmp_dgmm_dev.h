// vmp_dgmm_dev.h -- arithmetic of the diagonal-Gaussian-mixture block (csrc/vmp_dgmm.hip), shared
// with the host build of the CPU tests (tests/host/dgmm_host.cpp).  vmp_digamma and vmp_lgamma
// (vmp_common.h) are declared before this header is included.
//
//     alpha = Dirichlet(a);  Z = Categorical(alpha, plates=(N, 1))
//     mu = GaussianARD(m0, beta0, plates=(D, K));  tau = Gamma(a0, b0, plates=(D, K))
//     Y = Mixture(Z, GaussianARD, mu, tau);  Y.observe(y)                     y (N, D)
//
// A row n of real observations y_n (D doubles) has the logits
//     l_k = c[k] + sum_d y_nd h[d, k] + y_nd^2 q[d, k],        k = 0 .. K-1,
// with h = <tau><mu>, q = -1/2 <tau>, g = 1/2 <log tau> - 1/2 <tau><mu^2> (all D x K) and
// c[k] = <log pi_k> + sum_d g[d, k] (mixture.py: the (N, D, K) broadcast of the GaussianARD
// log-density summed over D plus the message of the Categorical parent).  The constant
// -1/2 log 2 pi per element is the same for every k and stays out of the tables.  The
// responsibilities are r_k = exp(l_k - lse), lse = m + log(sum_k exp(l_k - m)), m = max_k l_k.
//
// A CONSTANT IS TAKEN OUT OF c: vmp_dgmm_tables subtracts max_k c[k], for the reason vmp_bmm_dev.h
// gives (a Dirichlet prior of 1e-5 has <log pi> near -1e5, and sum_d g grows with D).  lse and
// sum lse are relative to the constant taken out.
//
// ORDER OF THE ADDITIONS (what the host build restates):
//   * c[k]: sum_d g[d, k] from zero in ascending d, then + <log pi_k>, then - the maximum;
//   * logit: starts at zero; the columns are walked in steps of 4: the four y h of a step in
//     ascending d, then its four y^2 q in ascending d (one matrix instruction each); c[k] last;
//   * K is padded to KP = a multiple of 16 with -inf logits; lane j of a 16-lane group holds columns
//     j, j + 16, ...: the sum under the logarithm adds a lane's columns in ascending order, then
//     runs the butterfly (partner j ^ off, off = 8, 4, 2, 1);
//   * rows are walked in TILES of 64; row t of a tile belongs to SLOT (t / 16) * 4 + (t % 16) % 4.
//     N_k and sum lse are kept per slot in row order; the 16 slots are added in slot order at the
//     end of a CHUNK;
//   * S1[k, d] = sum r_k y_d and S2[k, d] = sum r_k y_d^2 in two levels: within a tile of 64 rows
//     from zero in ascending row order, and the tiles' sums in tile order to the running sum of the
//     chunk (vmp_bmm_dev.h: sums of many nearly equal terms drift less that way);
//   * a workgroup owns one chunk of vmp_dgmm_chunk_rows(N, D, K) consecutive rows; the chunks'
//     partial S1, S2, N_k and sum lse are added in chunk order by a second kernel;
//   * the bound term of an update: element e = d K + k belongs to thread e % 256, which adds its
//     elements in ascending order; the 256 sums are halved eight times, v[i] += v[i + off] for
//     off = 128, 64, ..., 1.  (Added in thread order, 256 sums of one sign and one size put the
//     bound term of mu at 1.5 times its allowance at (N, D, K) = (300, 257, 5).)
// The bits of every output therefore depend on the inputs and (N, D, K) only.
//
// Non-finite y or tables are OUTSIDE the contract.  A logit of -inf (padding) gives r = 0 exactly.
#pragma once

#include <stdint.h>

#define VMP_DGMM_MAX_K 64
#define VMP_DGMM_MAX_D 1024
#define VMP_DGMM_TILE 64           // rows per tile: 16 per wavefront of a four-wavefront workgroup
#define VMP_DGMM_MIN_CHUNK 256
#define VMP_DGMM_MAX_CHUNKS 1024
#define VMP_DGMM_DBLOCK 64         // columns of y, S1 and S2 a workgroup holds at a time
#define VMP_DGMM_NT 256            // threads of every kernel of the block

__host__ __device__ inline int vmp_dgmm_kpad(int K) { return (K + 15) & ~15; }

// doubles one chunk leaves behind: S1 (K x D), S2 (K x D), N_k (K), sum lse (1)
__host__ __device__ inline int64_t vmp_dgmm_partial_doubles(int D, int K)
{
    return 2 * (int64_t)D * K + K + 1;
}

// rows of a chunk: a function of (N, D, K) alone.  At most VMP_DGMM_MAX_CHUNKS chunks and at most
// 2^25 doubles (256 MB) of partials; a multiple of the tile, at least VMP_DGMM_MIN_CHUNK.
__host__ __device__ inline int64_t vmp_dgmm_chunk_rows(int64_t N, int D, int K)
{
    int64_t maxc = ((int64_t)1 << 25) / vmp_dgmm_partial_doubles(D, K);
    if (maxc > VMP_DGMM_MAX_CHUNKS) maxc = VMP_DGMM_MAX_CHUNKS;
    if (maxc < 1) maxc = 1;
    int64_t rows = (N + maxc - 1) / maxc;
    rows = (rows + VMP_DGMM_TILE - 1) / VMP_DGMM_TILE * VMP_DGMM_TILE;
    if (rows < VMP_DGMM_MIN_CHUNK) rows = VMP_DGMM_MIN_CHUNK;
    return rows;
}

__host__ __device__ inline int64_t vmp_dgmm_chunks(int64_t N, int D, int K)
{
    const int64_t rows = vmp_dgmm_chunk_rows(N, D, K);
    return N > 0 ? (N + rows - 1) / rows : 0;
}

// slot of row t (0 .. 63) of a tile
__host__ __device__ inline int vmp_dgmm_slot(int t) { return (t >> 4) * 4 + (t & 3); }

// -- the tables -------------------------------------------------------------------------------------
__host__ __device__ inline double vmp_dgmm_h(double tau, double mu) { return tau * mu; }

__host__ __device__ inline double vmp_dgmm_q(double tau) { return -0.5 * tau; }

__host__ __device__ inline double vmp_dgmm_g(double tau, double log_tau, double mu2)
{
    return 0.5 * log_tau - 0.5 * tau * mu2;
}

// -- the pass -----------------------------------------------------------------------------------------
__host__ __device__ inline double vmp_dgmm_square(double y) { return y * y; }

// one step of a product
__host__ __device__ inline double vmp_dgmm_mac(double acc, double a, double b) { return acc + a * b; }

// the column's constant, added last
__host__ __device__ inline double vmp_dgmm_logit_finish(double sum, double c_k) { return sum + c_k; }

// exp(l - m) of the sum under the logarithm; m is the row's maximum, so the argument is <= 0
__host__ __device__ inline double vmp_dgmm_shifted_exp(double logit, double m)
{
    return exp(logit - m);
}

__host__ __device__ inline double vmp_dgmm_lse(double m, double s) { return m + log(s); }

__host__ __device__ inline double vmp_dgmm_resp(double logit, double lse) { return exp(logit - lse); }

// -- the updates (expfamily.py:400-480 for the bound terms) -----------------------------------------------
// q(mu_dk) = N(m, 1 / lambda): par = (m, lambda), mom = (<mu>, <mu^2>).  Returns the node's bound
// term <log p(mu)> - <log q(mu)> = 1/2 log(beta0 / lambda) - 1/2 beta0 ((m - m0)^2 + 1 / lambda)
// + 1/2: the sum of the reference's five terms with what cancels between them taken out, and with
// lambda - beta0 = <tau> N_k kept as it is, so that the term is exactly zero where q is the prior.
__host__ __device__ inline double vmp_dgmm_update_mu(double m0, double beta0, double tau, double nk,
                                                     double s1, double *par, double *mom)
{
    const double add = tau * nk;                     // lambda - beta0
    const double lambda = beta0 + add;
    const double dm = tau * (s1 - nk * m0) / lambda; // m - m0: (beta0 m0 + <tau> S1) / lambda - m0
    const double m = m0 + dm;
    par[0] = m;
    par[1] = lambda;
    mom[0] = m;
    mom[1] = m * m + 1.0 / lambda;
    return -0.5 * log1p(add / beta0) - 0.5 * beta0 * (dm * dm) + 0.5 * (add / lambda);
}

// q(tau_dk) = Gamma(a, b): par = (a, b), mom = (<tau>, <log tau>).  Returns <log p(tau)> -
// <log q(tau)> = a0 (log b0 - log b) - lgamma(a0) + lgamma(a) + (a0 - a) psi(a) + a - b0 a / b,
// with b - b0 kept as it is (a - b0 a / b = (b - b0) a / b): exactly zero where q is the prior.
__host__ __device__ inline double vmp_dgmm_update_tau(double a0, double b0, double mu1, double mu2,
                                                      double nk, double s1, double s2, double *par,
                                                      double *mom)
{
    const double a = a0 + 0.5 * nk;
    const double add = 0.5 * (s2 - 2.0 * mu1 * s1 + mu2 * nk);       // b - b0
    const double b = b0 + add;
    const double psi = vmp_digamma(a), tau = a / b;
    par[0] = a;
    par[1] = b;
    mom[0] = tau;
    mom[1] = psi - log(b);
    return -a0 * log1p(add / b0) - vmp_lgamma(a0) + vmp_lgamma(a) + (a0 - a) * psi + add * tau;
}

// -- deterministic annealing (expfamily.py:343-350, :400-480) ------------------------------------------
// A node with the coefficient ab in (0, 1] updates to ab times its natural parameters; its bound term
// is A - T B with T = 1 / ab AT THE REQUEST, A = cgf from the parents + phi_p . u and B = phi_q . u +
// g_q (the base measure cancels as at T = 1).  ab = 1 gives the bits of the plain forms: par and mom
// are formed by the same expressions from ab * (the plain parameters).
__host__ __device__ inline double vmp_dgmm_anneal(double ab, double x) { return ab * x; }

// A and B of q(mu_dk) = N(m, 1 / lambda) under the prior N(m0, 1 / beta0):
//   A = 1/2 log beta0 - 1/2 beta0 ((m - m0)^2 + 1 / lambda),   B = 1/2 log lambda - 1/2
__host__ __device__ inline void vmp_dgmm_parts_mu(double m0, double beta0, const double *par,
                                                  double *A, double *B)
{
    const double dm = par[0] - m0, lambda = par[1];
    *A = 0.5 * log(beta0) - 0.5 * beta0 * (dm * dm + 1.0 / lambda);
    *B = 0.5 * log(lambda) - 0.5;
}

// A and B of q(tau_dk) = Gamma(a, b) under the prior Gamma(a0, b0), mom = (<tau>, <log tau>):
//   A = a0 log b0 - lgamma(a0) - b0 <tau> + a0 <log tau>,   B = a psi(a) - a - lgamma(a)
__host__ __device__ inline void vmp_dgmm_parts_tau(double a0, double b0, const double *par,
                                                   const double *mom, double *A, double *B)
{
    // psi(a) itself, not <log tau> + log b, which carries the rounding of both of its terms times a
    const double a = par[0], psi = vmp_digamma(a);
    *A = a0 * log(b0) - vmp_lgamma(a0) - b0 * mom[0] + a0 * mom[1];
    *B = a * (psi - 1.0) - vmp_lgamma(a);
}

// mu with the coefficient ab: precision ab (beta0 + N_k <tau>), the mean as at ab = 1
__host__ __device__ inline void vmp_dgmm_update_mu_annealed(double ab, double m0, double beta0,
                                                            double tau, double nk, double s1,
                                                            double *par, double *mom, double *A,
                                                            double *B)
{
    vmp_dgmm_update_mu(m0, beta0, tau, nk, s1, par, mom);
    const double m = par[0], lambda = vmp_dgmm_anneal(ab, par[1]);
    par[1] = lambda;
    mom[1] = m * m + 1.0 / lambda;
    vmp_dgmm_parts_mu(m0, beta0, par, A, B);
}

// tau with the coefficient ab: a = ab (a0 + N_k / 2), b = ab (b0 + ...)
__host__ __device__ inline void vmp_dgmm_update_tau_annealed(double ab, double a0, double b0,
                                                             double mu1, double mu2, double nk,
                                                             double s1, double s2, double *par,
                                                             double *mom, double *A, double *B)
{
    vmp_dgmm_update_tau(a0, b0, mu1, mu2, nk, s1, s2, par, mom);
    const double a = vmp_dgmm_anneal(ab, par[0]), b = vmp_dgmm_anneal(ab, par[1]);
    const double psi = vmp_digamma(a), tau = a / b;
    par[0] = a;
    par[1] = b;
    mom[0] = tau;
    mom[1] = psi - log(b);
    vmp_dgmm_parts_tau(a0, b0, par, mom, A, B);
}

#ifndef __HIPCC__
// the butterfly of a 16-lane group over v[0 .. 15]; every element ends with the result
inline void vmp_dgmm_group_sum_host(double *v)
{
    double t[16];
    for (int off = 8; off > 0; off >>= 1) {
        for (int l = 0; l < 16; ++l) t[l] = v[l] + v[l ^ off];
        for (int l = 0; l < 16; ++l) v[l] = t[l];
    }
}
#endif
