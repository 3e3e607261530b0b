// vmp_dgmm_masked_dev.h -- arithmetic of the diagonal-Gaussian-mixture block with missing
// observations (csrc/vmp_dgmm_masked.hip), shared with the host build of the CPU tests
// (tests/host/dgmm_masked_host.cpp).  It adds to vmp_dgmm_dev.h, whose functions it uses unchanged.
//
//     Y = Mixture(Z, GaussianARD, mu, tau);  Y.observe(y, mask=m)            y, m (N, D)
//
// With m_nd in {0, 1} and yt = m o y a row has the logits
//     l_k = c[k] + sum_d m_nd g[d, k] + yt_nd h[d, k] + yt_nd^2 q[d, k],
// h = <tau><mu>, q = -1/2 <tau>, g = 1/2 <log tau> - 1/2 <tau><mu^2> (all D x K) and
// c = <log pi> less its largest element: sum_d g is no constant of the cluster any more, it leaves c
// and becomes a third product.  The statistics are M[d, k] = sum_n r_nk m_nd, S1 = sum r yt,
// S2 = sum r yt^2; N_k and sum lse run over the rows with an observed entry only.
//
// THE MASK TRAVELS INSIDE y: vmp_dgmm_pack_masked writes the pass's own copy of y with the one bit
// pattern VMP_DGMM_HIDDEN_BITS (a quiet NaN) at the hidden positions, chosen by a select, and the
// pass finds the mask again as y == y.  m, yt and yt^2 are formed by selects from the staged value,
// so whatever the caller's y holds at a hidden position (NaN, inf, 1e300) reaches no sum, and the
// masked pass reads the 8 N D bytes of the unmasked one and nothing else.  The padding of a tile
// (rows beyond the chunk, columns beyond D) is the same pattern.  A NaN of the caller's at an
// OBSERVED position is outside the contract, as every non-finite y is.
//
// ORDER OF THE ADDITIONS (what the host build restates); where nothing is said, vmp_dgmm_dev.h:
//   * logit: starts at zero; the columns are walked in steps of 4: the four m g of a step in
//     ascending d, then its four yt h, then its four yt^2 q (one matrix instruction each); c[k]
//     last.  A hidden entry adds 0 g, 0 h and 0 q: the sum does not move;
//   * softmax, slots, tiles of 64 rows and chunks as in vmp_dgmm_dev.h.  A row with nothing
//     observed has r = softmax(c); it adds nothing to its slot's N_k and sum lse, and zeros to M,
//     S1 and S2.  With fixed labels such a row is one-hot and stays out of N_k as well;
//   * M, S1 and S2 in two levels: within a tile of 64 rows from zero in ascending row order, the
//     tiles' sums in tile order to the running sum of the chunk.  The columns are held in COLUMN
//     BLOCKS of VMP_DGMM_MASKED_DBLOCK = 32 (three statistics at 64 columns do not fit the register
//     file); an element's sum does not depend on the block width;
//   * chunks of vmp_dgmm_masked_chunk_rows(N, D, K) rows, the partials (S1, S2, M as K x D, N_k,
//     sum lse) added in chunk order;
//   * scal[2] = (S1 . h + S2 . q) + M . g from three dot products;
//   * the updates: vmp_dgmm_update_mu and vmp_dgmm_masked_update_tau (below) with M[d, k] in the
//     place of N_k, the bound sums halved eight times as in vmp_dgmm_dev.h.
// The bits of every output therefore depend on the inputs and (N, D, K) only.
#pragma once

#include "vmp_dgmm_dev.h"

#define VMP_DGMM_MASKED_MAX_K 64
#define VMP_DGMM_MASKED_MAX_D 1024
#define VMP_DGMM_MASKED_DBLOCK 32  // columns of y, S1, S2 and M a workgroup holds at a time
#define VMP_DGMM_HIDDEN_BITS 0x7ff8000000000000ULL

// doubles one chunk leaves behind: S1, S2, M (K x D each), N_k (K), sum lse (1)
__host__ __device__ inline int64_t vmp_dgmm_masked_partial_doubles(int D, int K)
{
    return 3 * (int64_t)D * K + K + 1;
}

// rows of a chunk: the rule of vmp_dgmm_chunk_rows on the larger partial
__host__ __device__ inline int64_t vmp_dgmm_masked_chunk_rows(int64_t N, int D, int K)
{
    int64_t maxc = ((int64_t)1 << 25) / vmp_dgmm_masked_partial_doubles(D, K);
    if (maxc > VMP_DGMM_MAX_CHUNKS) maxc = VMP_DGMM_MAX_CHUNKS;
    if (maxc < 1) maxc = 1;
    int64_t rows = (N + maxc - 1) / maxc;
    rows = (rows + VMP_DGMM_TILE - 1) / VMP_DGMM_TILE * VMP_DGMM_TILE;
    if (rows < VMP_DGMM_MIN_CHUNK) rows = VMP_DGMM_MIN_CHUNK;
    return rows;
}

__host__ __device__ inline int64_t vmp_dgmm_masked_chunks(int64_t N, int D, int K)
{
    const int64_t rows = vmp_dgmm_masked_chunk_rows(N, D, K);
    return N > 0 ? (N + rows - 1) / rows : 0;
}

// the value of a hidden position: one bit pattern, whatever the caller's y holds there
__host__ __device__ inline double vmp_dgmm_hidden()
{
    union { unsigned long long u; double d; } v;
    v.u = VMP_DGMM_HIDDEN_BITS;
    return v.d;
}

// what the pack writes: a select, never a product
__host__ __device__ inline double vmp_dgmm_pack_value(double y, int observed)
{
    return observed ? y : vmp_dgmm_hidden();
}

// the mask, found again in the packed value
__host__ __device__ inline bool vmp_dgmm_observed(double packed) { return packed == packed; }

// the three A operands of a logit step (and B operands of the statistics) from the packed value
__host__ __device__ inline double vmp_dgmm_mask_value(double packed)
{
    return vmp_dgmm_observed(packed) ? 1.0 : 0.0;
}

__host__ __device__ inline double vmp_dgmm_masked_value(double packed)
{
    return vmp_dgmm_observed(packed) ? packed : 0.0;
}

// lgamma(a0 + delta) - lgamma(a0), delta >= 0, without the difference of two logarithms of the gamma
// function: both are shifted by 16 (Stirling's series to y^-9 is exact to 1e-16 from y = 16 on),
//     lgamma(x) = St(x + 16) - sum_{i < 16} log(x + i),  St(y) = (y - 1/2) log y - y + s(y) + const,
// and the differences are taken term by term: St(y1) - St(y0) = (y0 - 1/2) log1p(delta / y0) +
// delta log y1 - delta + s(y1) - s(y0) and log((x + delta + i) / (x + i)) = log1p(delta / (x + i)).
// With missing observations the count of an element can be 1e-6: vmp_lgamma(a) - vmp_lgamma(a0) is
// then the difference of two numbers of size one, each good to 1e-14, where the bound term is of
// size 1e-12.  Exactly zero at delta = 0.
__host__ __device__ inline double vmp_dgmm_stirling_tail(double y)
{
    const double z = 1.0 / (y * y);
    return (1.0 / 12.0 + z * (-1.0 / 360.0 + z * (1.0 / 1260.0 + z * (-1.0 / 1680.0
                                                                    + z * (1.0 / 1188.0))))) / y;
}

__host__ __device__ inline double vmp_dgmm_lgamma_diff(double a0, double delta)
{
    const double y0 = a0 + 16.0, y1 = y0 + delta;
    // the sixteen logarithms, all positive and in descending order, with the rounding errors of
    // their additions kept in `lost` (at a count of a hundred they add up to 40 and more)
    double logs = 0.0, lost = 0.0;
    for (int i = 0; i < 16; ++i) {
        const double v = log1p(delta / (a0 + i)), t = logs + v;
        lost += (logs >= v) ? (logs - t) + v : (v - t) + logs;
        logs = t;
    }
    const double st = (y0 - 0.5) * log1p(delta / y0) + delta * log(y1) - delta
                      + (vmp_dgmm_stirling_tail(y1) - vmp_dgmm_stirling_tail(y0));
    return (st - logs) - lost;
}

// vmp_dgmm_update_tau with the count of the element `cnt` in the place of N_k: the same parameters
// and moments, bit for bit; the bound term with vmp_dgmm_lgamma_diff in the place of
// -lgamma(a0) + lgamma(a), the other terms and their order as there.
__host__ __device__ inline double vmp_dgmm_masked_update_tau(double a0, double b0, double mu1,
                                                             double mu2, double cnt, double s1,
                                                             double s2, double *par, double *mom)
{
    const double delta = 0.5 * cnt;
    const double a = a0 + delta;
    const double add = 0.5 * (s2 - 2.0 * mu1 * s1 + mu2 * cnt);     // b - b0
    const double b = b0 + add;
    const double psi = vmp_digamma(a), tau = a / b;
    par[0] = a;
    par[1] = b;
    mom[0] = tau;
    mom[1] = psi - log(b);
    return -a0 * log1p(add / b0) + (vmp_dgmm_lgamma_diff(a0, delta) - delta * psi) + add * tau;
}

// scal[2] from its three dot products
__host__ __device__ inline double vmp_dgmm_masked_dots(double s1h, double s2q, double mg)
{
    return (s1h + s2q) + mg;
}
