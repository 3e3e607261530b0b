// vmp_bmm.hip -- the plate pass of the fused Bernoulli-mixture block
//
//     R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
//     P = Beta([a, b], plates=(D, K));  X = Mixture(Z, Bernoulli, P);  X.observe(x)
//
// (doc/source/examples/bmm.rst; the reference forms the (N, D, K) broadcast of
// x <log p> + (1 - x) <log(1 - p)>, the (N, D, K) message to P and the (N, K) responsibilities,
// mixture.py / bernoulli.py / categorical.py).  Here x is kept as bits (vmp_bmm_pack) and one pass
// over the rows leaves the sufficient statistics only:
//
//   per tile of 64 rows   logit = c + X_tile w          (16 rows per wavefront, all of D)
//                         lse, r = exp(logit - lse)     (r goes to LDS, never to memory)
//                         N_k += sum r,  sum lse
//                         S[k, d] += r^T X_tile         (all 64 rows, the (k, d) tiles dealt out
//                                                        to the four wavefronts)
//
// Both products run on v_mfma_f64_16x16x4_f64; the 0 / 1 operand is unpacked from the words in
// registers.  Lane l of the instruction holds A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15]
// and the four results C[i = (l >> 4) + 4 r][j = l & 15].  For logit = X w the result layout
// (row (l >> 4) + 4 r, column l & 15) is at once the A layout of r^T for the second product
// (i = column k, contraction index = row), so r needs no transposition, only the trip through LDS
// that lets every wavefront see all 64 rows.
//
// S is held in accumulators for one block of 256 columns at a time: K = 64 and 256 columns are 64
// tiles of 16 x 16, 16 tiles = 128 registers per wavefront.  With D <= 256 the accumulators live
// through the whole chunk; above, the workgroup walks the column blocks per tile and carries each
// block's accumulators through its own partial in memory (the same chain of additions).
//
// No floating-point atomics: a workgroup owns a chunk of consecutive rows (vmp_bmm_dev.h) and
// leaves one partial S, N_k and sum lse; bmm_combine_kernel adds the partials in chunk order.
//
// Missing observations (the MASKED instances, vmp_bmm_dev.h): a row is two bit planes, x & m and m.
// The first product runs over plane 0 against w and then over plane 1 against l0; the second gives
// S from plane 0 and M from plane 1.  The two results are one row of 2 ceil(D / 16) column tiles,
// walked in blocks of 8 tiles.  Half of the accumulators hold the sums of the present tile of 64
// rows, which start at zero; the other half hold the chunk's running sums, to which the tile's are
// added once per tile (sums of many equal terms, as a small D gives, drift less that way).  Up to
// D = 64 the running sums are resident through the chunk, above they are carried through the
// partial like the 256-column blocks above.
#include "vmp_common.h"
#include "vmp_bmm_dev.h"

namespace {

constexpr int BMM_NT = 256;

struct BmmArgs {
    int64_t N, chunk;
    int D, K, W;
    const uint64_t *xw;        // N x W packed rows
    const int32_t *labels;     // fixed classes (r = one-hot, lse = 0) or null
    const double *w;           // D x K
    const double *c;           // K
    double *part;              // chunks x vmp_bmm_partial_doubles
    double *r_out;             // N x K or null
};

struct BmmMaskedArgs : BmmArgs {   // xw: N x 2 W, part: chunks x vmp_bmm_partial_doubles_masked
    const double *l0;              // D x K
};

template <bool MASKED> struct BmmArgsOf { using type = BmmArgs; };
template <> struct BmmArgsOf<true> { using type = BmmMaskedArgs; };

template <int KT, bool MASKED>
__global__ void __launch_bounds__(BMM_NT) bmm_pass_kernel(typename BmmArgsOf<MASKED>::type a)
{
    constexpr int KP = KT * 16;
    constexpr int NJ = 4 * KT;                       // (k, d) tiles of a column block per wavefront
    __shared__ double r_s[VMP_BMM_TILE * KP];        // responsibilities of the tile, row-major
    __shared__ uint64_t x_s[VMP_BMM_TILE * (VMP_BMM_MAX_D / 64) * (MASKED ? 2 : 1)];
    __shared__ double nk_s[16 * KP];
    __shared__ double lse_s[16];
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, l15 = l & 15, l4 = l >> 4;
    const int D = a.D, K = a.K, W = a.W;
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t r1 = (r0 + a.chunk < a.N) ? r0 + a.chunk : a.N;
    const int WR = MASKED ? 2 * W : W;               // words of a row
    double *part = a.part + (int64_t)blockIdx.x * (MASKED ? vmp_bmm_partial_doubles_masked(D, K)
                                                          : vmp_bmm_partial_doubles(D, K));
    const int DT = (D + 15) >> 4;                    // column tiles of a plane (MASKED)
    const int nblk = MASKED ? (2 * DT + 7) >> 3 : (D + VMP_BMM_DBLOCK - 1) / VMP_BMM_DBLOCK;
    const bool soft = a.labels == nullptr;

    double cval[KT], nk[KT];
#pragma unroll
    for (int kb = 0; kb < KT; ++kb) {
        const int k = kb * 16 + l15;
        cval[kb] = k < K ? a.c[k] : -INFINITY;
        nk[kb] = 0.0;
    }
    double lsum = 0.0;
    constexpr int NH = NJ / 2;                       // MASKED: running sums and tile sums
    v4f64 acc[MASKED ? NH : NJ];
#pragma unroll
    for (int j = 0; j < (MASKED ? NH : NJ); ++j) acc[j] = v4f64{0.0, 0.0, 0.0, 0.0};

    for (int64_t row0 = r0; row0 < r1; row0 += VMP_BMM_TILE) {
        for (int i = tid; i < VMP_BMM_TILE * WR; i += BMM_NT) {
            const int64_t row = row0 + i / WR;
            x_s[i] = row < r1 ? a.xw[row * WR + (i % WR)] : 0;
        }
        __syncthreads();

        // -- logits of this wavefront's 16 rows ------------------------------------------------
        v4f64 lg[KT];
#pragma unroll
        for (int kb = 0; kb < KT; ++kb) lg[kb] = v4f64{0.0, 0.0, 0.0, 0.0};
        if (soft) {
            const uint64_t *myrow = x_s + (wave * 16 + l15) * WR;
            const int steps = (D + 3) >> 2;
            for (int s = 0; s < steps; ++s) {
                const int d = 4 * s + l4;
                const double av = vmp_bmm_bit(myrow, d);
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) {
                    const int k = kb * 16 + l15;
                    const double bv = (d < D && k < K) ? a.w[(int64_t)d * K + k] : 0.0;
                    lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, lg[kb], 0, 0, 0);
                }
            }
            if constexpr (MASKED) {
                // the mask plane against l0, after all of plane 0
                for (int s = 0; s < steps; ++s) {
                    const int d = 4 * s + l4;
                    const double av = vmp_bmm_bit(myrow + W, d);
#pragma unroll
                    for (int kb = 0; kb < KT; ++kb) {
                        const int k = kb * 16 + l15;
                        const double bv = (d < D && k < K) ? a.l0[(int64_t)d * K + k] : 0.0;
                        lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, lg[kb], 0, 0, 0);
                    }
                }
            }
        }
        // the constant of the column comes last, as one addition (-inf for the padding)
#pragma unroll
        for (int kb = 0; kb < KT; ++kb)
#pragma unroll
            for (int q = 0; q < 4; ++q) lg[kb][q] = vmp_bmm_logit_finish(lg[kb][q], cval[kb]);
        // -- softmax over the row: lane (l4, q) holds columns l15, l15 + 16, ... of row l4 + 4 q
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int t = wave * 16 + l4 + 4 * q;
            const int64_t row = row0 + t;
            const bool valid = row < r1;
            // a row with no observed bit keeps its r for r_out and adds nothing to the sums
            bool counted = valid;
            if constexpr (MASKED) counted = valid && vmp_bmm_row_observed(x_s + t * WR + W, W);
            double lse = 0.0;
            int lab = -1;
            if (soft) {
                double m = lg[0][q];
#pragma unroll
                for (int kb = 1; kb < KT; ++kb) m = fmax(m, lg[kb][q]);
                m = group16_max(m);
                double s = 0.0;
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) s += vmp_bmm_shifted_exp(lg[kb][q], m);
                s = group16_sum(s);
                lse = vmp_bmm_lse(m, s);
            } else if (valid) {
                lab = a.labels[row];
            }
#pragma unroll
            for (int kb = 0; kb < KT; ++kb) {
                const int k = kb * 16 + l15;
                double rv = 0.0;
                if (valid) rv = soft ? vmp_bmm_resp(lg[kb][q], lse) : (k == lab ? 1.0 : 0.0);
                if constexpr (MASKED) {
                    const double rs = counted ? rv : 0.0;    // r_out keeps the r of a row of nothing
                    r_s[t * KP + k] = rs;
                    nk[kb] += rs;
                } else {
                    r_s[t * KP + k] = rv;
                    nk[kb] += rv;
                }
                if (a.r_out && valid && k < K) a.r_out[row * K + k] = rv;
            }
            if (counted) lsum += lse;
        }
        __syncthreads();

        if constexpr (MASKED) {
            // -- (S, M) += r^T (plane 0, plane 1): the 2 DT column tiles in blocks of 8.  The sums
            // of the tile start at zero and are added to the chunk's running sums once per tile
            // (vmp_bmm_dev.h); half of the accumulators hold each.
            for (int blk = 0; blk < nblk; ++blk) {
                const int ct0 = blk * 8;
                const int ntile = KT * ((2 * DT - ct0 < 8) ? 2 * DT - ct0 : 8);
                v4f64 tacc[NH];
#pragma unroll
                for (int j = 0; j < NH; ++j) tacc[j] = v4f64{0.0, 0.0, 0.0, 0.0};
                if (nblk > 1) {
#pragma unroll
                    for (int j = 0; j < NH; ++j) {
                        const int tl = wave + 4 * j;
                        if (tl >= ntile) continue;
                        const int kb = tl % KT, ct = ct0 + tl / KT;
                        const int d = (ct < DT ? ct : ct - DT) * 16 + l15;
                        const int64_t po = ct < DT ? 0 : (int64_t)D * K;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int k = kb * 16 + l4 + 4 * q;
                            acc[j][q] = (row0 > r0 && k < K && d < D) ? part[po + (int64_t)k * D + d]
                                                                      : 0.0;
                        }
                    }
                }
                for (int s = 0; s < 16; ++s) {
                    const int t = 4 * s + l4;
                    const double *rrow = r_s + t * KP;
                    const uint64_t *xrow = x_s + t * WR;
#pragma unroll
                    for (int j = 0; j < NH; ++j) {
                        const int tl = wave + 4 * j;
                        if (tl >= ntile) continue;
                        const int kb = tl % KT, ct = ct0 + tl / KT;
                        const int d = (ct < DT ? ct : ct - DT) * 16 + l15;
                        const double av = rrow[kb * 16 + l15];
                        const double bv = vmp_bmm_bit(xrow + (ct < DT ? 0 : W), d);
                        tacc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, tacc[j], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int j = 0; j < NH; ++j)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[j][q] += tacc[j][q];
                if (nblk > 1 || row0 + VMP_BMM_TILE >= r1) {
#pragma unroll
                    for (int j = 0; j < NH; ++j) {
                        const int tl = wave + 4 * j;
                        if (tl >= ntile) continue;
                        const int kb = tl % KT, ct = ct0 + tl / KT;
                        const int d = (ct < DT ? ct : ct - DT) * 16 + l15;
                        const int64_t po = ct < DT ? 0 : (int64_t)D * K;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int k = kb * 16 + l4 + 4 * q;
                            if (k < K && d < D) part[po + (int64_t)k * D + d] = acc[j][q];
                        }
                    }
                }
            }
        } else {
            // -- S += r^T X_tile, one block of 256 columns at a time ----------------------------------
            for (int blk = 0; blk < nblk; ++blk) {
                const int d0 = blk * VMP_BMM_DBLOCK;
                const int dt = (((D - d0 < VMP_BMM_DBLOCK) ? D - d0 : VMP_BMM_DBLOCK) + 15) >> 4;
                const int ntile = KT * dt;
                if (nblk > 1) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int tl = wave + 4 * j;
                        if (tl >= ntile) continue;
                        const int kb = tl % KT, d = d0 + (tl / KT) * 16 + l15;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int k = kb * 16 + l4 + 4 * q;
                            acc[j][q] = (row0 > r0 && k < K && d < D) ? part[(int64_t)k * D + d] : 0.0;
                        }
                    }
                }
                for (int s = 0; s < 16; ++s) {
                    const int t = 4 * s + l4;
                    const double *rrow = r_s + t * KP;
                    const uint64_t *xrow = x_s + t * W;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int tl = wave + 4 * j;
                        if (tl >= ntile) continue;
                        const int kb = tl % KT, d = d0 + (tl / KT) * 16 + l15;
                        const double av = rrow[kb * 16 + l15];
                        const double bv = vmp_bmm_bit(xrow, d);
                        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[j], 0, 0, 0);
                    }
                }
                if (nblk > 1 || row0 + VMP_BMM_TILE >= r1) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        const int tl = wave + 4 * j;
                        if (tl >= ntile) continue;
                        const int kb = tl % KT, d = d0 + (tl / KT) * 16 + l15;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int k = kb * 16 + l4 + 4 * q;
                            if (k < K && d < D) part[(int64_t)k * D + d] = acc[j][q];
                        }
                    }
                }
            }
        }
        __syncthreads();                 // r_s and x_s are free for the next tile
    }

    // -- N_k and sum lse: the 16 slots in slot order ---------------------------------------------
#pragma unroll
    for (int kb = 0; kb < KT; ++kb) nk_s[(wave * 4 + l4) * KP + kb * 16 + l15] = nk[kb];
    if (l15 == 0) lse_s[wave * 4 + l4] = lsum;
    __syncthreads();
    if (tid < K) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += nk_s[s * KP + tid];
        part[(MASKED ? 2 : 1) * (int64_t)D * K + tid] = t;
    }
    if (tid == 0) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += lse_s[s];
        part[(MASKED ? 2 : 1) * (int64_t)D * K + K] = t;
    }
}

// the masked pass: S, M and counts = (S, M - S) per (k, d), the partials in chunk order
__global__ void __launch_bounds__(BMM_NT)
bmm_combine_masked_kernel(int64_t nc, int D, int K, const double *__restrict__ part,
                          double *__restrict__ S, double *__restrict__ M, double *__restrict__ Nk,
                          double *__restrict__ counts, double *__restrict__ sum_lse)
{
    const int idx = blockIdx.x * BMM_NT + threadIdx.x;
    if (idx >= D * K) return;
    const int k = idx / D, d = idx - k * D;
    const int64_t per = vmp_bmm_partial_doubles_masked(D, K), DK = (int64_t)D * K;
    double s = 0.0, m = 0.0;
    for (int64_t c = 0; c < nc; ++c) {
        s += part[c * per + idx];
        m += part[c * per + DK + idx];
    }
    const int64_t e = (int64_t)d * K + k;
    S[e] = s;
    M[e] = m;
    counts[2 * e] = s;
    counts[2 * e + 1] = m - s;
    if (d == 0) {
        double n = 0.0;
        for (int64_t c = 0; c < nc; ++c) n += part[c * per + 2 * DK + k];
        Nk[k] = n;
    }
    if (idx == 0) {
        double t = 0.0;
        for (int64_t c = 0; c < nc; ++c) t += part[c * per + 2 * DK + K];
        sum_lse[0] = t;
    }
}

// scal[2] of the masked pass: S . w + M . l0 from the two dot products
__global__ void bmm_add2_kernel(const double *__restrict__ two, double *__restrict__ out)
{
    out[0] = two[0] + two[1];
}

// w = <log p> - <log(1 - p)>, l0 = <log(1 - p)>; c = <log pi> less its largest element
__global__ void __launch_bounds__(BMM_NT)
bmm_tables_masked_kernel(int D, int K, const double *__restrict__ elog_p,
                         const double *__restrict__ elog_pi, double *__restrict__ w,
                         double *__restrict__ l0, double *__restrict__ c)
{
    const int idx = blockIdx.x * BMM_NT + threadIdx.x;
    if (idx < D * K) {
        w[idx] = elog_p ? elog_p[2 * (int64_t)idx] - elog_p[2 * (int64_t)idx + 1] : 0.0;
        l0[idx] = elog_p ? elog_p[2 * (int64_t)idx + 1] : 0.0;
    }
    if (blockIdx.x == 0 && idx < K) {
        double m = elog_pi[0];
        for (int k = 1; k < K; ++k) m = fmax(m, elog_pi[k]);
        c[idx] = elog_pi[idx] - m;
    }
}

// one thread per (k, d): the partials in chunk order; the Beta counts (S, N_k - S) as (D K, 2)
__global__ void __launch_bounds__(BMM_NT)
bmm_combine_kernel(int64_t nc, int D, int K, const double *__restrict__ part,
                   double *__restrict__ S, double *__restrict__ Nk, double *__restrict__ counts,
                   double *__restrict__ sum_lse)
{
    const int idx = blockIdx.x * BMM_NT + threadIdx.x;
    if (idx >= D * K) return;
    const int k = idx / D, d = idx - k * D;
    const int64_t per = vmp_bmm_partial_doubles(D, K);
    double s = 0.0, n = 0.0;
    for (int64_t c = 0; c < nc; ++c) {
        s += part[c * per + idx];
        n += part[c * per + (int64_t)D * K + k];
    }
    const int64_t e = (int64_t)d * K + k;
    S[e] = s;
    counts[2 * e] = s;
    counts[2 * e + 1] = n - s;
    if (d == 0) Nk[k] = n;
    if (idx == 0) {
        double t = 0.0;
        for (int64_t c = 0; c < nc; ++c) t += part[c * per + (int64_t)D * K + K];
        sum_lse[0] = t;
    }
}

// w = <log p> - <log(1 - p)>; c = <log pi> + sum_d <log(1 - p)> (the sum in ascending d, <log pi>
// last) less its largest element; elog_p: (D K, 2)
__global__ void __launch_bounds__(BMM_NT)
bmm_tables_kernel(int D, int K, const double *__restrict__ elog_p,
                  const double *__restrict__ elog_pi, double *__restrict__ w,
                  double *__restrict__ c)
{
    __shared__ double cs[VMP_BMM_MAX_K];
    const int idx = blockIdx.x * BMM_NT + threadIdx.x;
    if (idx < D * K) w[idx] = elog_p ? elog_p[2 * (int64_t)idx] - elog_p[2 * (int64_t)idx + 1] : 0.0;
    if (blockIdx.x == 0) {
        if (idx < K) {
            double t = 0.0;
            if (elog_p)
                for (int d = 0; d < D; ++d) t += elog_p[2 * ((int64_t)d * K + idx) + 1];
            cs[idx] = t + elog_pi[idx];
        }
        __syncthreads();
        if (idx < K) {
            double m = cs[0];
            for (int k = 1; k < K; ++k) m = fmax(m, cs[k]);
            c[idx] = cs[idx] - m;
        }
    }
}

template <typename T>
__global__ void __launch_bounds__(BMM_NT)
bmm_pack_kernel(int64_t N, int D, int W, const T *__restrict__ x, uint64_t *__restrict__ xw,
                int32_t *flag)
{
    const int64_t idx = (int64_t)blockIdx.x * BMM_NT + threadIdx.x;
    if (idx >= N * W) return;
    const int64_t row = idx / W;
    const int wd = (int)(idx - row * W);
    const int d0 = wd * 64, d1 = (d0 + 64 < D) ? d0 + 64 : D;
    uint64_t bits = 0;
    bool bad = false;
    for (int d = d0; d < d1; ++d) {
        const T v = x[row * D + d];
        if (v == (T)1) bits |= (uint64_t)1 << (d - d0);
        else if (!(v == (T)0)) bad = true;
    }
    xw[idx] = bits;
    if (bad) *flag = 1;
}

// plane 0 = x & m, plane 1 = m of one row and word; only observed values are looked at
template <typename T>
__global__ void __launch_bounds__(BMM_NT)
bmm_pack_masked_kernel(int64_t N, int D, int W, const T *__restrict__ x,
                       const uint8_t *__restrict__ mask, uint64_t *__restrict__ xw, int32_t *flag)
{
    const int64_t idx = (int64_t)blockIdx.x * BMM_NT + threadIdx.x;
    if (idx >= N * W) return;
    const int64_t row = idx / W;
    const int wd = (int)(idx - row * W);
    const int d0 = wd * 64, d1 = (d0 + 64 < D) ? d0 + 64 : D;
    uint64_t bits = 0, mbits = 0;
    bool bad = false;
    for (int d = d0; d < d1; ++d) {
        if (!mask[row * D + d]) continue;
        mbits |= (uint64_t)1 << (d - d0);
        const T v = x[row * D + d];
        if (v == (T)1) bits |= (uint64_t)1 << (d - d0);
        else if (!(v == (T)0)) bad = true;
    }
    xw[row * 2 * W + wd] = bits;
    xw[row * 2 * W + W + wd] = mbits;
    if (bad) *flag = 1;
}

template <int KT>
void launch_pass(vmp_ctx *ctx, int64_t nc, const BmmArgs &a)
{
    hipLaunchKernelGGL((bmm_pass_kernel<KT, false>), dim3((unsigned)nc), dim3(BMM_NT), 0,
                       ctx->stream, a);
}

template <int KT>
void launch_pass_masked(vmp_ctx *ctx, int64_t nc, const BmmMaskedArgs &a)
{
    hipLaunchKernelGGL((bmm_pass_kernel<KT, true>), dim3((unsigned)nc), dim3(BMM_NT), 0,
                       ctx->stream, a);
}

}  // namespace

extern "C" {

int32_t vmp_bmm_limits(int32_t *max_K, int32_t *max_D)
{
    if (!max_K || !max_D) return VMP_ERR_INVALID;
    *max_K = VMP_BMM_MAX_K;
    *max_D = VMP_BMM_MAX_D;
    return VMP_OK;
}

int32_t vmp_bmm_plan(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                     int64_t *workspace_doubles)
{
    if (N < 0 || D < 1 || K < 1 || !chunk_rows || !workspace_doubles) return VMP_ERR_INVALID;
    if (K > VMP_BMM_MAX_K || D > VMP_BMM_MAX_D) return VMP_ERR_UNSUPPORTED;
    *chunk_rows = vmp_bmm_chunk_rows(N, D, K);
    *workspace_doubles = vmp_bmm_chunks(N, D, K) * vmp_bmm_partial_doubles(D, K) + 1024;
    return VMP_OK;
}

int32_t vmp_bmm_pack(vmp_ctx *ctx, int64_t N, int32_t D, int32_t dtype, const void *x,
                     uint64_t *xw, int32_t *flag)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && dtype >= 0 && dtype <= 2, VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, D <= VMP_BMM_MAX_D, VMP_ERR_UNSUPPORTED, "D = %d exceeds the limit %d", D,
                VMP_BMM_MAX_D);
    VMP_REQUIRE(ctx, flag && (N == 0 || (x && xw)), VMP_ERR_INVALID, "null argument");
    if (N == 0) return VMP_OK;
    const int W = vmp_bmm_words(D);
    const dim3 grid((unsigned)((N * W + BMM_NT - 1) / BMM_NT));
    if (dtype == 0)
        hipLaunchKernelGGL(bmm_pack_kernel<double>, grid, dim3(BMM_NT), 0, ctx->stream, N, D, W,
                           (const double *)x, xw, flag);
    else if (dtype == 1)
        hipLaunchKernelGGL(bmm_pack_kernel<int64_t>, grid, dim3(BMM_NT), 0, ctx->stream, N, D, W,
                           (const int64_t *)x, xw, flag);
    else
        hipLaunchKernelGGL(bmm_pack_kernel<uint8_t>, grid, dim3(BMM_NT), 0, ctx->stream, N, D, W,
                           (const uint8_t *)x, xw, flag);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_bmm_tables(vmp_ctx *ctx, int32_t D, int32_t K, const double *elog_p,
                       const double *elog_pi, double *w, double *c)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_BMM_MAX_K && D <= VMP_BMM_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_BMM_MAX_D, VMP_BMM_MAX_K);
    VMP_REQUIRE(ctx, elog_pi && w && c, VMP_ERR_INVALID, "null argument");
    hipLaunchKernelGGL(bmm_tables_kernel, dim3((unsigned)((D * K + BMM_NT - 1) / BMM_NT)),
                       dim3(BMM_NT), 0, ctx->stream, D, K, elog_p, elog_pi, w, c);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_bmm_pass(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, const uint64_t *xw,
                     const int32_t *labels, const double *w, const double *c, double *ws,
                     double *S, double *Nk, double *counts, double *scal, double *r_out)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_BMM_MAX_K && D <= VMP_BMM_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_BMM_MAX_D, VMP_BMM_MAX_K);
    VMP_REQUIRE(ctx, w && c && ws && S && Nk && counts && scal && (N == 0 || xw),
                VMP_ERR_INVALID, "null argument");
    const int64_t nc = vmp_bmm_chunks(N, D, K);
    if (nc > 0) {
        BmmArgs a = {N, vmp_bmm_chunk_rows(N, D, K), D, K, vmp_bmm_words(D), xw, labels, w, c, ws,
                     r_out};
        switch (vmp_bmm_kpad(K) / 16) {
        case 1: launch_pass<1>(ctx, nc, a); break;
        case 2: launch_pass<2>(ctx, nc, a); break;
        case 3: launch_pass<3>(ctx, nc, a); break;
        default: launch_pass<4>(ctx, nc, a); break;
        }
    }
    hipLaunchKernelGGL(bmm_combine_kernel, dim3((unsigned)((D * K + BMM_NT - 1) / BMM_NT)),
                       dim3(BMM_NT), 0, ctx->stream, nc, D, K, ws, S, Nk, counts, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    double *dot_ws = ws + nc * vmp_bmm_partial_doubles(D, K);
    int32_t rc = vmp_lda_dot(ctx, K, Nk, c, dot_ws, scal + 1);
    if (rc != VMP_OK) return rc;
    return vmp_lda_dot(ctx, (int64_t)D * K, S, w, dot_ws, scal + 2);
}

int32_t vmp_bmm_limits_masked(int32_t *max_K, int32_t *max_D)
{
    if (!max_K || !max_D) return VMP_ERR_INVALID;
    *max_K = VMP_BMM_MASKED_MAX_K;
    *max_D = VMP_BMM_MASKED_MAX_D;
    return VMP_OK;
}

int32_t vmp_bmm_plan_masked(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                            int64_t *workspace_doubles)
{
    if (N < 0 || D < 1 || K < 1 || !chunk_rows || !workspace_doubles) return VMP_ERR_INVALID;
    if (K > VMP_BMM_MASKED_MAX_K || D > VMP_BMM_MASKED_MAX_D) return VMP_ERR_UNSUPPORTED;
    *chunk_rows = vmp_bmm_chunk_rows_masked(N, D, K);
    // the partials, the partial sums of a dot product, the two dot products of scal[2]
    *workspace_doubles = vmp_bmm_chunks_masked(N, D, K) * vmp_bmm_partial_doubles_masked(D, K)
                         + 1024 + 2;
    return VMP_OK;
}

int32_t vmp_bmm_pack_masked(vmp_ctx *ctx, int64_t N, int32_t D, int32_t dtype, const void *x,
                            const uint8_t *mask, uint64_t *xw, int32_t *flag)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && dtype >= 0 && dtype <= 2, VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, D <= VMP_BMM_MASKED_MAX_D, VMP_ERR_UNSUPPORTED, "D = %d exceeds the limit %d",
                D, VMP_BMM_MASKED_MAX_D);
    VMP_REQUIRE(ctx, flag && (N == 0 || (x && mask && xw)), VMP_ERR_INVALID, "null argument");
    if (N == 0) return VMP_OK;
    const int W = vmp_bmm_words(D);
    const dim3 grid((unsigned)((N * W + BMM_NT - 1) / BMM_NT));
    if (dtype == 0)
        hipLaunchKernelGGL(bmm_pack_masked_kernel<double>, grid, dim3(BMM_NT), 0, ctx->stream, N,
                           D, W, (const double *)x, mask, xw, flag);
    else if (dtype == 1)
        hipLaunchKernelGGL(bmm_pack_masked_kernel<int64_t>, grid, dim3(BMM_NT), 0, ctx->stream, N,
                           D, W, (const int64_t *)x, mask, xw, flag);
    else
        hipLaunchKernelGGL(bmm_pack_masked_kernel<uint8_t>, grid, dim3(BMM_NT), 0, ctx->stream, N,
                           D, W, (const uint8_t *)x, mask, xw, flag);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_bmm_tables_masked(vmp_ctx *ctx, int32_t D, int32_t K, const double *elog_p,
                              const double *elog_pi, double *w, double *l0, double *c)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_BMM_MASKED_MAX_K && D <= VMP_BMM_MASKED_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_BMM_MASKED_MAX_D,
                VMP_BMM_MASKED_MAX_K);
    VMP_REQUIRE(ctx, elog_pi && w && l0 && c, VMP_ERR_INVALID, "null argument");
    hipLaunchKernelGGL(bmm_tables_masked_kernel, dim3((unsigned)((D * K + BMM_NT - 1) / BMM_NT)),
                       dim3(BMM_NT), 0, ctx->stream, D, K, elog_p, elog_pi, w, l0, c);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_bmm_pass_masked(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, const uint64_t *xw,
                            const int32_t *labels, const double *w, const double *l0,
                            const double *c, double *ws, double *S, double *M, double *Nk,
                            double *counts, double *scal, double *r_out)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_BMM_MASKED_MAX_K && D <= VMP_BMM_MASKED_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_BMM_MASKED_MAX_D,
                VMP_BMM_MASKED_MAX_K);
    VMP_REQUIRE(ctx, w && l0 && c && ws && S && M && Nk && counts && scal && (N == 0 || xw),
                VMP_ERR_INVALID, "null argument");
    const int64_t nc = vmp_bmm_chunks_masked(N, D, K);
    if (nc > 0) {
        BmmMaskedArgs a = {{N, vmp_bmm_chunk_rows_masked(N, D, K), D, K, vmp_bmm_words(D), xw,
                            labels, w, c, ws, r_out}, l0};
        switch (vmp_bmm_kpad(K) / 16) {
        case 1: launch_pass_masked<1>(ctx, nc, a); break;
        case 2: launch_pass_masked<2>(ctx, nc, a); break;
        case 3: launch_pass_masked<3>(ctx, nc, a); break;
        default: launch_pass_masked<4>(ctx, nc, a); break;
        }
    }
    hipLaunchKernelGGL(bmm_combine_masked_kernel, dim3((unsigned)((D * K + BMM_NT - 1) / BMM_NT)),
                       dim3(BMM_NT), 0, ctx->stream, nc, D, K, ws, S, M, Nk, counts, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    double *dot_ws = ws + nc * vmp_bmm_partial_doubles_masked(D, K), *two = dot_ws + 1024;
    int32_t rc = vmp_lda_dot(ctx, K, Nk, c, dot_ws, scal + 1);
    if (rc != VMP_OK) return rc;
    rc = vmp_lda_dot(ctx, (int64_t)D * K, S, w, dot_ws, two);
    if (rc != VMP_OK) return rc;
    rc = vmp_lda_dot(ctx, (int64_t)D * K, M, l0, dot_ws, two + 1);
    if (rc != VMP_OK) return rc;
    hipLaunchKernelGGL(bmm_add2_kernel, dim3(1), dim3(1), 0, ctx->stream, two, scal + 2);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
