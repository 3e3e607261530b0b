// vmp_dgmm.hip -- the plate pass and the updates of the fused diagonal-Gaussian-mixture block
//
//     alpha = Dirichlet(a);  Z = Categorical(alpha, plates=(N, 1))
//     mu = GaussianARD(m0, beta0, plates=(D, K));  tau = Gamma(a0, b0, plates=(D, K))
//     Y = Mixture(Z, GaussianARD, mu, tau);  Y.observe(y)
//
// (the reference forms the (N, D, K) broadcast of the log-density and the (N, D, K) messages to mu
// and tau, mixture.py / gaussian.py / gamma.py).  One pass over the rows leaves the sufficient
// statistics only:
//
//   per tile of 64 rows   logit = Y h + (Y o Y) q, + c       (16 rows per wavefront, all of D)
//                         lse, r = exp(logit - lse)          (r goes to LDS, never to memory)
//                         N_k += sum r,  sum lse
//                         S1 += r^T Y,  S2 += r^T (Y o Y)    (all 64 rows, the (k, d) tiles dealt
//                                                             out to the four wavefronts)
//
// All four products run on v_mfma_f64_16x16x4_f64; y^2 is formed in registers from the y operand.
// Lane l of the instruction holds A[i = l & 15][k = l >> 4], B[k = l >> 4][j = l & 15] and the four
// results C[i = (l >> 4) + 4 r][j = l & 15] (vmp_bmm.hip: the result layout of the first product is
// the A layout of r^T for the second).
//
// D is walked in COLUMN BLOCKS of 64.  The y tile of a block (64 x 64 doubles, 32 KB) is staged in
// LDS; a block of S1 and S2 is 2 x 4 column tiles x KT cluster tiles, 2 KT per wavefront, held twice
// (the sums of the present tile of 64 rows, which start at zero, and the chunk's running sums,
// vmp_dgmm_dev.h): 4 KT accumulators of 4 doubles, 128 registers at K = 64.  With D <= 64 there is
// one block: its y tile stays in LDS between the two products, y is read from memory once, and the
// running sums live in registers through the chunk.  Above, the logits walk the blocks first, the
// second product walks them again (y is read a second time, from L2 where the tile still is
// there) and each block's running sums are carried through the chunk's partial in memory.
//
// No floating-point atomics: a workgroup owns a chunk of consecutive rows (vmp_dgmm_dev.h) and
// leaves one partial; dgmm_combine_kernel adds the partials in chunk order.
#include "vmp_common.h"
#include "vmp_dgmm_dev.h"

namespace {

constexpr int DGMM_NT = VMP_DGMM_NT;
constexpr int DB = VMP_DGMM_DBLOCK;

struct DgmmArgs {
    int64_t N, chunk;
    int D, K;
    const double *y;           // N x D
    const int32_t *labels;     // fixed classes (r = one-hot, lse = 0) or null
    const double *h, *q;       // D x K
    const double *c;           // K
    double *part;              // chunks x vmp_dgmm_partial_doubles
    double *r_out;             // N x K or null
};

// place of element (row t, column j) of the y tile in LDS: the column is XORed with a function of
// the row (below 32, so it stays inside the row of 64), which spreads both the A reads (16 rows,
// one column per lane quarter) and the B reads (16 columns, one row per lane quarter) over the banks
__device__ __forceinline__ int y_at(int t, int j)
{
    return t * DB + (j ^ (((t & 15) << 1) ^ ((t & 1) << 4)));
}

template <int KT>
__global__ void __launch_bounds__(DGMM_NT) dgmm_pass_kernel(DgmmArgs a)
{
    constexpr int KP = KT * 16;
    constexpr int NH = 2 * KT;                       // (k, d) tiles of a column block per wavefront
    __shared__ double y_s[VMP_DGMM_TILE * DB];       // the y tile of a block; the slots at the end
    __shared__ double r_s[VMP_DGMM_TILE * KP];       // responsibilities of the tile, row-major
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, l15 = l & 15, l4 = l >> 4;
    const int D = a.D, K = a.K;
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t r1 = (r0 + a.chunk < a.N) ? r0 + a.chunk : a.N;
    double *part = a.part + (int64_t)blockIdx.x * vmp_dgmm_partial_doubles(D, K);
    const int64_t DK = (int64_t)D * K;
    const int nblk = (D + DB - 1) / DB;
    const bool soft = a.labels == nullptr;

    double cval[KT], nk[KT];
#pragma unroll
    for (int kb = 0; kb < KT; ++kb) {
        const int k = kb * 16 + l15;
        cval[kb] = k < K ? a.c[k] : -INFINITY;
        nk[kb] = 0.0;
    }
    double lsum = 0.0;
    v4f64 acc[NH];                                   // the chunk's running sums
#pragma unroll
    for (int j = 0; j < NH; ++j) acc[j] = v4f64{0.0, 0.0, 0.0, 0.0};

    // rows row0 .. of columns d0 .. d0 + 63 into y_s; zeros beyond the chunk and beyond D
    auto load_y = [&](int64_t row0, int d0) {
        for (int i = tid; i < VMP_DGMM_TILE * DB; i += DGMM_NT) {
            const int t = i / DB, j = i % DB;
            const int64_t row = row0 + t;
            const int d = d0 + j;
            y_s[y_at(t, j)] = (row < r1 && d < D) ? a.y[row * D + d] : 0.0;
        }
    };

    for (int64_t row0 = r0; row0 < r1; row0 += VMP_DGMM_TILE) {
        // -- logits of this wavefront's 16 rows, block after block -------------------------------
        v4f64 lg[KT];
#pragma unroll
        for (int kb = 0; kb < KT; ++kb) lg[kb] = v4f64{0.0, 0.0, 0.0, 0.0};
        if (soft || nblk == 1) {
            for (int blk = 0; blk < nblk; ++blk) {
                const int d0 = blk * DB;
                if (blk > 0) __syncthreads();        // the block before has been read
                load_y(row0, d0);
                __syncthreads();
                if (!soft) continue;
                const int cols = (D - d0 < DB) ? D - d0 : DB;
                const int steps = (cols + 3) >> 2;
                for (int s = 0; s < steps; ++s) {
                    const int j = 4 * s + l4, d = d0 + j;
                    const double av = y_s[y_at(wave * 16 + l15, j)];
                    const double av2 = vmp_dgmm_square(av);
#pragma unroll
                    for (int kb = 0; kb < KT; ++kb) {
                        const int k = kb * 16 + l15;
                        const bool in = d < D && k < K;
                        const double bh = in ? a.h[(int64_t)d * K + k] : 0.0;
                        const double bq = in ? a.q[(int64_t)d * K + k] : 0.0;
                        lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bh, lg[kb], 0, 0, 0);
                        lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av2, bq, lg[kb], 0, 0, 0);
                    }
                }
            }
        }
        // the constant of the column comes last, as one addition (-inf for the padding)
#pragma unroll
        for (int kb = 0; kb < KT; ++kb)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
                lg[kb][qq] = vmp_dgmm_logit_finish(lg[kb][qq], cval[kb]);
        // -- softmax over the row: lane (l4, qq) holds columns l15, l15 + 16, ... of row l4 + 4 qq
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int t = wave * 16 + l4 + 4 * qq;
            const int64_t row = row0 + t;
            const bool valid = row < r1;
            double lse = 0.0;
            int lab = -1;
            if (soft) {
                double m = lg[0][qq];
#pragma unroll
                for (int kb = 1; kb < KT; ++kb) m = fmax(m, lg[kb][qq]);
                m = group16_max(m);
                double s = 0.0;
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) s += vmp_dgmm_shifted_exp(lg[kb][qq], m);
                s = group16_sum(s);
                lse = vmp_dgmm_lse(m, s);
            } else if (valid) {
                lab = a.labels[row];
            }
#pragma unroll
            for (int kb = 0; kb < KT; ++kb) {
                const int k = kb * 16 + l15;
                double rv = 0.0;
                if (valid) rv = soft ? vmp_dgmm_resp(lg[kb][qq], lse) : (k == lab ? 1.0 : 0.0);
                r_s[t * KP + k] = rv;
                nk[kb] += rv;
                if (a.r_out && valid && k < K) a.r_out[row * K + k] = rv;
            }
            if (valid) lsum += lse;
        }
        __syncthreads();

        // -- (S1, S2) += r^T (Y, Y o Y), block after block: per block the KT x ct tiles of S1 and
        // then those of S2, dealt out to the wavefronts.  The sums of the tile start at zero and
        // are added to the chunk's running sums once per tile (vmp_dgmm_dev.h).
        for (int blk = 0; blk < nblk; ++blk) {
            const int d0 = blk * DB;
            if (nblk > 1) {
                __syncthreads();                     // what y_s held has been read
                load_y(row0, d0);
                __syncthreads();
            }
            const int cols = (D - d0 < DB) ? D - d0 : DB;
            const int half = KT * ((cols + 15) >> 4);    // tiles of S1 in this block
            const int ntile = 2 * half;
            v4f64 tacc[NH];
#pragma unroll
            for (int j = 0; j < NH; ++j) tacc[j] = v4f64{0.0, 0.0, 0.0, 0.0};
            if (nblk > 1) {
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int tl = wave + 4 * j;
                    if (tl >= ntile) continue;
                    const int second = tl >= half, rem = second ? tl - half : tl;
                    const int kb = rem % KT, d = d0 + (rem / KT) * 16 + l15;
                    const int64_t po = second ? DK : 0;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int k = kb * 16 + l4 + 4 * qq;
                        acc[j][qq] = (row0 > r0 && k < K && d < D) ? part[po + (int64_t)k * D + d]
                                                                   : 0.0;
                    }
                }
            }
            for (int s = 0; s < 16; ++s) {
                const int t = 4 * s + l4;
                const double *rrow = r_s + t * KP;
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int tl = wave + 4 * j;
                    if (tl >= ntile) continue;
                    const int second = tl >= half, rem = second ? tl - half : tl;
                    const int kb = rem % KT, jc = (rem / KT) * 16 + l15;
                    const double av = rrow[kb * 16 + l15];
                    const double yv = y_s[y_at(t, jc)];
                    const double bv = second ? vmp_dgmm_square(yv) : yv;
                    tacc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, tacc[j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int j = 0; j < NH; ++j)
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) acc[j][qq] += tacc[j][qq];
            if (nblk > 1 || row0 + VMP_DGMM_TILE >= r1) {
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int tl = wave + 4 * j;
                    if (tl >= ntile) continue;
                    const int second = tl >= half, rem = second ? tl - half : tl;
                    const int kb = rem % KT, d = d0 + (rem / KT) * 16 + l15;
                    const int64_t po = second ? DK : 0;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int k = kb * 16 + l4 + 4 * qq;
                        if (k < K && d < D) part[po + (int64_t)k * D + d] = acc[j][qq];
                    }
                }
            }
        }
        __syncthreads();                 // r_s and y_s are free for the next tile
    }

    // -- N_k and sum lse: the 16 slots in slot order (they stand in y_s, which is free now) ------
    double *nk_s = y_s, *lse_s = y_s + 16 * KP;
#pragma unroll
    for (int kb = 0; kb < KT; ++kb) nk_s[(wave * 4 + l4) * KP + kb * 16 + l15] = nk[kb];
    if (l15 == 0) lse_s[wave * 4 + l4] = lsum;
    __syncthreads();
    if (tid < K) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += nk_s[s * KP + tid];
        part[2 * DK + tid] = t;
    }
    if (tid == 0) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += lse_s[s];
        part[2 * DK + K] = t;
    }
}

// one thread per (k, d): the partials in chunk order
__global__ void __launch_bounds__(DGMM_NT)
dgmm_combine_kernel(int64_t nc, int D, int K, const double *__restrict__ part,
                    double *__restrict__ S1, double *__restrict__ S2, double *__restrict__ Nk,
                    double *__restrict__ sum_lse)
{
    const int idx = blockIdx.x * DGMM_NT + threadIdx.x;
    if (idx >= D * K) return;
    const int k = idx / D, d = idx - k * D;
    const int64_t per = vmp_dgmm_partial_doubles(D, K), DK = (int64_t)D * K;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t c = 0; c < nc; ++c) {
        s1 += part[c * per + idx];
        s2 += part[c * per + DK + idx];
    }
    const int64_t e = (int64_t)d * K + k;
    S1[e] = s1;
    S2[e] = s2;
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

// scal[2]: S1 . h + S2 . q from the two dot products
__global__ void dgmm_add2_kernel(const double *__restrict__ two, double *__restrict__ out)
{
    out[0] = two[0] + two[1];
}

// h = <tau><mu>, q = -1/2 <tau>; gsum[k] = sum_d g[d, k] in ascending d; c = gsum + <log pi> less
// its largest element.  mu_mom, tau_mom: (D K, 2) or null (no observation term)
// ANN (deterministic annealing): h, q and gsum + <log pi> times `ab` before the maximum is taken
// out; gsum itself is not scaled (it feeds L_Y).  The plain instance ignores `ab`.
template <bool ANN>
__global__ void __launch_bounds__(DGMM_NT)
dgmm_tables_kernel(int D, int K, const double *__restrict__ mu_mom,
                   const double *__restrict__ tau_mom, const double *__restrict__ elog_pi,
                   double *__restrict__ h, double *__restrict__ q, double *__restrict__ c,
                   double *__restrict__ gsum, double ab)
{
    __shared__ double cs[VMP_DGMM_MAX_K];
    const int idx = blockIdx.x * DGMM_NT + threadIdx.x;
    const bool have = mu_mom && tau_mom;
    if (idx < D * K) {
        double hv = have ? vmp_dgmm_h(tau_mom[2 * (int64_t)idx], mu_mom[2 * (int64_t)idx]) : 0.0;
        double qv = have ? vmp_dgmm_q(tau_mom[2 * (int64_t)idx]) : 0.0;
        if constexpr (ANN) {
            hv = vmp_dgmm_anneal(ab, hv);
            qv = vmp_dgmm_anneal(ab, qv);
        }
        h[idx] = hv;
        q[idx] = qv;
    }
    if (blockIdx.x == 0) {
        if (idx < K) {
            double t = 0.0;
            if (have)
                for (int d = 0; d < D; ++d) {
                    const int64_t e = (int64_t)d * K + idx;
                    t += vmp_dgmm_g(tau_mom[2 * e], tau_mom[2 * e + 1], mu_mom[2 * e + 1]);
                }
            if (gsum) gsum[idx] = t;
            cs[idx] = t + elog_pi[idx];
            if constexpr (ANN) cs[idx] = vmp_dgmm_anneal(ab, cs[idx]);
        }
        __syncthreads();
        if (idx < K) {
            double m = cs[0];
            for (int k = 1; k < K; ++k) m = fmax(m, cs[k]);
            c[idx] = cs[idx] - m;
        }
    }
}

// one workgroup: element e belongs to thread e % 256; the 256 sums of the bound are halved
// eight times (vmp_dgmm_dev.h)
__global__ void __launch_bounds__(DGMM_NT)
dgmm_update_kernel(int D, int K, int which, const double *__restrict__ prior_a,
                   const double *__restrict__ prior_b, const double *__restrict__ S1,
                   const double *__restrict__ S2, const double *__restrict__ Nk,
                   const double *__restrict__ other, double *__restrict__ par,
                   double *__restrict__ mom, double *__restrict__ bound)
{
    __shared__ double bs[DGMM_NT];
    const int tid = threadIdx.x;
    const bool stats = S1 && S2 && Nk && other;
    double t = 0.0;
    for (int e = tid; e < D * K; e += DGMM_NT) {
        const int k = e % K;
        const double nk = stats ? Nk[k] : 0.0, s1 = stats ? S1[e] : 0.0, s2 = stats ? S2[e] : 0.0;
        const double o0 = stats ? other[2 * (int64_t)e] : 0.0;
        const double o1 = stats ? other[2 * (int64_t)e + 1] : 0.0;
        if (which == 0)
            t += vmp_dgmm_update_mu(prior_a[e], prior_b[e], o0, nk, s1, par + 2 * (int64_t)e,
                                    mom + 2 * (int64_t)e);
        else
            t += vmp_dgmm_update_tau(prior_a[e], prior_b[e], o0, o1, nk, s1, s2,
                                     par + 2 * (int64_t)e, mom + 2 * (int64_t)e);
    }
    bs[tid] = t;
    __syncthreads();
    block_halve_sum<DGMM_NT>(bs, tid);
    if (tid == 0) bound[0] = bs[0];
}

// The annealed update (which 0: mu, 1: tau) and, which 2 / 3, the parts alone of the q that par and
// mom hold: ab[0] = A, ab[1] = B, each the sum over the D K elements in the order of the plain
// bound term (element e to thread e % 256, the 256 sums halved eight times).
__global__ void __launch_bounds__(DGMM_NT)
dgmm_update_annealed_kernel(int D, int K, int which, double beta, const double *__restrict__ prior_a,
                            const double *__restrict__ prior_b, const double *__restrict__ S1,
                            const double *__restrict__ S2, const double *__restrict__ Nk,
                            const double *__restrict__ other, double *__restrict__ par,
                            double *__restrict__ mom, double *__restrict__ ab)
{
    __shared__ double as[DGMM_NT];
    __shared__ double bs[DGMM_NT];
    const int tid = threadIdx.x;
    const bool stats = S1 && S2 && Nk && other;
    double ta = 0.0, tb = 0.0;
    for (int e = tid; e < D * K; e += DGMM_NT) {
        const int k = e % K;
        double A, B;
        if (which >= 2) {
            if (which == 2) vmp_dgmm_parts_mu(prior_a[e], prior_b[e], par + 2 * (int64_t)e, &A, &B);
            else vmp_dgmm_parts_tau(prior_a[e], prior_b[e], par + 2 * (int64_t)e,
                                    mom + 2 * (int64_t)e, &A, &B);
        } else {
            const double nk = stats ? Nk[k] : 0.0, s1 = stats ? S1[e] : 0.0;
            const double s2 = stats ? S2[e] : 0.0;
            const double o0 = stats ? other[2 * (int64_t)e] : 0.0;
            const double o1 = stats ? other[2 * (int64_t)e + 1] : 0.0;
            if (which == 0)
                vmp_dgmm_update_mu_annealed(beta, prior_a[e], prior_b[e], o0, nk, s1,
                                            par + 2 * (int64_t)e, mom + 2 * (int64_t)e, &A, &B);
            else
                vmp_dgmm_update_tau_annealed(beta, prior_a[e], prior_b[e], o0, o1, nk, s1, s2,
                                             par + 2 * (int64_t)e, mom + 2 * (int64_t)e, &A, &B);
        }
        ta += A;
        tb += B;
    }
    as[tid] = ta;
    bs[tid] = tb;
    __syncthreads();
    block_halve_sum<DGMM_NT>(as, tid);
    block_halve_sum<DGMM_NT>(bs, tid);
    if (tid == 0) {
        ab[0] = as[0];
        ab[1] = bs[0];
    }
}

template <int KT>
void launch_pass(vmp_ctx *ctx, int64_t nc, const DgmmArgs &a)
{
    hipLaunchKernelGGL((dgmm_pass_kernel<KT>), dim3((unsigned)nc), dim3(DGMM_NT), 0, ctx->stream,
                       a);
}

}  // namespace

extern "C" {

int32_t vmp_dgmm_limits(int32_t *max_K, int32_t *max_D)
{
    if (!max_K || !max_D) return VMP_ERR_INVALID;
    *max_K = VMP_DGMM_MAX_K;
    *max_D = VMP_DGMM_MAX_D;
    return VMP_OK;
}

int32_t vmp_dgmm_plan(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                      int64_t *workspace_doubles)
{
    if (N < 0 || D < 1 || K < 1 || !chunk_rows || !workspace_doubles) return VMP_ERR_INVALID;
    if (K > VMP_DGMM_MAX_K || D > VMP_DGMM_MAX_D) return VMP_ERR_UNSUPPORTED;
    *chunk_rows = vmp_dgmm_chunk_rows(N, D, K);
    // the partials, the partial sums of a dot product, the two dot products of scal[2]
    *workspace_doubles = vmp_dgmm_chunks(N, D, K) * vmp_dgmm_partial_doubles(D, K) + 1024 + 2;
    return VMP_OK;
}

int32_t vmp_dgmm_tables(vmp_ctx *ctx, int32_t D, int32_t K, const double *mu_mom,
                        const double *tau_mom, const double *elog_pi, double *h, double *q,
                        double *c, double *gsum)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_DGMM_MAX_K && D <= VMP_DGMM_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_DGMM_MAX_D, VMP_DGMM_MAX_K);
    VMP_REQUIRE(ctx, elog_pi && h && q && c, VMP_ERR_INVALID, "null argument");
    hipLaunchKernelGGL(dgmm_tables_kernel<false>, dim3((unsigned)((D * K + DGMM_NT - 1) / DGMM_NT)),
                       dim3(DGMM_NT), 0, ctx->stream, D, K, mu_mom, tau_mom, elog_pi, h, q, c, gsum,
                       1.0);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_dgmm_tables_annealed(vmp_ctx *ctx, int32_t D, int32_t K, double annealing,
                                 const double *mu_mom, const double *tau_mom, const double *elog_pi,
                                 double *h, double *q, double *c, double *gsum)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_DGMM_MAX_K && D <= VMP_DGMM_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_DGMM_MAX_D, VMP_DGMM_MAX_K);
    VMP_REQUIRE(ctx, elog_pi && h && q && c, VMP_ERR_INVALID, "null argument");
    VMP_REQUIRE(ctx, annealing > 0.0 && annealing <= 1.0, VMP_ERR_INVALID,
                "annealing must be in (0, 1], got %g", annealing);
    hipLaunchKernelGGL(dgmm_tables_kernel<true>, dim3((unsigned)((D * K + DGMM_NT - 1) / DGMM_NT)),
                       dim3(DGMM_NT), 0, ctx->stream, D, K, mu_mom, tau_mom, elog_pi, h, q, c, gsum,
                       annealing);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_dgmm_pass(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, const double *y,
                      const int32_t *labels, const double *h, const double *q, const double *c,
                      double *ws, double *S1, double *S2, double *Nk, double *scal, double *r_out)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_DGMM_MAX_K && D <= VMP_DGMM_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_DGMM_MAX_D, VMP_DGMM_MAX_K);
    VMP_REQUIRE(ctx, h && q && c && ws && S1 && S2 && Nk && scal && (N == 0 || y),
                VMP_ERR_INVALID, "null argument");
    const int64_t nc = vmp_dgmm_chunks(N, D, K);
    if (nc > 0) {
        DgmmArgs a = {N, vmp_dgmm_chunk_rows(N, D, K), D, K, y, labels, h, q, c, ws, r_out};
        switch (vmp_dgmm_kpad(K) / 16) {
        case 1: launch_pass<1>(ctx, nc, a); break;
        case 2: launch_pass<2>(ctx, nc, a); break;
        case 3: launch_pass<3>(ctx, nc, a); break;
        default: launch_pass<4>(ctx, nc, a); break;
        }
    }
    hipLaunchKernelGGL(dgmm_combine_kernel, dim3((unsigned)((D * K + DGMM_NT - 1) / DGMM_NT)),
                       dim3(DGMM_NT), 0, ctx->stream, nc, D, K, ws, S1, S2, Nk, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    double *dot_ws = ws + nc * vmp_dgmm_partial_doubles(D, K), *two = dot_ws + 1024;
    int32_t rc = vmp_lda_dot(ctx, K, Nk, c, dot_ws, scal + 1);
    if (rc != VMP_OK) return rc;
    rc = vmp_lda_dot(ctx, (int64_t)D * K, S1, h, dot_ws, two);
    if (rc != VMP_OK) return rc;
    rc = vmp_lda_dot(ctx, (int64_t)D * K, S2, q, dot_ws, two + 1);
    if (rc != VMP_OK) return rc;
    hipLaunchKernelGGL(dgmm_add2_kernel, dim3(1), dim3(1), 0, ctx->stream, two, scal + 2);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_dgmm_update(vmp_ctx *ctx, int32_t D, int32_t K, int32_t which, const double *prior_a,
                        const double *prior_b, const double *S1, const double *S2,
                        const double *Nk, const double *other_mom, double *par, double *mom,
                        double *bound)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1 && (which == 0 || which == 1), VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_DGMM_MAX_K && D <= VMP_DGMM_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_DGMM_MAX_D, VMP_DGMM_MAX_K);
    VMP_REQUIRE(ctx, prior_a && prior_b && par && mom && bound, VMP_ERR_INVALID, "null argument");
    hipLaunchKernelGGL(dgmm_update_kernel, dim3(1), dim3(DGMM_NT), 0, ctx->stream, D, K, which,
                       prior_a, prior_b, S1, S2, Nk, other_mom, par, mom, bound);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_dgmm_update_annealed(vmp_ctx *ctx, int32_t D, int32_t K, int32_t which,
                                 double annealing, const double *prior_a, const double *prior_b,
                                 const double *S1, const double *S2, const double *Nk,
                                 const double *other_mom, double *par, double *mom, double *ab)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1 && which >= 0 && which <= 3, VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_DGMM_MAX_K && D <= VMP_DGMM_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_DGMM_MAX_D, VMP_DGMM_MAX_K);
    VMP_REQUIRE(ctx, prior_a && prior_b && par && mom && ab, VMP_ERR_INVALID, "null argument");
    VMP_REQUIRE(ctx, annealing > 0.0 && annealing <= 1.0, VMP_ERR_INVALID,
                "annealing must be in (0, 1], got %g", annealing);
    hipLaunchKernelGGL(dgmm_update_annealed_kernel, dim3(1), dim3(DGMM_NT), 0, ctx->stream, D, K,
                       which, annealing, prior_a, prior_b, S1, S2, Nk, other_mom, par, mom, ab);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
