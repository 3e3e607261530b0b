// vmp_dgmm_masked.hip -- the fused diagonal-Gaussian-mixture block with missing observations
//
//     alpha = Dirichlet(a);  Z = Categorical(alpha, plates=(N, 1))
//     mu = GaussianARD(m0, beta0, plates=(D, K));  tau = Gamma(a0, b0, plates=(D, K))
//     Y = Mixture(Z, GaussianARD, mu, tau);  Y.observe(y, mask=m)             y, m (N, D)
//
// The pass of vmp_dgmm.hip with a third product (vmp_dgmm_masked_dev.h):
//
//   per tile of 64 rows   logit = M g + Yt h + (Yt o Yt) q, + c     (16 rows per wavefront, all of D)
//                         lse, r = exp(logit - lse)                 (r goes to LDS, never to memory)
//                         N_k += sum r, sum lse                     (rows with an observed entry)
//                         M += r^T M,  S1 += r^T Yt,  S2 += r^T (Yt o Yt)
//
// All six products run on v_mfma_f64_16x16x4_f64 (operand layout: vmp_dgmm.hip).  The mask is not
// read: the packed y holds one quiet-NaN pattern at the hidden positions, and m = (y == y),
// yt = m ? y : 0 and yt^2 are formed in registers from the staged value, by selects.
//
// D is walked in COLUMN BLOCKS of 32.  A block of M, S1 and S2 is 3 x 2 column tiles x KT cluster
// tiles, ceil(6 KT / 4) per wavefront, held twice (the sums of the present tile of 64 rows and the
// chunk's running sums): 12 accumulators of 4 doubles, 96 registers, at K = 64.  Three statistics
// at the 64 columns of the unmasked pass would be 192 registers beside the 16 of the logits.  With
// D <= 32 there is one block: its y tile stays in LDS between the products and the running sums
// live in registers through the chunk.  Above, the logits walk the blocks first, the second
// product walks them again and each block's running sums are carried through the chunk's partial.
//
// The y tile of a block is 64 rows of 32 doubles, one bank row of the LDS each.  ds_read_b64 is
// served per half of 32 lanes and the bank pair of a double is its index modulo 32, so a half must
// read 32 different columns-after-swizzle.  Element (t, j) stands at column j ^ f(t) of row t,
//     f(t) = ((t & 15) << 1) ^ ((t & 1) << 4):
//   * first product: lane (l15, l4) reads row 16 w + l15, column 4 s + l4; a half holds two values
//     of l4 that differ in bit 0, and bits 1 .. 4 of f are an invertible function of l15
//     (b0, b1, b2, b3 ^ b0), so the 32 lanes read 32 different bank pairs;
//   * second product: lane (l15, l4) reads row 4 s + l4, column 16 ct + l15; a half holds rows t and
//     t + 1 of one parity pair, f differs between them in bit 4 (and bit 1), and l15 fills bits
//     0 .. 3, so the two rows' sixteen columns fall on different halves of the bank row.
// f is below 32 and stays inside the row; it is the function vmp_dgmm.hip uses for rows of 64.
//
// No floating-point atomics: a workgroup owns a chunk of consecutive rows and leaves one partial;
// dgmm_masked_combine_kernel adds the partials in chunk order.
#include "vmp_common.h"
#include "vmp_dgmm_masked_dev.h"

namespace {

constexpr int NT = VMP_DGMM_NT;
constexpr int DBM = VMP_DGMM_MASKED_DBLOCK;

struct MaskedArgs {
    int64_t N, chunk;
    int D, K;
    const double *y;           // N x D, packed
    const int32_t *labels;     // fixed classes (r = one-hot, lse = 0) or null
    const double *h, *q, *g;   // D x K
    const double *c;           // K
    double *part;              // chunks x vmp_dgmm_masked_partial_doubles
    double *r_out;             // N x K or null
};

__device__ __forceinline__ int y_at(int t, int j)
{
    return t * DBM + (j ^ (((t & 15) << 1) ^ ((t & 1) << 4)));
}

// one thread per element; the observed entries are counted in integers
__global__ void __launch_bounds__(NT)
dgmm_pack_masked_kernel(int64_t n, const double *__restrict__ y, const uint8_t *__restrict__ mask,
                        double *__restrict__ out, unsigned long long *__restrict__ count)
{
    __shared__ int cs[NT];
    const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
    int ob = 0;
    if (i < n) {
        ob = mask[i] != 0;
        out[i] = vmp_dgmm_pack_value(y[i], ob);
    }
    cs[threadIdx.x] = ob;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) cs[threadIdx.x] += cs[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0 && cs[0]) atomicAdd(count, (unsigned long long)cs[0]);
}

template <int KT>
__global__ void __launch_bounds__(NT) dgmm_masked_pass_kernel(MaskedArgs a)
{
    constexpr int KP = KT * 16;
    constexpr int NH = (6 * KT + 3) / 4;             // (statistic, k, d) tiles of a block per wavefront
    __shared__ double y_s[VMP_DGMM_TILE * DBM];      // the y tile of a block; the slots at the end
    __shared__ double r_s[VMP_DGMM_TILE * KP];       // responsibilities of the tile, row-major
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, l15 = l & 15, l4 = l >> 4;
    const int D = a.D, K = a.K;
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t r1 = (r0 + a.chunk < a.N) ? r0 + a.chunk : a.N;
    double *part = a.part + (int64_t)blockIdx.x * vmp_dgmm_masked_partial_doubles(D, K);
    const int64_t DK = (int64_t)D * K;
    const int nblk = (D + DBM - 1) / DBM;
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

    // rows row0 .. of columns d0 .. d0 + 31 into y_s; hidden beyond the chunk and beyond D
    auto load_y = [&](int64_t row0, int d0) {
        for (int i = tid; i < VMP_DGMM_TILE * DBM; i += NT) {
            const int t = i / DBM, j = i % DBM;
            const int64_t row = row0 + t;
            const int d = d0 + j;
            y_s[y_at(t, j)] = (row < r1 && d < D) ? a.y[row * D + d] : vmp_dgmm_hidden();
        }
    };

    for (int64_t row0 = r0; row0 < r1; row0 += VMP_DGMM_TILE) {
        // -- logits of this wavefront's 16 rows, block after block; `seen` counts the observed
        // entries this lane met in its row (16 wave + l15)
        v4f64 lg[KT];
#pragma unroll
        for (int kb = 0; kb < KT; ++kb) lg[kb] = v4f64{0.0, 0.0, 0.0, 0.0};
        int seen = 0;
        for (int blk = 0; blk < nblk; ++blk) {
            const int d0 = blk * DBM;
            if (blk > 0) __syncthreads();            // the block before has been read
            load_y(row0, d0);
            __syncthreads();
            const int cols = (D - d0 < DBM) ? D - d0 : DBM;
            const int steps = (cols + 3) >> 2;
            for (int s = 0; s < steps; ++s) {
                const int j = 4 * s + l4, d = d0 + j;
                const double v = y_s[y_at(wave * 16 + l15, j)];
                seen += vmp_dgmm_observed(v) ? 1 : 0;
                if (!soft) continue;
                const double am = vmp_dgmm_mask_value(v), av = vmp_dgmm_masked_value(v);
                const double av2 = vmp_dgmm_square(av);
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) {
                    const int k = kb * 16 + l15;
                    const bool in = d < D && k < K;
                    const double bg = in ? a.g[(int64_t)d * K + k] : 0.0;
                    const double bh = in ? a.h[(int64_t)d * K + k] : 0.0;
                    const double bq = in ? a.q[(int64_t)d * K + k] : 0.0;
                    lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, bg, lg[kb], 0, 0, 0);
                    lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bh, lg[kb], 0, 0, 0);
                    lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av2, bq, lg[kb], 0, 0, 0);
                }
            }
        }
        // the four lanes of a row (l15, l15 + 16, + 32, + 48) add their counts
        seen += __shfl_xor(seen, 16);
        seen += __shfl_xor(seen, 32);
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
            const bool obs = __shfl(seen, l4 + 4 * qq) > 0;      // lane l15 = l4 + 4 qq has the row
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
                if (obs) nk[kb] += rv;
                if (a.r_out && valid && k < K) a.r_out[row * K + k] = rv;
            }
            if (valid && obs) lsum += lse;
        }
        __syncthreads();

        // -- (S1, S2, M) += r^T (Yt, Yt o Yt, M), block after block.  Tile tl of a block is
        // (column tile ct, statistic st, cluster tile kb) = (tl / (3 KT), (tl / KT) % 3, tl % KT),
        // dealt out to the wavefronts; the sums of the tile of rows start at zero and are added to
        // the chunk's running sums once per tile (vmp_dgmm_masked_dev.h).
        for (int blk = 0; blk < nblk; ++blk) {
            const int d0 = blk * DBM;
            if (nblk > 1) {
                __syncthreads();                     // what y_s held has been read
                load_y(row0, d0);
                __syncthreads();
            }
            const int cols = (D - d0 < DBM) ? D - d0 : DBM;
            const int ntile = 3 * KT * ((cols + 15) >> 4);
            v4f64 tacc[NH];
#pragma unroll
            for (int j = 0; j < NH; ++j) tacc[j] = v4f64{0.0, 0.0, 0.0, 0.0};
            if (nblk > 1) {
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int tl = wave + 4 * j;
                    if (tl >= ntile) continue;
                    const int kb = tl % KT, st = (tl / KT) % 3, d = d0 + (tl / (3 * KT)) * 16 + l15;
                    const int64_t po = st * DK;
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
                    const int kb = tl % KT, st = (tl / KT) % 3, jc = (tl / (3 * KT)) * 16 + l15;
                    const double av = rrow[kb * 16 + l15];
                    const double yv = y_s[y_at(t, jc)];
                    const double yt = vmp_dgmm_masked_value(yv);
                    const double bv = st == 0 ? yt : st == 1 ? vmp_dgmm_square(yt)
                                                             : vmp_dgmm_mask_value(yv);
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
                    const int kb = tl % KT, st = (tl / KT) % 3, d = d0 + (tl / (3 * KT)) * 16 + l15;
                    const int64_t po = st * DK;
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
        part[3 * DK + tid] = t;
    }
    if (tid == 0) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += lse_s[s];
        part[3 * DK + K] = t;
    }
}

// one thread per (k, d): the partials in chunk order
__global__ void __launch_bounds__(NT)
dgmm_masked_combine_kernel(int64_t nc, int D, int K, const double *__restrict__ part,
                           double *__restrict__ S1, double *__restrict__ S2,
                           double *__restrict__ M, double *__restrict__ Nk,
                           double *__restrict__ sum_lse)
{
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx >= D * K) return;
    const int k = idx / D, d = idx - k * D;
    const int64_t per = vmp_dgmm_masked_partial_doubles(D, K), DK = (int64_t)D * K;
    double s1 = 0.0, s2 = 0.0, m = 0.0;
    for (int64_t c = 0; c < nc; ++c) {
        s1 += part[c * per + idx];
        s2 += part[c * per + DK + idx];
        m += part[c * per + 2 * DK + idx];
    }
    const int64_t e = (int64_t)d * K + k;
    S1[e] = s1;
    S2[e] = s2;
    M[e] = m;
    if (d == 0) {
        double n = 0.0;
        for (int64_t c = 0; c < nc; ++c) n += part[c * per + 3 * DK + k];
        Nk[k] = n;
    }
    if (idx == 0) {
        double t = 0.0;
        for (int64_t c = 0; c < nc; ++c) t += part[c * per + 3 * DK + K];
        sum_lse[0] = t;
    }
}

// scal[2]: S1 . h + S2 . q + M . g from the three dot products
__global__ void dgmm_masked_add3_kernel(const double *__restrict__ three, double *__restrict__ out)
{
    out[0] = vmp_dgmm_masked_dots(three[0], three[1], three[2]);
}

// h = <tau><mu>, q = -1/2 <tau>, g = 1/2 <log tau> - 1/2 <tau><mu^2>; c = <log pi> less its largest
// element.  mu_mom, tau_mom: (D K, 2) or null (no observation term)
__global__ void __launch_bounds__(NT)
dgmm_masked_tables_kernel(int D, int K, const double *__restrict__ mu_mom,
                          const double *__restrict__ tau_mom, const double *__restrict__ elog_pi,
                          double *__restrict__ h, double *__restrict__ q, double *__restrict__ g,
                          double *__restrict__ c)
{
    const int idx = blockIdx.x * NT + threadIdx.x;
    const bool have = mu_mom && tau_mom;
    if (idx < D * K) {
        const int64_t e = 2 * (int64_t)idx;
        h[idx] = have ? vmp_dgmm_h(tau_mom[e], mu_mom[e]) : 0.0;
        q[idx] = have ? vmp_dgmm_q(tau_mom[e]) : 0.0;
        g[idx] = have ? vmp_dgmm_g(tau_mom[e], tau_mom[e + 1], mu_mom[e + 1]) : 0.0;
    }
    if (blockIdx.x == 0 && idx < K) {
        double m = elog_pi[0];
        for (int k = 1; k < K; ++k) m = fmax(m, elog_pi[k]);
        c[idx] = elog_pi[idx] - m;
    }
}

// dgmm_update_kernel of vmp_dgmm.hip with the count of the element, M[d, k], in the place of N_k
__global__ void __launch_bounds__(NT)
dgmm_masked_update_kernel(int D, int K, int which, const double *__restrict__ prior_a,
                          const double *__restrict__ prior_b, const double *__restrict__ S1,
                          const double *__restrict__ S2, const double *__restrict__ M,
                          const double *__restrict__ other, double *__restrict__ par,
                          double *__restrict__ mom, double *__restrict__ bound)
{
    __shared__ double bs[NT];
    const int tid = threadIdx.x;
    const bool stats = S1 && S2 && M && other;
    double t = 0.0;
    for (int e = tid; e < D * K; e += NT) {
        const double cnt = stats ? M[e] : 0.0, s1 = stats ? S1[e] : 0.0, s2 = stats ? S2[e] : 0.0;
        const double o0 = stats ? other[2 * (int64_t)e] : 0.0;
        const double o1 = stats ? other[2 * (int64_t)e + 1] : 0.0;
        if (which == 0)
            t += vmp_dgmm_update_mu(prior_a[e], prior_b[e], o0, cnt, s1, par + 2 * (int64_t)e,
                                    mom + 2 * (int64_t)e);
        else
            t += vmp_dgmm_masked_update_tau(prior_a[e], prior_b[e], o0, o1, cnt, s1, s2,
                                            par + 2 * (int64_t)e, mom + 2 * (int64_t)e);
    }
    bs[tid] = t;
    __syncthreads();
    block_halve_sum<NT>(bs, tid);
    if (tid == 0) bound[0] = bs[0];
}

template <int KT>
void launch_pass(vmp_ctx *ctx, int64_t nc, const MaskedArgs &a)
{
    hipLaunchKernelGGL((dgmm_masked_pass_kernel<KT>), dim3((unsigned)nc), dim3(NT), 0, ctx->stream,
                       a);
}

}  // namespace

extern "C" {

int32_t vmp_dgmm_limits_masked(int32_t *max_K, int32_t *max_D)
{
    if (!max_K || !max_D) return VMP_ERR_INVALID;
    *max_K = VMP_DGMM_MASKED_MAX_K;
    *max_D = VMP_DGMM_MASKED_MAX_D;
    return VMP_OK;
}

int32_t vmp_dgmm_plan_masked(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                             int64_t *workspace_doubles)
{
    if (N < 0 || D < 1 || K < 1 || !chunk_rows || !workspace_doubles) return VMP_ERR_INVALID;
    if (K > VMP_DGMM_MASKED_MAX_K || D > VMP_DGMM_MASKED_MAX_D) return VMP_ERR_UNSUPPORTED;
    *chunk_rows = vmp_dgmm_masked_chunk_rows(N, D, K);
    // the partials, the partial sums of a dot product, the three dot products of scal[2]
    *workspace_doubles = vmp_dgmm_masked_chunks(N, D, K) * vmp_dgmm_masked_partial_doubles(D, K)
                         + 1024 + 3;
    return VMP_OK;
}

int32_t vmp_dgmm_pack_masked(vmp_ctx *ctx, int64_t N, int32_t D, const double *y,
                             const uint8_t *mask, double *y_packed, int64_t *n_observed)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, D <= VMP_DGMM_MASKED_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d exceeds the limit %d", D, VMP_DGMM_MASKED_MAX_D);
    VMP_REQUIRE(ctx, n_observed && (N == 0 || (y && mask && y_packed)), VMP_ERR_INVALID,
                "null argument");
    VMP_HIP_CHECK(ctx, hipMemsetAsync(n_observed, 0, sizeof(int64_t), ctx->stream));
    if (N == 0) return VMP_OK;
    const int64_t n = N * D;
    hipLaunchKernelGGL(dgmm_pack_masked_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0,
                       ctx->stream, n, y, mask, y_packed, (unsigned long long *)n_observed);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_dgmm_tables_masked(vmp_ctx *ctx, int32_t D, int32_t K, const double *mu_mom,
                               const double *tau_mom, const double *elog_pi, double *h, double *q,
                               double *g, double *c)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_DGMM_MASKED_MAX_K && D <= VMP_DGMM_MASKED_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_DGMM_MASKED_MAX_D,
                VMP_DGMM_MASKED_MAX_K);
    VMP_REQUIRE(ctx, elog_pi && h && q && g && c, VMP_ERR_INVALID, "null argument");
    hipLaunchKernelGGL(dgmm_masked_tables_kernel, dim3((unsigned)((D * K + NT - 1) / NT)), dim3(NT),
                       0, ctx->stream, D, K, mu_mom, tau_mom, elog_pi, h, q, g, c);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_dgmm_pass_masked(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, const double *y_packed,
                             const int32_t *labels, const double *h, const double *q,
                             const double *g, const double *c, double *ws, double *S1, double *S2,
                             double *M, double *Nk, double *scal, double *r_out)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_DGMM_MASKED_MAX_K && D <= VMP_DGMM_MASKED_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_DGMM_MASKED_MAX_D,
                VMP_DGMM_MASKED_MAX_K);
    VMP_REQUIRE(ctx, h && q && g && c && ws && S1 && S2 && M && Nk && scal && (N == 0 || y_packed),
                VMP_ERR_INVALID, "null argument");
    const int64_t nc = vmp_dgmm_masked_chunks(N, D, K);
    if (nc > 0) {
        MaskedArgs a = {N, vmp_dgmm_masked_chunk_rows(N, D, K), D, K, y_packed, labels, h, q, g, c,
                        ws, r_out};
        switch (vmp_dgmm_kpad(K) / 16) {
        case 1: launch_pass<1>(ctx, nc, a); break;
        case 2: launch_pass<2>(ctx, nc, a); break;
        case 3: launch_pass<3>(ctx, nc, a); break;
        default: launch_pass<4>(ctx, nc, a); break;
        }
    }
    hipLaunchKernelGGL(dgmm_masked_combine_kernel, dim3((unsigned)((D * K + NT - 1) / NT)),
                       dim3(NT), 0, ctx->stream, nc, D, K, ws, S1, S2, M, Nk, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    double *dot_ws = ws + nc * vmp_dgmm_masked_partial_doubles(D, K), *three = dot_ws + 1024;
    int32_t rc = vmp_lda_dot(ctx, K, Nk, c, dot_ws, scal + 1);
    if (rc != VMP_OK) return rc;
    rc = vmp_lda_dot(ctx, (int64_t)D * K, S1, h, dot_ws, three);
    if (rc != VMP_OK) return rc;
    rc = vmp_lda_dot(ctx, (int64_t)D * K, S2, q, dot_ws, three + 1);
    if (rc != VMP_OK) return rc;
    rc = vmp_lda_dot(ctx, (int64_t)D * K, M, g, dot_ws, three + 2);
    if (rc != VMP_OK) return rc;
    hipLaunchKernelGGL(dgmm_masked_add3_kernel, dim3(1), dim3(1), 0, ctx->stream, three, scal + 2);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_dgmm_update_masked(vmp_ctx *ctx, int32_t D, int32_t K, int32_t which,
                               const double *prior_a, const double *prior_b, const double *S1,
                               const double *S2, const double *M, const double *other_mom,
                               double *par, double *mom, double *bound)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1 && (which == 0 || which == 1), VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_DGMM_MASKED_MAX_K && D <= VMP_DGMM_MASKED_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_DGMM_MASKED_MAX_D,
                VMP_DGMM_MASKED_MAX_K);
    VMP_REQUIRE(ctx, prior_a && prior_b && par && mom && bound, VMP_ERR_INVALID, "null argument");
    hipLaunchKernelGGL(dgmm_masked_update_kernel, dim3(1), dim3(NT), 0, ctx->stream, D, K, which,
                       prior_a, prior_b, S1, S2, M, other_mom, par, mom, bound);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
