// vmp_mmm.hip -- the pack, the tables and the plate pass of the fused multinomial-mixture block
//
//     R = Dirichlet(a);  Z = Categorical(R, plates=(N,))
//     P = Dirichlet(a0, plates=(K,)) over M words;  X = Mixture(Z, Multinomial, n, P);  X.observe(x)
//
// (the reference forms the (N, K) log-density from an (N, K, M) broadcast and an (N, K, M) message
// to P, mixture.py / multinomial.py / dirichlet.py).  One pass over the rows leaves the sufficient
// statistics only (vmp_mmm_dev.h), with L[m, k] = <log p_km> - <log p_0m>:
//
//   per tile of 64 rows   logit = X L + c
//                         lse, r = exp(logit - lse)                 (r goes to LDS, never to memory)
//                         N_k += sum r, sum lse
//                         S += r^T X                                (K x M, a row per cluster)
//
// Both products run on v_mfma_f64_16x16x4_f64 (operand layout: vmp_dgmm.hip).  x is 16 bits per
// entry (the fragment loads, the softmax and the compensated sums are those of vmp_pmm_dev.h); the
// tile of a word block is staged in LDS as it is and becomes a double when an operand is formed.
// The pass reads no other array of size N M.
//
// M is walked in WORD BLOCKS of 128: 32 accumulator tiles of 16 x 16 at K = 64, eight per
// wavefront, held twice (the sums of the present tile of 64 rows and the chunk's running sums): 128
// registers.  With one block its x tile stays in LDS between the two products and the running sums
// live in registers through the chunk.  Above, the logits walk the blocks first, the second product
// walks them again (from L2) and each block's running sums are carried through the chunk's partial
// in memory; that holds M = 1024.
//
// A row of the staged tile is 128 + 2 halfwords: 65 dwords, so the 16 rows of an A read and the 4
// rows of a B read fall on different banks.
//
// No floating-point atomics: a workgroup owns a chunk of consecutive rows and leaves one partial;
// mmm_combine_kernel adds the partials in chunk order.
#include "vmp_common.h"
#include "vmp_mmm_dev.h"

namespace {

constexpr int NT = VMP_MMM_NT;

struct MmmArgs {
    int64_t N, chunk;
    int M, K;
    const uint16_t *x;         // N x M, packed
    const int32_t *labels;     // fixed classes (r = one-hot, lse = 0) or null
    const double *L;           // M x K, word-major
    const double *c;           // K
    double *part;              // chunks x vmp_mmm_partial_doubles
    double *r_out;             // N x K or null
};

__device__ __forceinline__ double group16_max(double v)
{
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 16));
    return v;
}

__device__ __forceinline__ double group16_sum(double v)
{
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
    return v;
}

template <int KT>
__global__ void __launch_bounds__(NT) mmm_pass_kernel(MmmArgs a)
{
    constexpr int KP = KT * 16;
    constexpr int MB = VMP_MMM_MBLOCK;
    constexpr int STR = MB + 2;                      // halfwords of a staged row
    constexpr int NH = KT * (MB / 16) / 4;           // (word, k) tiles per wavefront
    __shared__ __attribute__((aligned(8))) uint16_t x_s[VMP_MMM_TILE * STR];
    __shared__ double r_s[VMP_MMM_TILE * KP];        // responsibilities of the tile, row-major
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int M = a.M, K = a.K;
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t r1 = (r0 + a.chunk < a.N) ? r0 + a.chunk : a.N;
    double *part = a.part + (int64_t)blockIdx.x * vmp_mmm_partial_doubles(M, K);
    const int64_t MK = (int64_t)M * K;
    const int nblk = (M + MB - 1) / MB;
    const bool soft = a.labels == nullptr;
    const bool x8 = ((uintptr_t)a.x & 7) == 0;

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

    // rows row0 .. of words m0 .. m0 + MB - 1 into x_s, four halfwords per thread and step; zero
    // beyond the chunk and beyond M
    auto load_x = [&](int64_t row0, int m0) {
        for (int i = tid; i < VMP_MMM_TILE * (MB / 4); i += NT) {
            const int t = i / (MB / 4), j = 4 * (i % (MB / 4));
            const int64_t row = row0 + t;
            const int m = m0 + j;
            const int64_t e = row * M + m;
            uint32_t lo, hi;
            if (row < r1 && m + 3 < M && x8 && (e & 3) == 0) {
                const uint64_t v = *(const uint64_t *)(a.x + e);
                lo = (uint32_t)v;
                hi = (uint32_t)(v >> 32);
            } else {
                uint32_t h[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) h[b] = (row < r1 && m + b < M) ? a.x[e + b] : 0u;
                lo = h[0] | (h[1] << 16);
                hi = h[2] | (h[3] << 16);
            }
            uint32_t *dst = (uint32_t *)(x_s + t * STR + j);
            dst[0] = lo;
            dst[1] = hi;
        }
    };

    for (int64_t row0 = r0; row0 < r1; row0 += VMP_MMM_TILE) {
        // -- logits of this wavefront's 16 rows, block after block
        v4f64 lg[KT];
#pragma unroll
        for (int kb = 0; kb < KT; ++kb) lg[kb] = v4f64{0.0, 0.0, 0.0, 0.0};
        if (soft || nblk == 1) {
            for (int blk = 0; blk < nblk; ++blk) {
                const int m0 = blk * MB;
                if (blk > 0) __syncthreads();        // the block before has been read
                load_x(row0, m0);
                __syncthreads();
                if (!soft) continue;
                const int cols = (M - m0 < MB) ? M - m0 : MB;
                const int steps = (cols + 3) >> 2;
                for (int s = 0; s < steps; ++s) {
                    const int j = 4 * s + l4, m = m0 + j;
                    const double av = vmp_pmm_count(x_s[(wave * 16 + l15) * STR + j]);
#pragma unroll
                    for (int kb = 0; kb < KT; ++kb) {
                        const int k = kb * 16 + l15;
                        const double bl = (m < M && k < K) ? a.L[(int64_t)m * K + k] : 0.0;
                        lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bl, lg[kb], 0, 0, 0);
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
            double lse = 0.0, s = 1.0, ex[KT];
            int lab = -1;
            if (soft) {
                double mx = lg[0][qq];
#pragma unroll
                for (int kb = 1; kb < KT; ++kb) mx = fmax(mx, lg[kb][qq]);
                mx = group16_max(mx);
                s = 0.0;
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) {
                    ex[kb] = vmp_dgmm_shifted_exp(lg[kb][qq], mx);
                    s += ex[kb];
                }
                s = group16_sum(s);
                lse = vmp_dgmm_lse(mx, s);
            } else if (valid) {
                lab = a.labels[row];
            }
#pragma unroll
            for (int kb = 0; kb < KT; ++kb) {
                const int k = kb * 16 + l15;
                double rv = 0.0;
                if (valid) rv = soft ? vmp_pmm_resp(ex[kb], s) : (k == lab ? 1.0 : 0.0);
                r_s[t * KP + k] = rv;
                nk[kb] += rv;
                if (a.r_out && valid && k < K) a.r_out[row * K + k] = rv;
            }
            if (valid) lsum += lse;
        }
        __syncthreads();

        // -- S += r^T X, block after block.  Tile tl of a block is (word tile, cluster tile) =
        // (tl / KT, tl % KT), dealt out to the wavefronts; the sums of the tile of rows start at
        // zero and are added to the chunk's running sums once per tile (vmp_mmm_dev.h).
        for (int blk = 0; blk < nblk; ++blk) {
            const int m0 = blk * MB;
            if (nblk > 1) {
                __syncthreads();                     // what x_s held has been read
                load_x(row0, m0);
                __syncthreads();
            }
            const int cols = (M - m0 < MB) ? M - m0 : MB;
            const int ntile = KT * ((cols + 15) >> 4);
            v4f64 tacc[NH];
#pragma unroll
            for (int j = 0; j < NH; ++j) tacc[j] = v4f64{0.0, 0.0, 0.0, 0.0};
            if (nblk > 1) {
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int tl = wave + 4 * j;
                    if (tl >= ntile) continue;
                    const int kb = tl % KT;
                    const int m = m0 + (tl / KT) * 16 + l15;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int k = kb * 16 + l4 + 4 * qq;
                        acc[j][qq] = (row0 > r0 && k < K && m < M) ? part[(int64_t)k * M + m] : 0.0;
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
                    const int kb = tl % KT;
                    const int jc = (tl / KT) * 16 + l15;
                    const double av = rrow[kb * 16 + l15];
                    const double bv = vmp_pmm_count(x_s[t * STR + jc]);
                    tacc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, tacc[j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int j = 0; j < NH; ++j)
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) acc[j][qq] += tacc[j][qq];
            if (nblk > 1 || row0 + VMP_MMM_TILE >= r1) {
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int tl = wave + 4 * j;
                    if (tl >= ntile) continue;
                    const int kb = tl % KT;
                    const int m = m0 + (tl / KT) * 16 + l15;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int k = kb * 16 + l4 + 4 * qq;
                        if (k < K && m < M) part[(int64_t)k * M + m] = acc[j][qq];
                    }
                }
            }
        }
        __syncthreads();                 // r_s and x_s are free for the next tile
    }

    // -- N_k and sum lse: the 16 slots in slot order (they stand in r_s, which is free now) ------
    double *nk_s = r_s, *lse_s = r_s + 16 * KP;
#pragma unroll
    for (int kb = 0; kb < KT; ++kb) nk_s[(wave * 4 + l4) * KP + kb * 16 + l15] = nk[kb];
    if (l15 == 0) lse_s[wave * 4 + l4] = lsum;
    __syncthreads();
    if (tid < K) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += nk_s[s * KP + tid];
        part[MK + tid] = t;
    }
    if (tid == 0) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += lse_s[s];
        part[MK + K] = t;
    }
}

// one thread per (k, m): the partials in chunk order
__global__ void __launch_bounds__(NT)
mmm_combine_kernel(int64_t nc, int M, int K, const double *__restrict__ part,
                   double *__restrict__ S, double *__restrict__ Nk, double *__restrict__ sum_lse)
{
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx >= M * K) return;
    const int64_t per = vmp_mmm_partial_doubles(M, K), MK = (int64_t)M * K;
    double s = 0.0;
    for (int64_t c = 0; c < nc; ++c) s += part[c * per + idx];
    S[idx] = s;
    if (idx < K) {
        double n = 0.0;
        for (int64_t c = 0; c < nc; ++c) n += part[c * per + MK + idx];
        Nk[idx] = n;
    }
    if (idx == 0) {
        double t = 0.0;
        for (int64_t c = 0; c < nc; ++c) t += part[c * per + MK + K];
        sum_lse[0] = t;
    }
}

// one workgroup: scal[1] = N_k . c in ascending k; scal[2] = S . L with S (K x M) and L (M x K):
// element e = k M + m belongs to thread e % 256, the 256 sums are halved eight times
__global__ void __launch_bounds__(NT)
mmm_dots_kernel(int M, int K, const double *__restrict__ S, const double *__restrict__ L,
                const double *__restrict__ Nk, const double *__restrict__ c,
                double *__restrict__ scal)
{
    __shared__ double ds[NT];
    const int tid = threadIdx.x;
    double t = 0.0;
    for (int e = tid; e < M * K; e += NT) {
        const int k = e / M, m = e - k * M;
        t = vmp_pmm_mac(t, S[e], L[(int64_t)m * K + k]);
    }
    ds[tid] = t;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (tid < off) ds[tid] += ds[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        double n = 0.0;
        for (int k = 0; k < K; ++k) n = vmp_pmm_mac(n, Nk[k], c[k]);
        scal[1] = n;
        scal[2] = ds[0];
    }
}

// L[m, k] = <log p_km> - <log p_0m> from elog_p (K x M), zeros without it; c = <log pi> less its
// largest element
__global__ void __launch_bounds__(NT)
mmm_tables_kernel(int M, int K, const double *__restrict__ elog_p,
                  const double *__restrict__ elog_pi, double *__restrict__ L,
                  double *__restrict__ c)
{
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx < M * K) {
        const int m = idx / K, k = idx - m * K;
        L[idx] = elog_p ? vmp_mmm_table(elog_p[(int64_t)k * M + m], elog_p[m]) : 0.0;
    }
    if (blockIdx.x == 0 && idx < K) {
        double mx = elog_pi[0];
        for (int k = 1; k < K; ++k) mx = fmax(mx, elog_pi[k]);
        c[idx] = elog_pi[idx] - mx;
    }
}

__device__ __forceinline__ uint16_t mmm_pack_value(double v, int *bad)
{
    return vmp_mmm_entry(vmp_pmm_pack_f64(v, true, bad));
}
__device__ __forceinline__ uint16_t mmm_pack_value(int64_t v, int *bad)
{
    return vmp_mmm_entry(vmp_pmm_pack_i64(v, true, bad));
}
__device__ __forceinline__ uint16_t mmm_pack_value(int32_t v, int *bad)
{
    return vmp_mmm_entry(vmp_pmm_pack_i64((int64_t)v, true, bad));
}
__device__ __forceinline__ uint16_t mmm_pack_value(uint8_t v, int *bad)
{
    return vmp_mmm_entry(vmp_pmm_pack_i64((int64_t)v, true, bad));
}

// block b: the rows [b span, (b + 1) span); its sum of the multinomial coefficients goes to
// lg_part[b]
template <typename T>
__global__ void __launch_bounds__(NT)
mmm_pack_kernel(int64_t N, int M, int64_t span, const T *__restrict__ x,
                const int64_t *__restrict__ trials, uint16_t *__restrict__ xp, int32_t *flags,
                double *__restrict__ lg_part)
{
    __shared__ double ls[NT];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * span;
    double lg = 0.0, lge = 0.0;
    int bad = 0;
    for (int64_t i = tid; i < span; i += NT) {
        const int64_t row = row0 + i;
        if (row >= N) break;
        const int64_t n = trials[row];
        int bad_row = 0;
        int64_t sum = 0;
        vmp_pmm_sum_add(&lg, &lge, vmp_mmm_lgamma1_trials(n));
        for (int m = 0; m < M; ++m) {
            const uint16_t p = mmm_pack_value(x[row * M + m], &bad_row);
            xp[row * M + m] = p;
            sum += p;
            vmp_pmm_sum_add(&lg, &lge, -vmp_pmm_lgamma1(p));
        }
        if (vmp_mmm_sum_mismatch(sum, n, bad_row)) bad_row |= VMP_MMM_BAD_SUM;
        bad |= bad_row;
    }
    if (bad & VMP_PMM_BAD_INVALID) flags[0] = 1;
    if (bad & VMP_PMM_BAD_ABOVE) flags[1] = 1;
    if (bad & VMP_PMM_BAD_FRACTION) flags[2] = 1;
    if (bad & VMP_MMM_BAD_SUM) flags[3] = 1;
    ls[tid] = lg + lge;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (tid < off) ls[tid] += ls[tid + off];
        __syncthreads();
    }
    if (tid == 0) lg_part[blockIdx.x] = ls[0];
}

// the blocks' partials in block order
__global__ void mmm_pack_finish_kernel(int64_t nb, const double *__restrict__ lg_part,
                                       double *__restrict__ lcoef)
{
    double t = 0.0, te = 0.0;
    for (int64_t b = 0; b < nb; ++b) vmp_pmm_sum_add(&t, &te, lg_part[b]);
    lcoef[0] = t + te;
}

template <typename T>
void launch_pack(vmp_ctx *ctx, int64_t N, int M, const void *x, const int64_t *trials,
                 uint16_t *xp, int32_t *flags, double *ws)
{
    hipLaunchKernelGGL(mmm_pack_kernel<T>, dim3((unsigned)vmp_pmm_pack_blocks(N)), dim3(NT), 0,
                       ctx->stream, N, M, vmp_pmm_pack_span(N), (const T *)x, trials, xp, flags,
                       ws);
}

}  // namespace

#define MMM_SHAPE(ctx, M, K)                                                                      \
    VMP_REQUIRE(ctx, K <= VMP_MMM_MAX_K && M <= VMP_MMM_MAX_M, VMP_ERR_UNSUPPORTED,               \
                "M = %d, K = %d exceed the limits (%d, %d)", M, K, VMP_MMM_MAX_M, VMP_MMM_MAX_K)

extern "C" {

int32_t vmp_mmm_limits(int32_t *max_K, int32_t *max_M, int32_t *max_count)
{
    if (!max_K || !max_M || !max_count) return VMP_ERR_INVALID;
    *max_K = VMP_MMM_MAX_K;
    *max_M = VMP_MMM_MAX_M;
    *max_count = VMP_MMM_MAX_COUNT;
    return VMP_OK;
}

int32_t vmp_mmm_plan(int64_t N, int32_t M, int32_t K, int64_t *chunk_rows,
                     int64_t *workspace_doubles)
{
    if (N < 0 || M < 1 || K < 1) return VMP_ERR_INVALID;
    if (K > VMP_MMM_MAX_K || M > VMP_MMM_MAX_M) return VMP_ERR_UNSUPPORTED;
    if (!chunk_rows || !workspace_doubles) return VMP_ERR_INVALID;
    *chunk_rows = vmp_mmm_chunk_rows(N, M, K);
    *workspace_doubles = vmp_mmm_workspace_doubles(N, M, K);
    return VMP_OK;
}

int32_t vmp_mmm_pack(vmp_ctx *ctx, int64_t N, int32_t M, int32_t dtype, const void *x,
                     const int64_t *trials, uint16_t *x_packed, int32_t *flags, double *lcoef,
                     double *ws)
{
    VMP_REQUIRE(ctx, ctx && N >= 0 && M >= 1 && dtype >= 0 && dtype <= 3, VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, M <= VMP_MMM_MAX_M, VMP_ERR_UNSUPPORTED, "M = %d exceeds the limit %d", M,
                VMP_MMM_MAX_M);
    VMP_REQUIRE(ctx, flags && lcoef && ws && (N == 0 || (x && trials && x_packed)),
                VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    if (N > 0) {
        switch (dtype) {
        case 0: launch_pack<double>(ctx, N, M, x, trials, x_packed, flags, ws); break;
        case 1: launch_pack<int64_t>(ctx, N, M, x, trials, x_packed, flags, ws); break;
        case 2: launch_pack<uint8_t>(ctx, N, M, x, trials, x_packed, flags, ws); break;
        default: launch_pack<int32_t>(ctx, N, M, x, trials, x_packed, flags, ws); break;
        }
        VMP_HIP_CHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(mmm_pack_finish_kernel, dim3(1), dim3(1), 0, ctx->stream,
                       N > 0 ? vmp_pmm_pack_blocks(N) : 0, ws, lcoef);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_mmm_tables(vmp_ctx *ctx, int32_t M, int32_t K, const double *elog_p,
                       const double *elog_pi, double *L, double *c)
{
    VMP_REQUIRE(ctx, ctx && M >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    MMM_SHAPE(ctx, M, K);
    VMP_REQUIRE(ctx, elog_pi && L && c, VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    hipLaunchKernelGGL(mmm_tables_kernel, dim3((unsigned)((M * K + NT - 1) / NT)), dim3(NT), 0,
                       ctx->stream, M, K, elog_p, elog_pi, L, c);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_mmm_pass(vmp_ctx *ctx, int64_t N, int32_t M, int32_t K, const uint16_t *x_packed,
                     const int32_t *labels, const double *L, const double *c, double *ws,
                     double *S, double *Nk, double *scal, double *r_out)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, ctx && N >= 0 && M >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    MMM_SHAPE(ctx, M, K);
    VMP_REQUIRE(ctx, L && c && ws && S && Nk && scal && (N == 0 || x_packed), VMP_ERR_INVALID,
                "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int64_t nc = vmp_mmm_chunks(N, M, K);
    if (nc > 0) {
        MmmArgs a = {N, vmp_mmm_chunk_rows(N, M, K), M, K, x_packed, labels, L, c, ws, r_out};
        switch (vmp_pmm_kpad(K) / 16) {
        case 1:
            hipLaunchKernelGGL(mmm_pass_kernel<1>, dim3((unsigned)nc), dim3(NT), 0, ctx->stream, a);
            break;
        case 2:
            hipLaunchKernelGGL(mmm_pass_kernel<2>, dim3((unsigned)nc), dim3(NT), 0, ctx->stream, a);
            break;
        case 3:
            hipLaunchKernelGGL(mmm_pass_kernel<3>, dim3((unsigned)nc), dim3(NT), 0, ctx->stream, a);
            break;
        default:
            hipLaunchKernelGGL(mmm_pass_kernel<4>, dim3((unsigned)nc), dim3(NT), 0, ctx->stream, a);
            break;
        }
        VMP_HIP_CHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(mmm_combine_kernel, dim3((unsigned)((M * K + NT - 1) / NT)), dim3(NT), 0,
                       ctx->stream, nc, M, K, ws, S, Nk, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(mmm_dots_kernel, dim3(1), dim3(NT), 0, ctx->stream, M, K, S, L, Nk, c, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
