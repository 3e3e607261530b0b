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
// THE PASS KERNEL IS THE POISSON BLOCK'S: vmp_mmm_pass launches pmm_pass_kernel<KT, false>
// (vmp_pmm.hip, through vmp_pmm_launch_pass of vmp_common.h) with the M words for its D columns and
// L for its l; nothing is hidden, so its lb is never read.  The 16-bit x, the word blocks of 128
// that hold M = 1024, the staged tile, the softmax and the chunk's partial (S as K x M, N_k, sum
// lse: vmp_mmm_partial_doubles(M, K) = vmp_pmm_partial_doubles(M, K, 0)) are described there.  A
// profile of a multinomial model therefore lists pmm_pass_kernel.
//
// What follows the pass is this block's own and defines the bits of its outputs: mmm_combine_kernel
// adds the partials in chunk order and leaves S as K x M (a row per cluster, where the Poisson
// block writes D x K); mmm_dots_kernel forms scal[1] and scal[2] in the order of vmp_mmm_dev.h.
#include "vmp_common.h"
#include "vmp_mmm_dev.h"

namespace {

constexpr int NT = VMP_MMM_NT;

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
    block_halve_sum<NT>(ds, tid);
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

template <typename T>
__device__ __forceinline__ uint16_t mmm_pack_value(T v, int *bad)
{
    return vmp_mmm_entry(vmp_pmm_pack(v, true, bad));
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
    block_halve_sum<NT>(ls, tid);
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
        // the Poisson pass, nothing hidden: words for columns, L for l; lb is not read
        PmmArgs a = {N, vmp_mmm_chunk_rows(N, M, K), M, K, x_packed, labels, L, L, c, ws, r_out};
        vmp_pmm_launch_pass(ctx, nc, false, a);
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
