// vmp_chain_tv.hip -- plate sums of the messages of a Gaussian Markov chain to time-varying
// dynamics A_t / innovation precisions nu_t that many sequences share (reference formulas:
// gaussian_markov_chain.py:462-527).  From the smoothed means x (ny, N, D), row-major:
//   Sxx[t] = sum_b x_{b,t} x_{b,t}^T   (N, D, D)      Sxp[t] = sum_b x_{b,t} x_{b,t+1}^T   (N-1, D, D)
// (the caller adds ny V_t and ny C_t, which the solver returns once when the dynamics carry no
// sequence plate).  x is the only plate-sized array touched.
//
// Stage 1, grid (time tiles, slices of the sequences): a workgroup stages the (TT + 1) D
// contiguous doubles of its tile -- its TT = 256 / D time instances plus one instance of halo for
// the cross term -- of BB = 8 sequences in LDS with coalesced loads, then lane (t, i) adds
// x_{t,i} x_{t,j} and x_{t,i} x_{t+1,j}, j < D, to its 2 D accumulators (32 doubles at D = 16).
// Every element of x is read from memory once, plus 1 / TT for the halo.  A lane's row of partials
// goes to the slice's block of the workspace.  Stage 2 adds the slices' partials in slice order.
// No atomics; the order of every sum is fixed by (ny, N, D) (vmp_chain_tv_dev.h).
#include "vmp_common.h"
#include "vmp_chain_tv_dev.h"

namespace {

constexpr int NT = VMP_CHAIN_TV_NT;
constexpr int BB = VMP_CHAIN_TV_BB;

template <int D>
__global__ void __launch_bounds__(NT)
chain_pair_partials_kernel(int64_t ny, int N, int64_t per, const double *__restrict__ x,
                           double *__restrict__ work)
{
    constexpr int TT = NT / D;
    constexpr int ROW = (TT + 1) * D;
    __shared__ double s[BB][ROW];
    const int tid = threadIdx.x;
    const int t0 = (int)blockIdx.x * TT;
    const int64_t slice = blockIdx.y;
    const int nt = min(TT, N - t0);                       // time instances of this tile (>= 1)
    const int nload = min(TT + 1, N - t0) * D;            // with the halo, if there is a t + 1
    const int64_t b0 = slice * per;
    const int64_t b1 = min(ny, b0 + per);
    const int tl = tid / D, i = tid - tl * D;
    const bool active = tid < nt * D;
    const int64_t row = (int64_t)N * D;

    double axx[D], axp[D];
#pragma unroll
    for (int j = 0; j < D; ++j) axx[j] = axp[j] = 0.0;

    // the halo of the last tile does not exist: zeros there (their products are never stored)
    for (int r = 0; r < BB; ++r)
        for (int e = nload + tid; e < ROW; e += NT) s[r][e] = 0.0;

    for (int64_t bb = b0; bb < b1; bb += BB) {
        const int nb = (int)min((int64_t)BB, b1 - bb);
        for (int r = 0; r < nb; ++r) {
            const double *src = x + (bb + r) * row + (int64_t)t0 * D;
            for (int e = tid; e < nload; e += NT) s[r][e] = src[e];
        }
        __syncthreads();
        if (active) {
            for (int r = 0; r < nb; ++r) {
                const double xi = s[r][tl * D + i];
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    axx[j] = vmp_chain_tv_step(axx[j], xi, s[r][tl * D + j]);
                    axp[j] = vmp_chain_tv_step(axp[j], xi, s[r][(tl + 1) * D + j]);
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    const int t = t0 + tl;                                // < N
    double *wxx = work + slice * vmp_chain_tv_total(N, D) + ((int64_t)t * D + i) * D;
#pragma unroll
    for (int j = 0; j < D; ++j) wxx[j] = axx[j];
    if (t < N - 1) {
        double *wxp = wxx + (int64_t)N * D * D;
#pragma unroll
        for (int j = 0; j < D; ++j) wxp[j] = axp[j];
    }
}

__global__ void __launch_bounds__(NT)
chain_pair_combine_kernel(int64_t nslice, int64_t nxx, int64_t total,
                          const double *__restrict__ work, double *__restrict__ Sxx,
                          double *__restrict__ Sxp)
{
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= total) return;
    const double v = vmp_chain_tv_combine(work, nslice, total, e);
    if (e < nxx) Sxx[e] = v;
    else Sxp[e - nxx] = v;
}

template <int D>
void launch_partials(vmp_ctx *ctx, int64_t ny, int N, int64_t per, int64_t nslice, const double *x,
                     double *work)
{
    const dim3 grid((unsigned)vmp_chain_tv_ntile(N, D), (unsigned)nslice);
    hipLaunchKernelGGL((chain_pair_partials_kernel<D>), grid, dim3(NT), 0, ctx->stream, ny, N, per,
                       x, work);
}

}  // namespace

extern "C" {

int32_t vmp_chain_pair_stats_limits(int64_t ny, int32_t N, int32_t D, int32_t *max_d,
                                    int32_t *enabled, int64_t *work_doubles)
{
    if (!max_d || !enabled || !work_doubles) return VMP_ERR_INVALID;
    *max_d = VMP_CHAIN_TV_MAX_D;
    *enabled = vmp_tune_get("chain_pair_stats", 1) != 0 ? 1 : 0;
    *work_doubles = 0;
    if (ny < 0 || N < 1 || D < 1) return VMP_ERR_INVALID;
    if (D > VMP_CHAIN_TV_MAX_D) return VMP_ERR_UNSUPPORTED;
    *work_doubles = vmp_chain_tv_work_doubles(ny, N, D);
    return VMP_OK;
}

int32_t vmp_chain_pair_stats(vmp_ctx *ctx, int64_t ny, int32_t N, int32_t D, const double *x,
                             double *Sxx, double *Sxp, double *work, int64_t work_doubles)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && ny >= 0 && N >= 1 && D >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, D <= VMP_CHAIN_TV_MAX_D, VMP_ERR_UNSUPPORTED,
                "vmp_chain_pair_stats: D = %d above the limit %d", D, VMP_CHAIN_TV_MAX_D);
    VMP_REQUIRE(ctx, Sxx && work && (N == 1 || Sxp) && (ny == 0 || x), VMP_ERR_INVALID,
                "null argument");
    const int64_t per = vmp_chain_tv_per(ny, N, D);
    const int64_t nslice = vmp_chain_tv_nslice(ny, N, D);
    const int64_t total = vmp_chain_tv_total(N, D);
    VMP_REQUIRE(ctx, work_doubles >= nslice * total, VMP_ERR_INVALID,
                "vmp_chain_pair_stats: workspace of %lld doubles, %lld needed",
                (long long)work_doubles, (long long)(nslice * total));
    VMP_REQUIRE(ctx, nslice <= 65535 && (total + NT - 1) / NT <= 0x7fffffffLL, VMP_ERR_UNSUPPORTED,
                "vmp_chain_pair_stats: grid too large");
    switch (D) {
#define CASE(d) case d: launch_partials<d>(ctx, ny, N, per, nslice, x, work); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
        CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
        default: return VMP_ERR_UNSUPPORTED;
    }
    VMP_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(chain_pair_combine_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT),
                       0, ctx->stream, nslice, (int64_t)N * D * D, total, work, Sxx, Sxp);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
