// vmp_chain_in.hip -- plate sums of the input cross terms in the messages of a driven Gaussian
// Markov chain, x_t+1 = A x_t + B u_t + noise, to [A | B] and nu when ny sequences share them
// (reference formulas: gaussian_markov_chain.py:485-498).  From the smoothed means x (ny, N, D) and
// the means of the inputs z (zrows, N-1, K), row-major, with t = 0 .. N-2 the transitions:
//   Snz[t] = sum_b x_{b,t+1} z_{b,t}^T  (N-1, D, K)      Spz[t] = sum_b x_{b,t} z_{b,t}^T  (N-1, D, K)
//   Szz[t] = sum_b z_{b,t} z_{b,t}^T    (N-1, K, K), when the caller asks for it
// x and z are the only plate-sized arrays touched, and they are read once.
//
// Stage 1, grid (time tiles, slices of the sequences): a workgroup stages, of BB = 8 sequences at a
// time, the (TT + 1) D contiguous doubles of x of its tile -- TT = 256 / max(D, K) transitions plus
// one time instance of halo for x_{t+1} -- and the TT K doubles of z in LDS with coalesced loads
// (shared inputs, zrows = 1, are staged once).  Lane (t, i) of the tile adds x_{t+1,i} z_{t,k} and
// x_{t,i} z_{t,k} (i < D) and z_{t,i} z_{t,k} (i < K), k < K, to its 3 K accumulators.  A lane's
// rows of partials go to the slice's block of the workspace.  Stage 2 adds the slices' partials in
// slice order.  No atomics; the order of every sum is fixed by (ny, N, D, K) (vmp_chain_in_dev.h).
#include "vmp_common.h"
#include "vmp_chain_in_dev.h"

namespace {

constexpr int NT = VMP_CHAIN_IN_NT;
constexpr int BB = VMP_CHAIN_IN_BB;
constexpr int XROW = NT + VMP_CHAIN_IN_MAX_D;     // (TT + 1) D <= 256 + D
constexpr int ZROW = NT;                          // TT K <= 256

template <int K>
__global__ void __launch_bounds__(NT)
chain_input_partials_kernel(int64_t ny, int zshared, int N, int D, int64_t per, int want_zz,
                            const double *__restrict__ x, const double *__restrict__ z,
                            double *__restrict__ work)
{
    __shared__ double sx[BB][XROW];
    __shared__ double sz[BB][ZROW];
    const int P = vmp_chain_in_lanes(D, K);
    const int TT = NT / P;
    const int tid = threadIdx.x;
    const int t0 = (int)blockIdx.x * TT;
    const int64_t slice = blockIdx.y;
    const int nt = min(TT, (N - 1) - t0);                 // transitions of this tile (>= 1)
    const int nx = (nt + 1) * D;                          // t0 + nt <= N - 1: the halo exists
    const int nz = nt * K;
    const int64_t b0 = slice * per;
    const int64_t b1 = min(ny, b0 + per);
    const int tl = tid / P, i = tid - tl * P;
    const bool active = tl < nt;
    const bool row_x = active && i < D;
    const bool row_z = active && i < K && want_zz;
    const int64_t xrow = (int64_t)N * D;
    const int64_t zrow = (int64_t)(N - 1) * K;

    double anz[K], apz[K], azz[K];
#pragma unroll
    for (int k = 0; k < K; ++k) anz[k] = apz[k] = azz[k] = 0.0;

    if (zshared && b0 < b1) {
        const double *src = z + (int64_t)t0 * K;
        for (int e = tid; e < nz; e += NT) sz[0][e] = src[e];
    }
    for (int64_t bb = b0; bb < b1; bb += BB) {
        const int nb = (int)min((int64_t)BB, b1 - bb);
        for (int r = 0; r < nb; ++r) {
            const double *src = x + (bb + r) * xrow + (int64_t)t0 * D;
            for (int e = tid; e < nx; e += NT) sx[r][e] = src[e];
            if (!zshared) {
                const double *zsrc = z + (bb + r) * zrow + (int64_t)t0 * K;
                for (int e = tid; e < nz; e += NT) sz[r][e] = zsrc[e];
            }
        }
        __syncthreads();
        if (active) {
            for (int r = 0; r < nb; ++r) {
                const double *zr = sz[zshared ? 0 : r] + tl * K;
                if (row_x) {
                    const double xp = sx[r][tl * D + i];
                    const double xn = sx[r][(tl + 1) * D + i];
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        anz[k] = vmp_chain_in_step(anz[k], xn, zr[k]);
                        apz[k] = vmp_chain_in_step(apz[k], xp, zr[k]);
                    }
                }
                if (row_z) {
                    const double zi = zr[i];
#pragma unroll
                    for (int k = 0; k < K; ++k) azz[k] = vmp_chain_in_step(azz[k], zi, zr[k]);
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;
    const int t = t0 + tl;                                // < N - 1
    double *w = work + slice * vmp_chain_in_total(N, D, K);
    const int64_t ncross = vmp_chain_in_cross(N, D, K);
    if (row_x) {
        double *wnz = w + ((int64_t)t * D + i) * K;
        double *wpz = wnz + ncross;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            wnz[k] = anz[k];
            wpz[k] = apz[k];
        }
    }
    if (row_z) {
        double *wzz = w + 2 * ncross + ((int64_t)t * K + i) * K;
#pragma unroll
        for (int k = 0; k < K; ++k) wzz[k] = azz[k];
    }
}

// `used`: the leading doubles of a slice's partials that are combined (all, or the two cross
// blocks when Szz is not asked for)
__global__ void __launch_bounds__(NT)
chain_input_combine_kernel(int64_t nslice, int64_t ncross, int64_t used, int64_t total,
                           const double *__restrict__ work, double *__restrict__ Snz,
                           double *__restrict__ Spz, double *__restrict__ Szz)
{
    const int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (e >= used) return;
    const double v = vmp_chain_in_combine(work, nslice, total, e);
    if (e < ncross) Snz[e] = v;
    else if (e < 2 * ncross) Spz[e - ncross] = v;
    else Szz[e - 2 * ncross] = v;
}

template <int K>
void launch_partials(vmp_ctx *ctx, int64_t ny, int zshared, int N, int D, int64_t per,
                     int64_t nslice, int want_zz, const double *x, const double *z, double *work)
{
    const dim3 grid((unsigned)vmp_chain_in_ntile(N, D, K), (unsigned)nslice);
    hipLaunchKernelGGL((chain_input_partials_kernel<K>), grid, dim3(NT), 0, ctx->stream, ny,
                       zshared, N, D, per, want_zz, x, z, work);
}

}  // namespace

extern "C" {

int32_t vmp_chain_input_stats_limits(int64_t ny, int64_t zrows, int32_t N, int32_t D, int32_t K,
                                     int32_t *max_d, int32_t *max_k, int32_t *enabled,
                                     int64_t *work_doubles)
{
    if (!max_d || !max_k || !enabled || !work_doubles) return VMP_ERR_INVALID;
    *max_d = VMP_CHAIN_IN_MAX_D;
    *max_k = VMP_CHAIN_IN_MAX_K;
    *enabled = vmp_tune_get("chain_input_stats", 1) != 0 ? 1 : 0;
    *work_doubles = 0;
    if (ny < 0 || (zrows != 1 && zrows != ny) || N < 2 || D < 1 || K < 1) return VMP_ERR_INVALID;
    if (D > VMP_CHAIN_IN_MAX_D || K > VMP_CHAIN_IN_MAX_K) return VMP_ERR_UNSUPPORTED;
    *work_doubles = vmp_chain_in_work_doubles(ny, N, D, K);
    return VMP_OK;
}

int32_t vmp_chain_input_stats(vmp_ctx *ctx, int64_t ny, int64_t zrows, int32_t N, int32_t D,
                              int32_t K, const double *x, const double *z, double *Snz,
                              double *Spz, double *Szz, double *work, int64_t work_doubles)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && ny >= 0 && N >= 2 && D >= 1 && K >= 1, VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, zrows == 1 || zrows == ny, VMP_ERR_INVALID,
                "vmp_chain_input_stats: zrows = %lld is neither 1 nor ny = %lld",
                (long long)zrows, (long long)ny);
    VMP_REQUIRE(ctx, D <= VMP_CHAIN_IN_MAX_D && K <= VMP_CHAIN_IN_MAX_K, VMP_ERR_UNSUPPORTED,
                "vmp_chain_input_stats: D = %d, K = %d above the limits %d, %d", D, K,
                VMP_CHAIN_IN_MAX_D, VMP_CHAIN_IN_MAX_K);
    VMP_REQUIRE(ctx, Snz && Spz && work && (ny == 0 || (x && z)), VMP_ERR_INVALID, "null argument");
    const int64_t per = vmp_chain_in_per(ny, N, D, K);
    const int64_t nslice = vmp_chain_in_nslice(ny, N, D, K);
    const int64_t total = vmp_chain_in_total(N, D, K);
    const int64_t ncross = vmp_chain_in_cross(N, D, K);
    const int64_t used = Szz ? total : 2 * ncross;
    VMP_REQUIRE(ctx, work_doubles >= nslice * total, VMP_ERR_INVALID,
                "vmp_chain_input_stats: workspace of %lld doubles, %lld needed",
                (long long)work_doubles, (long long)(nslice * total));
    VMP_REQUIRE(ctx, nslice <= 65535 && vmp_chain_in_ntile(N, D, K) <= 0x7fffffffLL
                    && (used + NT - 1) / NT <= 0x7fffffffLL, VMP_ERR_UNSUPPORTED,
                "vmp_chain_input_stats: grid too large");
    // a sequence's z is shared when there is one row of it for several sequences
    const int zshared = (zrows == 1 && ny != 1) ? 1 : 0;
    switch (K) {
#define CASE(k) case k: launch_partials<k>(ctx, ny, zshared, N, D, per, nslice, Szz ? 1 : 0, x, z, \
                                           work); break;
        CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6) CASE(7) CASE(8)
        CASE(9) CASE(10) CASE(11) CASE(12) CASE(13) CASE(14) CASE(15) CASE(16)
#undef CASE
        default: return VMP_ERR_UNSUPPORTED;
    }
    VMP_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL(chain_input_combine_kernel, dim3((unsigned)((used + NT - 1) / NT)), dim3(NT),
                       0, ctx->stream, nslice, ncross, used, total, work, Snz, Spz, Szz);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
