// vmp_chain_tv_dev.h -- how vmp_chain_pair_stats (vmp_chain_tv.hip) splits its work and in which
// order every output element is accumulated, shared by the kernels and the host build of the CPU
// tests.  Plain integer / fp64 code: include after <math.h> / <stdint.h> with __host__ and
// __device__ defined.
//
// Sxx[t][i][j] = sum_b x[b][t][i] x[b][t][j],  Sxp[t][i][j] = sum_b x[b][t][i] x[b][t+1][j].
// The ny sequences are cut into `nslice` contiguous slices of `per` sequences.  Within a slice an
// element is ONE chain of fused multiply-adds over b in ascending order, starting from +0; the
// slice partials are then added in ascending slice order, starting from partial 0.  Nothing else
// enters a sum, so the result depends on (ny, N, D) and the data alone.
#pragma once

#define VMP_CHAIN_TV_MAX_D 16        // largest state dimension with an instance
#define VMP_CHAIN_TV_NT 256          // lanes of a workgroup of the first stage
#define VMP_CHAIN_TV_BB 8            // sequences staged in LDS per step
#define VMP_CHAIN_TV_TARGET_WGS 1024 // workgroups the first stage aims for (4 per CU of 256)

// time instances of a workgroup's tile: one lane per (t, i) of the tile
__host__ __device__ inline int vmp_chain_tv_tile(int D) { return VMP_CHAIN_TV_NT / D; }

__host__ __device__ inline int64_t vmp_chain_tv_ntile(int N, int D)
{
    const int TT = vmp_chain_tv_tile(D);
    return ((int64_t)N + TT - 1) / TT;
}

// sequences per slice: enough slices to reach the target grid, whole staging steps, at least one
__host__ __device__ inline int64_t vmp_chain_tv_per(int64_t ny, int N, int D)
{
    const int64_t ntile = vmp_chain_tv_ntile(N, D);
    int64_t want = (VMP_CHAIN_TV_TARGET_WGS + ntile - 1) / ntile;        // slices wanted
    if (want < 1) want = 1;
    int64_t per = (ny + want - 1) / want;
    per = (per + VMP_CHAIN_TV_BB - 1) / VMP_CHAIN_TV_BB * VMP_CHAIN_TV_BB;
    if (per < VMP_CHAIN_TV_BB) per = VMP_CHAIN_TV_BB;
    return per;
}

__host__ __device__ inline int64_t vmp_chain_tv_nslice(int64_t ny, int N, int D)
{
    const int64_t per = vmp_chain_tv_per(ny, N, D);
    const int64_t ns = (ny + per - 1) / per;
    return ns < 1 ? 1 : ns;
}

// doubles of one slice's partials: Sxx (N, D, D) followed by Sxp (N-1, D, D)
__host__ __device__ inline int64_t vmp_chain_tv_total(int N, int D)
{
    return (int64_t)(2 * (int64_t)N - 1) * D * D;
}

__host__ __device__ inline int64_t vmp_chain_tv_work_doubles(int64_t ny, int N, int D)
{
    return vmp_chain_tv_nslice(ny, N, D) * vmp_chain_tv_total(N, D);
}

// one step of an element's chain
__host__ __device__ inline double vmp_chain_tv_step(double acc, double a, double b)
{
    return fma(a, b, acc);
}

// the second stage: partials[s * total + e] over s = 0 .. nslice-1 in this order
__host__ __device__ inline double vmp_chain_tv_combine(const double *partials, int64_t nslice,
                                                       int64_t total, int64_t e)
{
    double s = partials[e];
    for (int64_t k = 1; k < nslice; ++k) s += partials[k * total + e];
    return s;
}
