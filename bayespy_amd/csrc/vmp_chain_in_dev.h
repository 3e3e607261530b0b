// vmp_chain_in_dev.h -- how vmp_chain_input_stats (vmp_chain_in.hip) splits its work and in which
// order every output element is accumulated, shared by the kernels and the host build of the CPU
// tests.  Plain integer / fp64 code: include after <math.h> / <stdint.h> with __host__ and
// __device__ defined.
//
// With t = 0 .. N-2 the transitions, x (ny, N, D) the means of the states and z (zrows, N-1, K) the
// means of the inputs (zrows = ny, or 1 for inputs that every sequence shares: row 0 then stands for
// every b):
//   Snz[t][i][k] = sum_b x[b][t+1][i] z[b][t][k]      Spz[t][i][k] = sum_b x[b][t][i] z[b][t][k]
//   Szz[t][k][l] = sum_b z[b][t][k] z[b][t][l]
// The ny sequences are cut into `nslice` contiguous slices of `per` sequences.  Within a slice an
// element is ONE chain of fused multiply-adds over b in ascending order, starting from +0; the
// slice partials are then added in ascending slice order, starting from partial 0.  Nothing else
// enters a sum, so the result depends on (ny, zrows, N, D, K) and the data alone.
#pragma once

#define VMP_CHAIN_IN_MAX_D 16        // largest state dimension with an instance
#define VMP_CHAIN_IN_MAX_K 16        // largest input dimension with an instance
#define VMP_CHAIN_IN_NT 256          // lanes of a workgroup of the first stage
#define VMP_CHAIN_IN_BB 8            // sequences staged in LDS per step
#define VMP_CHAIN_IN_TARGET_WGS 1024 // workgroups the first stage aims for (4 per CU of 256)

// lanes per transition: lane i owns row i of Snz / Spz (i < D) and row i of Szz (i < K)
__host__ __device__ inline int vmp_chain_in_lanes(int D, int K) { return D > K ? D : K; }

// transitions of a workgroup's tile
__host__ __device__ inline int vmp_chain_in_tile(int D, int K)
{
    return VMP_CHAIN_IN_NT / vmp_chain_in_lanes(D, K);
}

__host__ __device__ inline int64_t vmp_chain_in_ntile(int N, int D, int K)
{
    const int TT = vmp_chain_in_tile(D, K);
    const int64_t nt = ((int64_t)N - 1 + TT - 1) / TT;
    return nt < 1 ? 1 : nt;
}

// sequences per slice: enough slices to reach the target grid, whole staging steps, at least one
__host__ __device__ inline int64_t vmp_chain_in_per(int64_t ny, int N, int D, int K)
{
    const int64_t ntile = vmp_chain_in_ntile(N, D, K);
    int64_t want = (VMP_CHAIN_IN_TARGET_WGS + ntile - 1) / ntile;        // slices wanted
    if (want < 1) want = 1;
    int64_t per = (ny + want - 1) / want;
    per = (per + VMP_CHAIN_IN_BB - 1) / VMP_CHAIN_IN_BB * VMP_CHAIN_IN_BB;
    if (per < VMP_CHAIN_IN_BB) per = VMP_CHAIN_IN_BB;
    return per;
}

__host__ __device__ inline int64_t vmp_chain_in_nslice(int64_t ny, int N, int D, int K)
{
    const int64_t per = vmp_chain_in_per(ny, N, D, K);
    const int64_t ns = (ny + per - 1) / per;
    return ns < 1 ? 1 : ns;
}

// doubles of one of the two cross blocks, Snz or Spz: (N-1, D, K)
__host__ __device__ inline int64_t vmp_chain_in_cross(int N, int D, int K)
{
    return ((int64_t)N - 1) * D * K;
}

// doubles of one slice's partials: Snz, Spz (N-1, D, K) each, followed by Szz (N-1, K, K)
__host__ __device__ inline int64_t vmp_chain_in_total(int N, int D, int K)
{
    return 2 * vmp_chain_in_cross(N, D, K) + ((int64_t)N - 1) * K * K;
}

__host__ __device__ inline int64_t vmp_chain_in_work_doubles(int64_t ny, int N, int D, int K)
{
    return vmp_chain_in_nslice(ny, N, D, K) * vmp_chain_in_total(N, D, K);
}

// one step of an element's chain
__host__ __device__ inline double vmp_chain_in_step(double acc, double a, double b)
{
    return fma(a, b, acc);
}

// the second stage: partials[s * total + e] over s = 0 .. nslice-1 in this order
__host__ __device__ inline double vmp_chain_in_combine(const double *partials, int64_t nslice,
                                                       int64_t total, int64_t e)
{
    double s = partials[e];
    for (int64_t k = 1; k < nslice; ++k) s += partials[k * total + e];
    return s;
}
