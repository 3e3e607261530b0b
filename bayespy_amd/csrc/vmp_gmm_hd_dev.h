// vmp_gmm_hd_dev.h -- the two plate kernels of the high-dimensional form of the Gaussian-mixture
// block (vmp_gmm_hd.hip: 1 <= D <= 64, K <= 64; the plan uses it for 33 <= D <= 64).
//
// The compact feature list of vmp_gmm.hip / vmp_gmm_wide.hip has 2145 entries at D = 64: the
// statistics accumulators of one 16-cluster tile would be more than 1000 registers per lane.  This
// form contracts over the matrices themselves, D padded to DP = 16 DT in {16, 32, 48, 64}:
//
//   gmm_hd_resp_kernel   ell_nk = c_k + y^T (h_k + A_k y), A_k = -1/2 <Lambda_k>, as the matrix
//                        product Z = A_k Y_tile^T followed by the column sums of Z o Y_tile^T; the
//                        softmax over k (utils/misc.py:1388-1401); R (N, K) and sum_n lse_n
//   gmm_hd_s2_kernel     S2_k = (r_k o Y)^T Y on the upper 16 x 16 tiles, and with the operand
//                        r_k o Y already in registers also S1_k = r_k^T Y and R_k = sum r_k
//
// Both leave one partial per workgroup; gmm_hd_reduce_kernel (vmp_gmm_hd.hip) adds them in a fixed
// order.  No atomics, nothing of size (N, K, D).
#pragma once
#include "vmp_gmm_dev.h"

namespace {

constexpr int HD_MAXD = 64, HD_MAXK = 64;
constexpr int HD_NW = 4;                          // responsibility kernel: wavefronts of a workgroup
constexpr int HD_PT = 4;                          // ... point tiles of a wavefront
constexpr int HD_WGP = HD_NW * HD_PT * TNC;       // ... points of a workgroup per trip (256)
constexpr int HD_NW2 = 8;                         // second-moment kernel: wavefronts = clusters
constexpr int HD_SLAB = 64;                       // ... points of the shared Y slab

constexpr int hd_ls(int DP) { return DP + 4; }                        // row stride of A_k in LDS
constexpr int hd_ys(int DP) { return DP % 32 == 0 ? DP + 16 : DP; }   // row stride of the Y slab
constexpr int hd_rsk(int KP) { return KP + 1; }                       // row stride of the r tile
constexpr int hd_ntiles(int DT) { return DT * (DT + 1) / 2; }         // upper 16 x 16 tiles
// partial of one (chunk, cluster): [R_k, 7 pad, S1 (DP), upper tiles of S2 (256 each)]
constexpr int hd_ps(int DT) { return 8 + 16 * DT + 256 * hd_ntiles(DT); }
constexpr size_t hd_resp_lds(int DT, int KT)
{
    return (size_t)(2 * 16 * DT * hd_ls(16 * DT) + 2 * 16 * DT + 256
                    + HD_NW * TNC * hd_rsk(16 * KT) + 8) * sizeof(double);
}

// ---------------------------------------------------------------------------
// Responsibilities.  A persistent workgroup of four wavefronts owns 256 points per trip, 64 per
// wavefront as four 16-point tiles whose y values stay in registers: lane (l15, g) holds
// y[n = l15][d = 4q + g], q < 4 DT -- the B operand of Z = A_k Y^T (k-step q) AND, because
// 16 et + g + 4 r = 4 (4 et + r) + g, the factor of the result element Z[16 et + g + 4 r][n] the
// lane receives.  A_k (DP x DP, 32 KB at DP = 64; the K of them are 2 MB: L2) is staged through
// LDS, double-buffered over k: the workgroup fetches A_{k+1} into registers before the matrix
// instructions of k and stores it behind them, one barrier per k.  A fragment read from LDS serves
// the four tiles of the wavefront, whose four accumulators are independent chains.
//   ell[n] = c_k + sum over the lane groups g of  sum_q y[n][4q + g] (Z[4q + g][n] + h_k[4q + g])
// Lane group g parks ell of the clusters k = 4 j + g in the point's own row of R (256 logits per
// lane would not fit beside the y values; the row is in L2 and about to be written anyway) and
// the SAME lane reads them back after the last k: program order, no fence.  The softmax is then
// the one of vmp_gmm.hip -- row maximum, table exponential, p = e / sum -- and the row is
// overwritten with r.
// ---------------------------------------------------------------------------
template <int DT, int KT>
__global__ void __launch_bounds__(64 * HD_NW, 1)
gmm_hd_resp_kernel(const double *__restrict__ Y, int64_t N, int D, int K,
                   const double *__restrict__ C, int64_t F2P, double *__restrict__ Rout,
                   double *__restrict__ Plse, int64_t ntrips)
{
    constexpr int DP = 16 * DT, KP = 16 * KT, KQ = 4 * KT, NQ = 4 * DT;
    constexpr int LS = hd_ls(DP), RSK = hd_rsk(KP), NTP = 64 * HD_NW;
    constexpr int NST = DP * DP / NTP;            // staged elements of A_k per thread
    static_assert(DP * DP % NTP == 0 && DP <= NTP, "staging covers A_k and h_k");

    extern __shared__ double lds[];
    double *Ab = lds;                             // [2][DP][LS]
    double *hb = Ab + 2 * DP * LS;                // [2][DP]
    double *tab = hb + 2 * DP;                    // 256
    double *rtb = tab + 256;                      // [HD_NW][16][RSK]
    double *red = rtb + HD_NW * TNC * RSK;        // [HD_NW]
    const int tid = threadIdx.x;
    const int l = tid & 63, l15 = l & 15, g = l >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *rt = rtb + w * TNC * RSK;
    for (int e = tid; e < 256; e += NTP) tab[e] = VMP_EXP2_TAB[e];
    const uint32_t tab_addr = (uint32_t)(uintptr_t)(lds_f64 *)tab;

    // A_k and h_k of the natural table row [c_k, h_k (D), A_k (D x D)], zero beyond D
    auto stage_load = [&](int k, double (&sa)[NST], double &sh) {
        const double *Ck = C + (int64_t)k * F2P;
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = tid + NTP * i, row = e / DP, col = e % DP;
            sa[i] = (row < D && col < D) ? Ck[1 + D + row * D + col] : 0.0;
        }
        sh = tid < D ? Ck[1 + tid] : 0.0;
    };
    auto stage_store = [&](int buf, const double (&sa)[NST], double sh) {
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = tid + NTP * i, row = e / DP, col = e % DP;
            Ab[buf * DP * LS + row * LS + col] = sa[i];
        }
        if (tid < DP) hb[buf * DP + tid] = sh;
    };

    double s_lse = 0.0;
    for (int64_t trip = 0; trip < ntrips; ++trip) {
        // every wavefront of the grid walks the same number of trips (the barriers); the surplus
        // ones hold zeros and write nothing
        const int64_t base = (trip * gridDim.x + blockIdx.x) * HD_WGP + (int64_t)w * (HD_PT * TNC);
        double yf[HD_PT][NQ];
#pragma unroll
        for (int t = 0; t < HD_PT; ++t) {
            const int64_t n = base + t * TNC + l15;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int d = 4 * q + g;
                yf[t][q] = (n < N && d < D) ? Y[n * D + d] : 0.0;
            }
        }
        double sa[NST], sh;
        stage_load(0, sa, sh);
        stage_store(0, sa, sh);
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            const bool more = k + 1 < K;
            if (more) stage_load(k + 1, sa, sh);
            const double *A = Ab + (k & 1) * DP * LS;
            const double *h = hb + (k & 1) * DP;
            const double ck = C[(int64_t)k * F2P];
            double part[HD_PT];
#pragma unroll
            for (int t = 0; t < HD_PT; ++t) part[t] = 0.0;
#pragma unroll
            for (int et = 0; et < DT; ++et) {
                v4f64 acc[HD_PT];
#pragma unroll
                for (int t = 0; t < HD_PT; ++t) acc[t] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    // keep the fragment reads next to their use (hoisted together they spill)
                    if ((q & 7) == 0) asm volatile("" ::: "memory");
                    const double a = A[(16 * et + l15) * LS + 4 * q + g];
#pragma unroll
                    for (int t = 0; t < HD_PT; ++t) acc[t] = mfma_f64(a, yf[t][q], acc[t]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double hh = h[16 * et + 4 * r + g];
#pragma unroll
                    for (int t = 0; t < HD_PT; ++t)
                        part[t] = __builtin_fma(yf[t][4 * et + r], acc[t][r] + hh, part[t]);
                }
            }
            const bool mine = (k & 3) == g;
#pragma unroll
            for (int t = 0; t < HD_PT; ++t) {
                double p = part[t];
                p += __shfl_xor(p, 16, 64);
                p += __shfl_xor(p, 32, 64);
                const int64_t n = base + t * TNC + l15;
                if (mine && n < N) Rout[n * K + k] = ck + p;
            }
            if (more) stage_store((k + 1) & 1, sa, sh);
            __syncthreads();
        }

        // ---- softmax over k for the point n = l15 of every tile; lane holds k = 4 j + g -------
#pragma unroll
        for (int t = 0; t < HD_PT; ++t) {
            const int64_t n0 = base + t * TNC;
            const bool nok = n0 + l15 < N;
            double ell[KQ];
#pragma unroll
            for (int j = 0; j < KQ; ++j)
                ell[j] = (nok && 4 * j + g < K) ? Rout[(n0 + l15) * K + 4 * j + g] : -INFINITY;
            double mx = ell[0];
#pragma unroll
            for (int j = 1; j < KQ; ++j) mx = fmax(mx, ell[j]);
            mx = fmax(mx, __shfl_xor(mx, 16, 64));
            mx = fmax(mx, __shfl_xor(mx, 32, 64));
            if (!isfinite(mx)) mx = 0.0;
            double s = 0.0;
#pragma unroll
            for (int j0 = 0; j0 < KQ; j0 += 4) {
                double v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = ell[j0 + i];
                exp_tab_batch<4>(v, mx, tab_addr);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ell[j0 + i] = v[i];
                    s += v[i];
                }
            }
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            // the four lane groups of a point hold the same (mx, s): group 0 counts
            if (g == 0 && nok) s_lse += mx + log(s);
            const double is = nok ? recip_small(s) : 0.0;
#pragma unroll
            for (int j = 0; j < KQ; ++j) rt[l15 * RSK + 4 * j + g] = ell[j] * is;
            lds_fence();
            // the rows n0 .. n0 + 15 of R (N, K) are one contiguous block
            const int64_t left = N - n0;
            const int rows = left >= TNC ? TNC : (left > 0 ? (int)left : 0);
            for (int e = l; e < rows * K; e += 64) {
                const int nn = e / K, kk = e - nn * K;
                Rout[n0 * K + e] = rt[nn * RSK + kk];
            }
            lds_fence();
        }
    }

    s_lse = wave_sum(s_lse);
    if (l == 0) red[w] = s_lse;
    __syncthreads();
    if (tid == 0) Plse[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------
// Second moments (and, from the same operand, S1 and R_k).  A workgroup of eight wavefronts takes
// eight clusters -- wavefront w owns cluster 8 blockIdx.x + w -- and the point chunk blockIdx.y;
// the grid is cluster groups x point chunks.  The wavefronts share a 64-point slab of Y in LDS
// (the next one is fetched into registers during the matrix instructions) and read their column
// of the R just written.  For the points n = 4 q + g of a 16-point tile lane (l15, g) forms
//   ya[a] = r[n][k] y[n][16 a + l15]     (A operand: rows d1 = 16 a + l15 of (r_k o Y)^T)
//   yt[b] =           y[n][16 b + l15]     (B operand: columns d2 = 16 b + l15 of Y)
// and adds ya[a] x yt[b] to the accumulator of every upper tile a <= b: DT (DT + 1) / 2 tiles,
// 10 at DP = 64 = 80 registers.  S1[16 a + l15] is the sum of ya[a] over the tile's points,
// R_k the sum of r.  The lower triangle is mirrored by the reduce kernel.
// ---------------------------------------------------------------------------
template <int DT>
__global__ void __launch_bounds__(64 * HD_NW2)
gmm_hd_s2_kernel(const double *__restrict__ Y, int64_t N, int D, int K,
                 const double *__restrict__ R, double *__restrict__ P, int64_t nslabs, int KP8)
{
    constexpr int DP = 16 * DT, YS = hd_ys(DP), NTP = 64 * HD_NW2;
    constexpr int NST = DP * HD_SLAB / NTP, NTL = hd_ntiles(DT), PS = hd_ps(DT);
    static_assert(DP * HD_SLAB % NTP == 0, "staging covers the slab");

    extern __shared__ double ysl[];               // [HD_SLAB][YS]
    const int tid = threadIdx.x;
    const int l = tid & 63, l15 = l & 15, g = l >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.x * HD_NW2 + w;
    const bool active = k < K;

    auto slab_load = [&](int64_t slab, double (&sy)[NST]) {
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = tid + NTP * i, row = e / DP, col = e % DP;
            const int64_t n = slab * HD_SLAB + row;
            sy[i] = (n < N && col < D) ? Y[n * D + col] : 0.0;
        }
    };
    auto slab_store = [&](const double (&sy)[NST]) {
#pragma unroll
        for (int i = 0; i < NST; ++i) {
            const int e = tid + NTP * i, row = e / DP, col = e % DP;
            ysl[row * YS + col] = sy[i];
        }
    };

    v4f64 acc[NTL];
#pragma unroll
    for (int i = 0; i < NTL; ++i) acc[i] = v4f64{0.0, 0.0, 0.0, 0.0};
    double s1[DT], nk = 0.0;
#pragma unroll
    for (int a = 0; a < DT; ++a) s1[a] = 0.0;

    double sy[NST];
    const int64_t nchunk = gridDim.y;
    int64_t slab = blockIdx.y;
    if (slab < nslabs) {
        slab_load(slab, sy);
        slab_store(sy);
    }
    __syncthreads();
    for (; slab < nslabs; slab += nchunk) {
        const bool more = slab + nchunk < nslabs;
        if (more) slab_load(slab + nchunk, sy);
        if (active) {
            double rv[HD_SLAB / 4];
#pragma unroll
            for (int i = 0; i < HD_SLAB / 4; ++i) {
                const int64_t n = slab * HD_SLAB + 4 * i + g;
                rv[i] = n < N ? R[n * K + k] : 0.0;
            }
#pragma unroll
            for (int i = 0; i < HD_SLAB / 4; ++i) {
                const double *yrow = ysl + (4 * i + g) * YS + l15;
                double yt[DT], ya[DT];
#pragma unroll
                for (int a = 0; a < DT; ++a) {
                    yt[a] = yrow[16 * a];
                    ya[a] = rv[i] * yt[a];
                    s1[a] += ya[a];
                }
                nk += rv[i];
                int tix = 0;
#pragma unroll
                for (int a = 0; a < DT; ++a)
#pragma unroll
                    for (int b = a; b < DT; ++b, ++tix) acc[tix] = mfma_f64(ya[a], yt[b], acc[tix]);
            }
        }
        __syncthreads();                          // every wavefront is done with the slab
        if (more) slab_store(sy);
        __syncthreads();
    }

    if (!active) return;
    double *Pk = P + ((int64_t)blockIdx.y * KP8 + k) * PS;
    nk += __shfl_xor(nk, 16, 64);
    nk += __shfl_xor(nk, 32, 64);
    if (l == 0) Pk[0] = nk;
#pragma unroll
    for (int a = 0; a < DT; ++a) {
        double s = s1[a];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (g == 0) Pk[8 + 16 * a + l15] = s;
    }
    // lane holds element (g + 4 r, l15) of every tile
#pragma unroll
    for (int i = 0; i < NTL; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) Pk[8 + DP + 256 * i + (g + 4 * r) * 16 + l15] = acc[i][r];
}

}  // namespace

// vmp_gmm.hip: kernels of the block that do not depend on D beyond a table size
int32_t vmp_gmm_launch_update_alpha(vmp_ctx *ctx, const vmp_gmm_layout &L, int D, int K,
                                    double *state);
int32_t vmp_gmm_launch_lower_bound_hd(vmp_ctx *ctx, const vmp_gmm_layout &L, int D, int K,
                                      double *state);
