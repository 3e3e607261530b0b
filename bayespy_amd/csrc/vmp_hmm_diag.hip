// vmp_hmm_diag.hip -- the pass of the fused hidden-Markov-model block with diagonal-Gaussian
// emissions: every time step carries D real numbers with one precision per dimension
//
//     Z = CategoricalMarkovChain(a0, A, states=T)
//     mu = GaussianARD(m0, beta0, shape=(D,), plates=(K,));  tau = Gamma(a0, b0, plates=(K, D))
//     Y = Mixture(Z, GaussianARD, mu, tau, 1);  Y.observe(y)
//
// The three-stage split of the multinomial pass (vmp_hmm_mult.hip) with real observations: the two
// products over the flattened (b, t) plate stand on either side of the chain.
//
//   hmmd_emit_kernel<NT>    E = g + Y h + (Y o Y) q as one contraction of length 2 D on the fp64
//                           matrix cores, every row less its largest element; y is read once, the
//                           square is formed in registers; the stacked table [h; q] streams
//                           through LDS in chunks of dimensions
//   hmmw_chain_kernel<KP>   the recursion alone (vmp_hmm_wide.hip, through vmp_hmmw_chain): reads E,
//                           leaves gamma in the workspace and one partial per workgroup
//   hmmd_stats_kernel<NT>   S1 = Y^T Gamma, S2 = (Y o Y)^T Gamma on the matrix cores and Nk, split
//                           over dimension slabs and row ranges; y is read once for both products
//   hmmd_combine_kernel     adds every partial in workgroup order
//   hmmd_shift_kernel       gives sum log Z and sum gamma . e the row shifts of E back
//
// Splits, workspace and the order of the additions: vmp_hmm_diag_dev.h.  Matrix-core layout of
// v_mfma_f64_16x16x4f64 (lane l, l15 = l & 15, l4 = l >> 4): A[row l15][k l4], B[k l4][col l15],
// accumulator element r = D[row l4 + 4 r][col l15].
#include <mutex>

#include "vmp_common.h"
#include "vmp_hmm_diag_dev.h"

namespace {

constexpr int HMMD_DCH = VMP_HMMD_D_CHUNK;
constexpr int HMMD_YS = HMMD_DCH + 2;                       // doubles per staged row, emission kernel
constexpr int HMMD_SW = VMP_HMMD_SLAB_TILES * 16;           // dimensions of a slab
constexpr int HMMD_XS = HMMD_SW + 16;                       // doubles per staged row, statistics kernel

// ---- the emission table -----------------------------------------------------------------------------
struct HmmdEmitArgs {
    int64_t R, nblk;              // rows of the (b, t) plate, blocks of 64 rows
    int D, K, KP;
    const double *y;              // R x D
    const double *h, *q, *g;      // D x K, D x K, K
    const uint8_t *mask;          // R bytes or null
    double *E;                    // R x KP
    double *shift;                // 4 per workgroup: a wavefront's sum of the shifts of its rows
};

// Four wavefronts, each with one tile of 16 rows; NT column tiles of 16 states.  LDS per chunk of
// c = HMMD_DCH dimensions: the stacked table (rows 0 .. c - 1 of h, then of q, row stride
// hmmw_stride(NT)) and the y of the 64 rows.  Slice qq of a chunk contracts the dimensions
// 4 qq + l4, so that the four table rows of one instruction are adjacent (distinct banks by
// hmmw_stride); a row's y is staged so that the c / 4 values of one l4 are contiguous,
// ys[row][(c / 4) l4 + qq], and a lane fetches them with c / 8 16-byte reads.  The row stride is
// c + 2 doubles = 17 x 16 bytes: the 16 rows that the lanes of one l4 read start an odd number of
// 16-byte units apart and fall into 16 distinct 16-byte bank groups, whichever of the reads it is.
// THE ROW SHIFT is that of hmmm_emit_kernel: a row is stored less c = max_k e[k] (0 at a masked
// row), the sum of c over all its rows is what a wavefront leaves, and hmmd_shift_kernel adds
// these.  The grid is a function of R alone, so the order is fixed.
template <int NT>
__global__ __launch_bounds__(256) void hmmd_emit_kernel(HmmdEmitArgs a)
{
    extern __shared__ __align__(16) double hmmd_lds[];
    constexpr int KPC = NT * 16, CS = hmmw_stride(NT), DC = HMMD_DCH, YS = HMMD_YS, NQ = DC / 4;
    const int D = a.D, K = a.K, KP = a.KP;
    double *Cs = hmmd_lds;                      // [2 DC][CS]
    double *ys = Cs + 2 * DC * CS;              // [64][YS]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const v2f64 *myy = reinterpret_cast<const v2f64 *>(ys + (w * 16 + l15) * YS + l4 * NQ);

    double csum = 0.0;          // this lane's rows l4, l4 + 4, l4 + 8, l4 + 12 of every block, in order
    for (int64_t blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {
        const int64_t row0 = blk * 64;
        v4f64 acc[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) acc[ct] = v4f64{0.0, 0.0, 0.0, 0.0};
        for (int c0 = 0; c0 < D; c0 += DC) {
            __syncthreads();                        // the readers of the previous chunk are done
            for (int e = tid; e < 2 * DC * KPC; e += 256) {
                const int rr = e / KPC, k = e % KPC, d = c0 + (rr < DC ? rr : rr - DC);
                const double *src = rr < DC ? a.h : a.q;
                Cs[rr * CS + k] = (k < K && d < D) ? src[(int64_t)d * K + k] : 0.0;
            }
            // zeros for a masked row, past the end of the plate and past the last dimension; the
            // y of such a row is not loaded
            for (int e = tid; e < 64 * DC; e += 256) {
                const int i = e / DC, j = e % DC, d = c0 + j;
                const int64_t r = row0 + i;
                double v = 0.0;
                if (r < a.R && d < D && (!a.mask || a.mask[r] != 0)) v = a.y[r * D + d];
                ys[i * YS + (j & 3) * NQ + (j >> 2)] = v;
            }
            __syncthreads();
            const int nq = (((D - c0 < DC) ? D - c0 : DC) + 3) >> 2;
            double yv[NQ];
#pragma unroll
            for (int p = 0; p < NQ / 2; ++p) {
                const v2f64 t = myy[p];
                yv[2 * p] = t[0];
                yv[2 * p + 1] = t[1];
            }
#pragma unroll
            for (int qq = 0; qq < NQ; ++qq) {
                if (qq < nq) {                      // uniform over the workgroup
                    const double *cb = Cs + (4 * qq + l4) * CS + l15;
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct)
                        acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(yv[qq], cb[ct * 16], acc[ct], 0, 0, 0);
                }
            }
#pragma unroll
            for (int qq = 0; qq < NQ; ++qq) {
                if (qq < nq) {
                    const double *cb = Cs + (DC + 4 * qq + l4) * CS + l15;
                    const double y2 = yv[qq] * yv[qq];
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct)
                        acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(y2, cb[ct * 16], acc[ct], 0, 0, 0);
                }
            }
        }
        double gk[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) gk[ct] = ct * 16 + l15 < K ? a.g[ct * 16 + l15] : 0.0;
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int64_t r = row0 + w * 16 + l4 + 4 * r4;
            const bool obs = r < a.R && (!a.mask || a.mask[r] != 0);
            double ev[NT], c = -INFINITY;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                ev[ct] = acc[ct][r4] + gk[ct];
                if (ct * 16 + l15 < K) c = fmax(c, ev[ct]);
            }
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) c = fmax(c, __shfl_xor(c, m, 64));
            if (!obs) c = 0.0;
            csum += c;
            if (r >= a.R) continue;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const int k = ct * 16 + l15;
                if (k < KP) a.E[r * KP + k] = k >= K ? -INFINITY : (obs ? ev[ct] - c : 0.0);
            }
        }
    }
    csum += __shfl_xor(csum, 16, 64);
    csum += __shfl_xor(csum, 32, 64);
    if (lane == 0) a.shift[blockIdx.x * 4 + w] = csum;
}

// one workgroup: the n sums of the row shifts (element e belongs to thread e % 256, the 256 sums
// are halved eight times) are added to scal[0] = sum log Z and scal[1] = sum gamma . e; the twin
// of hmmm_shift_kernel
__global__ void __launch_bounds__(256)
hmmd_shift_kernel(int64_t n, const double *__restrict__ shift, double *__restrict__ scal)
{
    __shared__ double ds[256];
    const int tid = threadIdx.x;
    double t = 0.0;
    for (int64_t e = tid; e < n; e += 256) t += shift[e];
    ds[tid] = t;
    __syncthreads();
    block_halve_sum<256>(ds, tid);
    if (tid == 0) {
        scal[0] += ds[0];
        scal[1] += ds[0];
    }
}

// ---- the statistics ---------------------------------------------------------------------------------
struct HmmdStatsArgs {
    int64_t R, rpw;               // rows of the plate, rows of a workgroup
    int D, K;
    const double *y;
    const double *gam;            // R x K (the in-place gamma of the chain kernel)
    const uint8_t *mask;
    double *part;                 // row ranges x vmp_hmmd_stat_doubles(D, K)
};

// Workgroup (blockIdx.x = row range, blockIdx.y = dimension slab), four wavefronts with two
// 16-dimension tiles each and all NT state tiles, for y and for y^2: 4 NT accumulators.  A step
// stages VMP_HMMD_ROWS rows of the slab's y and of gamma in LDS (row strides = 16 mod 32 doubles,
// so that the four rows 4 q + l4 of an instruction are in distinct banks); the A operand is the
// transposed y tile, read along the dimensions, and its square; the B operand gamma, shared by
// the wavefronts.  In the slab 0 workgroups thread k < 16 NT adds gamma[., k] of the staged rows.
template <int NT>
__global__ __launch_bounds__(256) void hmmd_stats_kernel(HmmdStatsArgs a)
{
    extern __shared__ __align__(16) double hmmd_lds[];
    constexpr int GS = hmmw_stride(NT), RW = VMP_HMMD_ROWS, TPW = VMP_HMMD_SLAB_TILES / 4;
    constexpr int SW = HMMD_SW, XS = HMMD_XS;
    const int D = a.D, K = a.K, NDT = (D + 15) / 16;
    double *gs = hmmd_lds;                      // [RW][GS]
    double *ys = gs + RW * GS;                  // [RW][XS]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int slab0 = blockIdx.y * SW;
    const int tile0 = blockIdx.y * VMP_HMMD_SLAB_TILES + w * TPW;
    v4f64 acc1[NT][TPW], acc2[NT][TPW];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < TPW; ++i) acc1[kt][i] = acc2[kt][i] = v4f64{0.0, 0.0, 0.0, 0.0};
    double nk = 0.0;
    const bool counts = blockIdx.y == 0 && tid < NT * 16;

    const int64_t r_begin = (int64_t)blockIdx.x * a.rpw;
    const int64_t r_end = (r_begin + a.rpw < a.R) ? r_begin + a.rpw : a.R;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += RW) {
        __syncthreads();
        for (int e = tid; e < RW * SW; e += 256) {
            const int i = e / SW, j = e % SW, d = slab0 + j;
            const int64_t r = r0 + i;
            double v = 0.0;
            if (r < r_end && d < D && (!a.mask || a.mask[r] != 0)) v = a.y[r * D + d];
            ys[i * XS + j] = v;
        }
        for (int e = tid; e < RW * NT * 16; e += 256) {
            const int i = e / (NT * 16), k = e % (NT * 16);
            const int64_t r = r0 + i;
            const bool ok = r < r_end && k < K && (!a.mask || a.mask[r] != 0);
            gs[i * GS + k] = ok ? a.gam[r * K + k] : 0.0;
        }
        __syncthreads();
        if (counts) {
#pragma unroll
            for (int i = 0; i < RW; ++i) nk += gs[i * GS + tid];
        }
#pragma unroll
        for (int q = 0; q < RW / 4; ++q) {
            const double *yr = ys + (4 * q + l4) * XS + w * TPW * 16 + l15;
            const double *gr = gs + (4 * q + l4) * GS + l15;
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                if (tile0 + i >= NDT) continue;             // uniform over the wavefront
                const double v = yr[i * 16], v2 = v * v;
#pragma unroll
                for (int kt = 0; kt < NT; ++kt) {
                    const double gv = gr[kt * 16];
                    acc1[kt][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(v, gv, acc1[kt][i], 0, 0, 0);
                    acc2[kt][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(v2, gv, acc2[kt][i], 0, 0, 0);
                }
            }
        }
    }
    const int64_t DK = (int64_t)D * K;
    double *part = a.part + (int64_t)blockIdx.x * vmp_hmmd_stat_doubles(D, K);
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int d = (tile0 + i) * 16 + l4 + 4 * r4;
            if (d >= D) continue;
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                const int k = kt * 16 + l15;
                if (k < K) {
                    part[(int64_t)d * K + k] = acc1[kt][i][r4];
                    part[DK + (int64_t)d * K + k] = acc2[kt][i][r4];
                }
            }
        }
    if (counts && tid < K) part[2 * DK + tid] = nk;
}

// ---- combine: every partial in workgroup order ------------------------------------------------------
// element e < per: the chain partials (z0sum, xisum, scal[0], scal[1]); then the D x K elements of
// S1, those of S2 and the K of Nk
__global__ void __launch_bounds__(256)
hmmd_combine_kernel(int64_t nwc, int64_t nwr, int D, int K, const double *__restrict__ cpart,
                    const double *__restrict__ spart, double *__restrict__ z0sum,
                    double *__restrict__ xisum, double *__restrict__ S1, double *__restrict__ S2,
                    double *__restrict__ Nk, double *__restrict__ scal)
{
    const int64_t per = vmp_hmmw_chain_partial_doubles(K), DK = (int64_t)D * K;
    const int64_t sd = vmp_hmmd_stat_doubles(D, K);
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per + sd) return;
    double v = 0.0;
    if (e < per) {
        for (int64_t w = 0; w < nwc; ++w) v += cpart[w * per + e];
        if (e < K) z0sum[e] = v;
        else if (e < per - 2) xisum[e - K] = v;
        else scal[e - (per - 2)] = v;
        return;
    }
    const int64_t j = e - per;
    for (int64_t w = 0; w < nwr; ++w) v += spart[w * sd + j];
    if (j < DK) S1[j] = v;
    else if (j < 2 * DK) S2[j - DK] = v;
    else Nk[j - 2 * DK] = v;
}

// the instances above 48 KB of LDS ask for it once per device; host threads may race
template <typename Kernel>
hipError_t raise_lds(vmp_ctx *ctx, Kernel kernel, size_t lds, std::once_flag *raised)
{
    hipError_t err = hipSuccess;
    if (lds > 48 * 1024)
        std::call_once(raised[ctx->device & 63], [&] {
            err = hipFuncSetAttribute((const void *)kernel,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        });
    return err;
}

template <int NT>
int32_t launch_emit(vmp_ctx *ctx, const HmmdEmitArgs &a)
{
    const size_t lds = ((size_t)2 * HMMD_DCH * hmmw_stride(NT) + (size_t)64 * HMMD_YS) * sizeof(double);
    static std::once_flag raised[64];
    VMP_HIP_CHECK(ctx, raise_lds(ctx, hmmd_emit_kernel<NT>, lds, raised));
    hipLaunchKernelGGL((hmmd_emit_kernel<NT>), dim3((unsigned)vmp_hmmd_emit_wgs(a.R)), dim3(256),
                       lds, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

template <int NT>
int32_t launch_stats(vmp_ctx *ctx, int64_t nwr, const HmmdStatsArgs &a)
{
    const size_t lds = (size_t)VMP_HMMD_ROWS * (hmmw_stride(NT) + HMMD_XS) * sizeof(double);
    hipLaunchKernelGGL((hmmd_stats_kernel<NT>), dim3((unsigned)nwr, (unsigned)vmp_hmmd_slabs(a.D)),
                       dim3(256), lds, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // namespace

extern "C" {

int32_t vmp_hmm_diag_limits(int32_t *max_K, int32_t *max_D)
{
    if (!max_K || !max_D) return VMP_ERR_INVALID;
    *max_K = VMP_HMMD_MAX_K;
    *max_D = VMP_HMMD_MAX_D;
    return VMP_OK;
}

int32_t vmp_hmm_diag_plan(int64_t B, int32_t T, int32_t D, int32_t K, int64_t *chains_per_wg,
                          int64_t *workspace_doubles)
{
    if (B < 0 || T < 2 || D < 1 || K < 1) return VMP_ERR_INVALID;
    if (K > VMP_HMMD_MAX_K || D > VMP_HMMD_MAX_D) return VMP_ERR_UNSUPPORTED;
    if (!chains_per_wg || !workspace_doubles) return VMP_ERR_INVALID;
    *chains_per_wg = vmp_hmmw_chains_per_wg(B, K);
    *workspace_doubles = vmp_hmmd_workspace_doubles(B, T, D, K);
    return VMP_OK;
}

int32_t vmp_hmm_diag_pass(vmp_ctx *ctx, int64_t B, int32_t T, int32_t D, int32_t K, const double *y,
                          const double *h, const double *q, const double *g, const double *elog_a0,
                          const double *elog_A, const int32_t *labels, const uint8_t *mask,
                          double *ws, double *z0sum, double *xisum, double *S1, double *S2,
                          double *Nk, double *scal, double *gamma, double *z0, double *zz)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, B >= 0 && T >= 2 && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_HMMD_MAX_K && D <= VMP_HMMD_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_HMMD_MAX_D, VMP_HMMD_MAX_K);
    VMP_REQUIRE(ctx, ctx && elog_a0 && elog_A && ws && z0sum && xisum && S1 && S2 && Nk && scal
                     && (B == 0 || y) && (!h || (q && g)), VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int KP = vmp_hmmf_kpad(K), NT = vmp_hmmd_state_tiles(K);
    const int64_t R = B * (int64_t)T;
    const int64_t nwc = vmp_hmmw_chain_wgs(B, K), nwr = vmp_hmmd_row_wgs(R, D, K);
    const int64_t per = vmp_hmmw_chain_partial_doubles(K);
    double *E = ws, *aw = E + R * KP, *cpart = aw + R * K, *spart = cpart + nwc * per;
    double *shift = spart + nwr * vmp_hmmd_stat_doubles(D, K);
    double *dot_ws = shift + 4 * vmp_hmmd_emit_wgs(R);
    int32_t rc = VMP_OK;
    const bool emit = R > 0 && h && !labels;
    if (R > 0) {
        if (emit) {
            HmmdEmitArgs ea = {R, (R + 63) / 64, D, K, KP, y, h, q, g, mask, E, shift};
            rc = NT == 1 ? launch_emit<1>(ctx, ea) : NT == 2 ? launch_emit<2>(ctx, ea)
                                                             : launch_emit<4>(ctx, ea);
            if (rc != VMP_OK) return rc;
        }
        rc = vmp_hmmw_chain(ctx, B, T, K, emit ? E : nullptr, elog_a0, elog_A, labels, mask, aw,
                            cpart, gamma, z0, zz);
        if (rc != VMP_OK) return rc;
        HmmdStatsArgs sa = {R, vmp_hmmd_rows_per_wg(R, D, K), D, K, y, aw, mask, spart};
        rc = NT == 1 ? launch_stats<1>(ctx, nwr, sa) : NT == 2 ? launch_stats<2>(ctx, nwr, sa)
                                                               : launch_stats<4>(ctx, nwr, sa);
        if (rc != VMP_OK) return rc;
    }
    const int64_t ne = per + vmp_hmmd_stat_doubles(D, K);
    hipLaunchKernelGGL(hmmd_combine_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0,
                       ctx->stream, nwc, nwr, D, K, cpart, spart, z0sum, xisum, S1, S2, Nk, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    if (emit) {
        hipLaunchKernelGGL(hmmd_shift_kernel, dim3(1), dim3(256), 0, ctx->stream,
                           4 * vmp_hmmd_emit_wgs(R), shift, scal);
        VMP_HIP_CHECK(ctx, hipGetLastError());
    }
    rc = vmp_lda_dot(ctx, K, z0sum, elog_a0, dot_ws, scal + 2);
    if (rc != VMP_OK) return rc;
    return vmp_lda_dot(ctx, (int64_t)K * K, xisum, elog_A, dot_ws, scal + 3);
}

}  // extern "C"
