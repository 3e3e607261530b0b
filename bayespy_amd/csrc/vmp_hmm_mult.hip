// vmp_hmm_mult.hip -- the pass of the fused hidden-Markov-model block with multinomial emissions:
// every time step carries a vector of counts over M categories
//
//     Z = CategoricalMarkovChain(a0, A, states=T);  Y = Mixture(Z, Multinomial, n, P);  Y.observe(x)
//
// The categorical block (vmp_hmm_cat.hip) is the n = 1 case, which avoids the product by a lookup.
// Here the two products over the flattened (b, t) plate stand on either side of the chain:
//
//   hmmm_emit_kernel<NT>    E = X <log P>^T, every row less its largest element, on the fp64
//                           matrix cores; the counts are read as uint16 (8 bytes per lane), staged
//                           in LDS and widened on the way into the instruction; the word-major
//                           table streams through LDS in chunks of words
//   hmmw_chain_kernel<KP>   the recursion alone (vmp_hmm_wide.hip, through vmp_hmmw_chain): reads E,
//                           leaves gamma in the workspace and one partial per workgroup
//   hmmm_stats_kernel<NT>   S = X^T Gamma on the matrix cores, split over word slabs and row ranges
//   hmmm_combine_kernel     adds every partial in workgroup order
//   hmmm_shift_kernel       gives sum log Z and sum gamma . e the row shifts of E back
//
// Splits, workspace and the order of the additions: vmp_hmm_mult_dev.h.  Matrix-core layout of
// v_mfma_f64_16x16x4f64 (lane l, l15 = l & 15, l4 = l >> 4): A[row l15][k l4], B[k l4][col l15],
// accumulator element r = D[row l4 + 4 r][col l15].
#include <mutex>

#include "vmp_common.h"
#include "vmp_hmm_mult_dev.h"

namespace {

constexpr int HMMM_WCH = VMP_HMMM_W_CHUNK;
constexpr int HMMM_XE = HMMM_WCH + 8;                       // uint16 per staged row, emission kernel
constexpr int HMMM_SW = VMP_HMMM_SLAB_TILES * 16;           // words of a slab
constexpr int HMMM_XS = HMMM_SW + 16;                       // uint16 per staged row, statistics kernel

// Four counts of row r from word w0 on (w0 a multiple of 4): one 8-byte load where the address
// allows, else the tail path word by word; zeros past M.  The caller has checked r and w0 < M.
__device__ __forceinline__ uint2 hmmm_load4(const uint16_t *__restrict__ x, int64_t r, int M, int w0,
                                            bool fast)
{
    const int64_t off = r * M + w0;
    if (fast && (off & 3) == 0 && w0 + 3 < M) return *reinterpret_cast<const uint2 *>(x + off);
    unsigned v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (w0 + j < M) v[j] = x[off + j];
    return make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
}

// ---- the emission table -----------------------------------------------------------------------------
struct HmmmEmitArgs {
    int64_t R, nblk;              // rows of the (b, t) plate, blocks of 64 rows
    int M, K, KP, fast;           // fast: x is 8-byte aligned
    const uint16_t *x;            // R x M
    const double *Pt;             // M x K, word-major
    const uint8_t *mask;          // R bytes or null
    double *E;                    // R x KP
    double *shift;                // 4 per workgroup: a wavefront's sum of the shifts of its rows
};

// Four wavefronts, each with one tile of 16 rows; NT column tiles of 16 states.  LDS per chunk of
// HMMM_WCH words: the table (HMMM_WCH x hmmw_stride(NT) doubles) and the counts of the 64 rows
// (64 x HMMM_XE uint16).  Step q of a chunk contracts the words 4 q + l4; a row's counts are
// staged so that the 16 words of one l4 are contiguous, xs[row][16 l4 + q], and a lane fetches
// them with two 16-byte reads.
// THE ROW SHIFT.  With counts in the hundreds e is of the order of -1000, and the chain recursion
// adds e to log-probabilities of order 1 before it normalises: every such sum would be rounded at
// ulp(1000).  So a row is stored less its largest element over the states, c = max_k e[k]: the
// states that compete at a step have E near 0, and the posterior does not change.  c is 0 at a
// masked row.  sum log Z and sum gamma . e both grow by the sum of c over the rows (gamma adds up
// to 1 at a step); a wavefront leaves the sum over all its rows, block after block, and
// hmmm_shift_kernel adds these.  The grid is a function of R alone, so the order is fixed.
template <int NT>
__global__ __launch_bounds__(256) void hmmm_emit_kernel(HmmmEmitArgs a)
{
    extern __shared__ double hmmm_lds[];
    constexpr int KPC = NT * 16, CS = hmmw_stride(NT), WCH = HMMM_WCH, XE = HMMM_XE;
    const int M = a.M, K = a.K, KP = a.KP;
    double *Cs = hmmm_lds;
    uint16_t *xs = reinterpret_cast<uint16_t *>(Cs + WCH * CS);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const uint4 *myx = reinterpret_cast<const uint4 *>(xs + (w * 16 + l15) * XE + l4 * 16);

    double csum = 0.0;          // this lane's rows l4, l4 + 4, l4 + 8, l4 + 12 of every block, in order
    for (int64_t blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {
        const int64_t row0 = blk * 64;
        v4f64 acc[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) acc[ct] = v4f64{0.0, 0.0, 0.0, 0.0};
        for (int c0 = 0; c0 < M; c0 += WCH) {
            __syncthreads();                        // the readers of the previous chunk are done
            for (int e = tid; e < WCH * KPC; e += 256) {
                const int ww = e / KPC, k = e % KPC;
                Cs[ww * CS + k] = (k < K && c0 + ww < M) ? a.Pt[(int64_t)(c0 + ww) * K + k] : 0.0;
            }
            // zeros for a masked row, past the end of the plate and past the last word
            for (int e = tid; e < 64 * (WCH / 4); e += 256) {
                const int i = e / (WCH / 4), qd = e % (WCH / 4), w0 = c0 + 4 * qd;
                const int64_t r = row0 + i;
                uint2 v = make_uint2(0u, 0u);
                if (r < a.R && w0 < M && (!a.mask || a.mask[r] != 0))
                    v = hmmm_load4(a.x, r, M, w0, a.fast != 0);
                uint16_t *dst = xs + i * XE + qd;
                dst[0] = (uint16_t)(v.x & 0xffffu);
                dst[16] = (uint16_t)(v.x >> 16);
                dst[32] = (uint16_t)(v.y & 0xffffu);
                dst[48] = (uint16_t)(v.y >> 16);
            }
            __syncthreads();
            const int nq = (((M - c0 < WCH) ? M - c0 : WCH) + 3) >> 2;
            const uint4 xa = myx[0], xb = myx[1];
            const unsigned xw[8] = {xa.x, xa.y, xa.z, xa.w, xb.x, xb.y, xb.z, xb.w};
#pragma unroll
            for (int q = 0; q < WCH / 4; ++q) {
                if (q < nq) {                       // uniform over the workgroup
                    const double cnt = (double)((xw[q >> 1] >> ((q & 1) * 16)) & 0xffffu);
                    const double *cb = Cs + (4 * q + l4) * CS + l15;
#pragma unroll
                    for (int ct = 0; ct < NT; ++ct)
                        acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(cnt, cb[ct * 16], acc[ct], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int64_t r = row0 + w * 16 + l4 + 4 * r4;
            const bool obs = r < a.R && (!a.mask || a.mask[r] != 0);
            double c = -INFINITY;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct)
                if (ct * 16 + l15 < K) c = fmax(c, acc[ct][r4]);
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) c = fmax(c, __shfl_xor(c, m, 64));
            if (!obs) c = 0.0;
            csum += c;
            if (r >= a.R) continue;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const int k = ct * 16 + l15;
                if (k < KP) a.E[r * KP + k] = k >= K ? -INFINITY : (obs ? acc[ct][r4] - c : 0.0);
            }
        }
    }
    csum += __shfl_xor(csum, 16, 64);
    csum += __shfl_xor(csum, 32, 64);
    if (lane == 0) a.shift[blockIdx.x * 4 + w] = csum;
}

// one workgroup: the n sums of the row shifts (element e belongs to thread e % 256, the 256 sums
// are halved eight times) are added to scal[0] = sum log Z and scal[1] = sum gamma . e
__global__ void __launch_bounds__(256)
hmmm_shift_kernel(int64_t n, const double *__restrict__ shift, double *__restrict__ scal)
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

// ---- the count statistics ---------------------------------------------------------------------------
struct HmmmStatsArgs {
    int64_t R, rpw;               // rows of the plate, rows of a workgroup
    int M, K, fast;
    const uint16_t *x;
    const double *gam;            // R x K (the in-place gamma of the chain kernel)
    const uint8_t *mask;
    double *part;                 // row ranges x M x K
};

// Workgroup (blockIdx.x = row range, blockIdx.y = word slab), four wavefronts with two 16-word
// tiles each and all NT state tiles: 2 NT accumulators.  A step stages VMP_HMMM_ROWS rows of the
// slab's counts (uint16) and of gamma in LDS; the A operand is the transposed count tile, read
// along the words and widened, the B operand gamma.
template <int NT>
__global__ __launch_bounds__(256) void hmmm_stats_kernel(HmmmStatsArgs a)
{
    extern __shared__ double hmmm_lds[];
    constexpr int GS = hmmw_stride(NT), RW = VMP_HMMM_ROWS, TPW = VMP_HMMM_SLAB_TILES / 4;
    constexpr int SW = HMMM_SW, XS = HMMM_XS;
    const int M = a.M, K = a.K, NWT = (M + 15) / 16;
    double *gs = hmmm_lds;                                              // [RW][GS]
    uint16_t *xs = reinterpret_cast<uint16_t *>(gs + RW * GS);          // [RW][XS]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int slab0 = blockIdx.y * SW;
    const int tile0 = blockIdx.y * VMP_HMMM_SLAB_TILES + w * TPW;
    v4f64 acc[NT][TPW];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < TPW; ++i) acc[kt][i] = v4f64{0.0, 0.0, 0.0, 0.0};

    const int64_t r_begin = (int64_t)blockIdx.x * a.rpw;
    const int64_t r_end = (r_begin + a.rpw < a.R) ? r_begin + a.rpw : a.R;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += RW) {
        __syncthreads();
        for (int e = tid; e < RW * (SW / 4); e += 256) {
            const int i = e / (SW / 4), qd = e % (SW / 4), w0 = slab0 + 4 * qd;
            const int64_t r = r0 + i;
            uint2 v = make_uint2(0u, 0u);
            if (r < r_end && w0 < M && (!a.mask || a.mask[r] != 0))
                v = hmmm_load4(a.x, r, M, w0, a.fast != 0);
            *reinterpret_cast<uint2 *>(xs + i * XS + 4 * qd) = v;
        }
        for (int e = tid; e < RW * NT * 16; e += 256) {
            const int i = e / (NT * 16), k = e % (NT * 16);
            const int64_t r = r0 + i;
            const bool ok = r < r_end && k < K && (!a.mask || a.mask[r] != 0);
            gs[i * GS + k] = ok ? a.gam[r * K + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RW / 4; ++q) {
            const uint16_t *xr = xs + (4 * q + l4) * XS + w * TPW * 16 + l15;
            const double *gr = gs + (4 * q + l4) * GS + l15;
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                if (tile0 + i >= NWT) continue;             // uniform over the wavefront
                const double cnt = (double)xr[i * 16];
#pragma unroll
                for (int kt = 0; kt < NT; ++kt)
                    acc[kt][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(cnt, gr[kt * 16], acc[kt][i], 0, 0, 0);
            }
        }
    }
    double *part = a.part + (int64_t)blockIdx.x * M * K;
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int m = (tile0 + i) * 16 + l4 + 4 * r4;
            if (m >= M) continue;
#pragma unroll
            for (int kt = 0; kt < NT; ++kt) {
                const int k = kt * 16 + l15;
                if (k < K) part[(int64_t)m * K + k] = acc[kt][i][r4];
            }
        }
}

// ---- combine: every partial in workgroup order ------------------------------------------------------
// element e < per: the chain partials (z0sum, xisum, scal[0], scal[1]); then the M x K elements of S
__global__ void __launch_bounds__(256)
hmmm_combine_kernel(int64_t nwc, int64_t nwr, int M, int K, const double *__restrict__ cpart,
                    const double *__restrict__ spart, double *__restrict__ z0sum,
                    double *__restrict__ xisum, double *__restrict__ S, double *__restrict__ scal)
{
    const int64_t per = vmp_hmmw_chain_partial_doubles(K), MK = (int64_t)M * K;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per + MK) return;
    double v = 0.0;
    if (e < per) {
        for (int64_t w = 0; w < nwc; ++w) v += cpart[w * per + e];
        if (e < K) z0sum[e] = v;
        else if (e < per - 2) xisum[e - K] = v;
        else scal[e - (per - 2)] = v;
        return;
    }
    for (int64_t w = 0; w < nwr; ++w) v += spart[w * MK + (e - per)];
    S[e - per] = v;
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
int32_t launch_emit(vmp_ctx *ctx, const HmmmEmitArgs &a)
{
    const size_t lds = (size_t)HMMM_WCH * hmmw_stride(NT) * sizeof(double)
                       + (size_t)64 * HMMM_XE * sizeof(uint16_t);
    static std::once_flag raised[64];
    VMP_HIP_CHECK(ctx, raise_lds(ctx, hmmm_emit_kernel<NT>, lds, raised));
    hipLaunchKernelGGL((hmmm_emit_kernel<NT>), dim3((unsigned)vmp_hmmm_emit_wgs(a.R)), dim3(256),
                       lds, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

template <int NT>
int32_t launch_stats(vmp_ctx *ctx, int64_t nwr, const HmmmStatsArgs &a)
{
    const size_t lds = (size_t)VMP_HMMM_ROWS * hmmw_stride(NT) * sizeof(double)
                       + (size_t)VMP_HMMM_ROWS * HMMM_XS * sizeof(uint16_t);
    hipLaunchKernelGGL((hmmm_stats_kernel<NT>), dim3((unsigned)nwr, (unsigned)vmp_hmmm_slabs(a.M)),
                       dim3(256), lds, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // namespace

// the stages around a chain stage (vmp_hmm_mult_dev.h); NT = 8 serves the wide-state pass
int32_t vmp_hmmm_stages(vmp_ctx *ctx, int64_t B, int T, int M, int K, int64_t nwc,
                        vmp_hmmm_chain_fn chain, const uint16_t *x_packed, const double *elogPt,
                        const double *elog_a0, const double *elog_A, const int32_t *labels,
                        const uint8_t *mask, double *ws, double *z0sum, double *xisum, double *S,
                        double *scal, double *gamma, double *z0, double *zz)
{
    const int KP = vmp_hmmf_kpad(K), NT = vmp_hmmm_state_tiles(K);
    const int64_t R = B * (int64_t)T;
    const int64_t nwr = vmp_hmmm_row_wgs(R, M, K);
    const int64_t per = vmp_hmmw_chain_partial_doubles(K);
    double *E = ws, *aw = E + R * KP, *cpart = aw + R * K, *spart = cpart + nwc * per;
    double *shift = spart + nwr * (int64_t)M * K, *dot_ws = shift + 4 * vmp_hmmm_emit_wgs(R);
    const int fast = ((uintptr_t)x_packed & 7) == 0;
    int32_t rc = VMP_OK;
    const bool emit = R > 0 && elogPt && !labels;
    if (R > 0) {
        if (emit) {
            HmmmEmitArgs ea = {R, (R + 63) / 64, M, K, KP, fast, x_packed, elogPt, mask, E, shift};
            rc = NT == 1 ? launch_emit<1>(ctx, ea) : NT == 2 ? launch_emit<2>(ctx, ea)
                 : NT == 4 ? launch_emit<4>(ctx, ea) : launch_emit<8>(ctx, ea);
            if (rc != VMP_OK) return rc;
        }
        rc = chain(ctx, B, T, K, emit ? E : nullptr, elog_a0, elog_A, labels, mask, aw, cpart, gamma,
                   z0, zz);
        if (rc != VMP_OK) return rc;
        HmmmStatsArgs sa = {R, vmp_hmmm_rows_per_wg(R, M, K), M, K, fast, x_packed, aw, mask, spart};
        rc = NT == 1 ? launch_stats<1>(ctx, nwr, sa) : NT == 2 ? launch_stats<2>(ctx, nwr, sa)
             : NT == 4 ? launch_stats<4>(ctx, nwr, sa) : launch_stats<8>(ctx, nwr, sa);
        if (rc != VMP_OK) return rc;
    }
    const int64_t ne = per + (int64_t)M * K;
    hipLaunchKernelGGL(hmmm_combine_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0,
                       ctx->stream, nwc, nwr, M, K, cpart, spart, z0sum, xisum, S, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    if (emit) {
        hipLaunchKernelGGL(hmmm_shift_kernel, dim3(1), dim3(256), 0, ctx->stream,
                           4 * vmp_hmmm_emit_wgs(R), shift, scal);
        VMP_HIP_CHECK(ctx, hipGetLastError());
    }
    rc = vmp_lda_dot(ctx, K, z0sum, elog_a0, dot_ws, scal + 2);
    if (rc != VMP_OK) return rc;
    return vmp_lda_dot(ctx, (int64_t)K * K, xisum, elog_A, dot_ws, scal + 3);
}

extern "C" {

int32_t vmp_hmm_mult_limits(int32_t *max_K, int32_t *max_M, int32_t *max_count)
{
    if (!max_K || !max_M || !max_count) return VMP_ERR_INVALID;
    *max_K = VMP_HMMM_MAX_K;
    *max_M = VMP_HMMM_MAX_M;
    *max_count = VMP_HMMM_MAX_COUNT;
    return VMP_OK;
}

int32_t vmp_hmm_mult_plan(int64_t B, int32_t T, int32_t M, int32_t K, int64_t *chains_per_wg,
                          int64_t *workspace_doubles)
{
    if (B < 0 || T < 2 || M < 1 || K < 1) return VMP_ERR_INVALID;
    if (K > VMP_HMMM_MAX_K || M > VMP_HMMM_MAX_M) return VMP_ERR_UNSUPPORTED;
    if (!chains_per_wg || !workspace_doubles) return VMP_ERR_INVALID;
    *chains_per_wg = vmp_hmmw_chains_per_wg(B, K);
    *workspace_doubles = vmp_hmmm_workspace_doubles(B, T, M, K);
    return VMP_OK;
}

int32_t vmp_hmm_mult_pass(vmp_ctx *ctx, int64_t B, int32_t T, int32_t M, int32_t K,
                          const uint16_t *x_packed, const double *elogPt, const double *elog_a0,
                          const double *elog_A, const int32_t *labels, const uint8_t *mask,
                          double *ws, double *z0sum, double *xisum, double *S, double *scal,
                          double *gamma, double *z0, double *zz)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, B >= 0 && T >= 2 && M >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_HMMM_MAX_K && M <= VMP_HMMM_MAX_M, VMP_ERR_UNSUPPORTED,
                "M = %d, K = %d exceed the limits (%d, %d)", M, K, VMP_HMMM_MAX_M, VMP_HMMM_MAX_K);
    VMP_REQUIRE(ctx, ctx && elog_a0 && elog_A && ws && z0sum && xisum && S && scal
                     && (B == 0 || x_packed), VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    return vmp_hmmm_stages(ctx, B, T, M, K, vmp_hmmw_chain_wgs(B, K), vmp_hmmw_chain, x_packed, elogPt,
                           elog_a0, elog_A, labels, mask, ws, z0sum, xisum, S, scal, gamma, z0, zz);
}

}  // extern "C"
