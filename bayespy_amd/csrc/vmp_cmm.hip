// vmp_cmm.hip -- the plate pass of the fused categorical-mixture block (latent class model)
//
//     R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
//     P = Dirichlet(conc, plates=(D, K));  X = Mixture(Z, Categorical, P);  X.observe(x)
//
// (the reference forms the (N, D, K) log-density <log P>[x], the (N, D, K, M) message to P and the
// (N, K) responsibilities, mixture.py / categorical.py).  Here x is kept as one byte per entry
// (vmp_cmm_pack, 255 = hidden) and one pass over the rows leaves the sufficient statistics only.
// Per tile of 64 rows, with the clusters on the KP lanes of a lane group (vmp_cmm_dev.h):
//
//   phase 1   a lane group takes a row and walks its D bytes, which are the same for the whole
//             group (an LDS broadcast); lane k adds L[x, d, k], one load from the category-major
//             table, whose K values are contiguous.  lse over the group by butterflies; r goes to
//             an LDS tile, N_k and sum lse stay in registers.
//   phase 2   the columns are dealt out to the wavefronts and lane groups; the group that owns
//             column d walks the 64 rows in ascending order and adds r_k to its own cell
//             (x, d, k) of the LDS count table.  One lane per cell, one cell per lane and step:
//             no LDS atomics, and the bank depends on the lane alone.
//
// THE TABLE <log P> IS READ FROM L2, NOT STAGED IN LDS: the LDS of a CU is the count table's
// (112 of 160 KB at the cap); a second table of the same size does not fit, and the D M K doubles
// (64 KB at D = 32, M = 8, K = 32) are read by every workgroup and stay resident in the 4 MB L2 of
// an XCD, as the word-major table of hmmc_pass_kernel does.
//
// No floating-point atomics: a workgroup owns a chunk of consecutive rows and leaves one partial
// S, N_k and sum lse; cmm_combine_kernel adds the partials in chunk order.
#include <mutex>

#include "vmp_common.h"
#include "vmp_cmm_dev.h"

namespace {

struct CmmArgs {
    int64_t N, chunk;
    int D, K, M;
    const uint8_t *x;          // N x D bytes
    const int32_t *labels;     // fixed classes (r = one-hot, lse = 0) or null
    const double *L;           // M x D x K
    const double *c;           // K
    double *part;              // chunks x vmp_cmm_partial_doubles
    double *r_out;             // N x K or null
};

template <int KP>
__device__ __forceinline__ double grp_max(double v)
{
#pragma unroll
    for (int off = KP / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

template <int KP>
__device__ __forceinline__ double grp_sum(double v)
{
#pragma unroll
    for (int off = KP / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The mask, the range check and the end of the chunk only select values and skip a lane's own
// accumulation: every shuffle and barrier stays in workgroup-uniform control flow.
template <int KP>
__global__ void __launch_bounds__(VMP_CMM_NT) cmm_pass_kernel(CmmArgs a)
{
    extern __shared__ double cmm_lds[];
    constexpr int G = 64 / KP, NG = 4 * G;
    const int D = a.D, K = a.K, M = a.M;
    const int cells = (int)vmp_cmm_cells(D, K, M);
    double *cnt = cmm_lds;                              // vmp_cmm_cell
    double *r_s = cnt + cells;                          // [t * KP + k]
    double *nk_s = r_s + VMP_CMM_TILE * KP;             // [group * KP + k]
    double *lse_s = nk_s + VMP_CMM_NT;                  // [group]
    uint8_t *x_s = (uint8_t *)(lse_s + 16);             // [t * D + d]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane / KP, k = lane % KP;
    const int gid = wave * G + g;
    const bool act = k < K, soft = a.labels == nullptr;
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t r1 = (r0 + a.chunk < a.N) ? r0 + a.chunk : a.N;

    for (int e = tid; e < cells; e += VMP_CMM_NT) cnt[e] = 0.0;
    const double cval = act ? a.c[k] : -INFINITY;
    double nk = 0.0, lsum = 0.0;

    for (int64_t row0 = r0; row0 < r1; row0 += VMP_CMM_TILE) {
        // -- the bytes of the tile; past the end of the chunk: hidden -------------------------------
        const int rows = (int)((r1 - row0 < VMP_CMM_TILE) ? r1 - row0 : VMP_CMM_TILE);
        const int nb = rows * D;
        const uint8_t *src = a.x + row0 * D;
        const bool aligned = ((uintptr_t)src & 7) == 0;
        for (int i = tid; i < 8 * D; i += VMP_CMM_NT) {       // 64 D bytes are 8 D words
            uint64_t v;
            if (aligned && 8 * i + 8 <= nb) {
                v = ((const uint64_t *)src)[i];
            } else {
                v = 0;
                for (int b = 0; b < 8; ++b) {
                    const uint64_t byte = (8 * i + b < nb) ? src[8 * i + b] : VMP_CMM_HIDDEN;
                    v |= byte << (8 * b);
                }
            }
            ((uint64_t *)x_s)[i] = v;
        }
        __syncthreads();

        // -- phase 1: the rows t = group, group + NG, ... of the tile -----------------------------
#pragma unroll 1
        for (int t = gid; t < VMP_CMM_TILE; t += NG) {
            const int64_t row = row0 + t;
            const bool valid = t < rows;
            const uint8_t *xr = x_s + t * D;
            double lg = 0.0;
            bool any = false;
#pragma unroll 4
            for (int d = 0; d < D; ++d) {
                const uint8_t xb = xr[d];
                const bool obs = vmp_cmm_observed(xb, M);
                any |= obs;
                if (soft && obs && act)
                    lg = vmp_cmm_logit_step(lg, a.L[((int64_t)xb * D + d) * K + k]);
            }
            lg = vmp_cmm_logit_finish(lg, cval);              // -inf on the padding lanes
            double lse = 0.0, rv;
            if (soft) {
                const double m = grp_max<KP>(lg);
                const double s = grp_sum<KP>(vmp_cmm_shifted_exp(lg, m));
                lse = vmp_cmm_lse(m, s);
                rv = vmp_cmm_resp(lg, lse);
            } else {
                const int lab = valid ? a.labels[row] : -1;
                rv = (k == lab) ? 1.0 : 0.0;
            }
            // a row with nothing observed keeps its r for r_out and adds nothing to the sums
            const bool counted = valid && any;
            const double rs = counted ? rv : 0.0;
            r_s[t * KP + k] = rs;
            nk += rs;
            if (counted) lsum += lse;
            if (a.r_out && valid && act) a.r_out[row * K + k] = rv;
        }
        __syncthreads();

        // -- phase 2: this group's columns d = cb G + g, cb = wave, wave + 4, ... -------------------
        for (int t = 0; t < rows; ++t) {
            const double rv = r_s[t * KP + k];
            const uint8_t *xr = x_s + t * D;
            for (int cb = wave; cb * G < D; cb += 4) {
                const int d = cb * G + g;
                if (d < D) {
                    const uint8_t xb = xr[d];
                    if (vmp_cmm_observed(xb, M)) cnt[(cb * M + xb) * 64 + lane] += rv;
                }
            }
        }
        __syncthreads();                 // r_s and x_s are free for the next tile
    }

    // -- the partial of this chunk: S category-major, then N_k and sum lse in group order ----------
    const int64_t MDK = (int64_t)M * D * K;
    double *part = a.part + (int64_t)blockIdx.x * vmp_cmm_partial_doubles(D, K, M);
    for (int e = tid; e < (int)MDK; e += VMP_CMM_NT) {
        const int kk = e % K, md = e / K, d = md % D, m = md / D;
        part[e] = cnt[vmp_cmm_cell(d, m, kk, M, KP)];
    }
    nk_s[gid * KP + k] = nk;
    if (k == 0) lse_s[gid] = lsum;
    __syncthreads();
    if (tid < K) {
        double t = 0.0;
        for (int s = 0; s < NG; ++s) t += nk_s[s * KP + tid];
        part[MDK + tid] = t;
    }
    if (tid == 0) {
        double t = 0.0;
        for (int s = 0; s < NG; ++s) t += lse_s[s];
        part[MDK + K] = t;
    }
}

// one thread per element of a partial: the chunks in order
__global__ void __launch_bounds__(VMP_CMM_NT)
cmm_combine_kernel(int64_t nc, int64_t MDK, int K, const double *__restrict__ part,
                   double *__restrict__ S, double *__restrict__ Nk, double *__restrict__ sum_lse)
{
    const int64_t per = MDK + K + 1;
    const int64_t e = (int64_t)blockIdx.x * VMP_CMM_NT + threadIdx.x;
    if (e >= per) return;
    double v = 0.0;
    for (int64_t c = 0; c < nc; ++c) v += part[c * per + e];
    if (e < MDK) S[e] = v;
    else if (e < MDK + K) Nk[e - MDK] = v;
    else sum_lse[0] = v;
}

// L = <log P> as it stands (category-major already), or zero; c = <log pi> less its largest element
__global__ void __launch_bounds__(VMP_CMM_NT)
cmm_tables_kernel(int64_t MDK, int K, const double *__restrict__ elog_p,
                  const double *__restrict__ elog_pi, double *__restrict__ L,
                  double *__restrict__ c)
{
    const int64_t idx = (int64_t)blockIdx.x * VMP_CMM_NT + threadIdx.x;
    if (idx < MDK) L[idx] = elog_p ? elog_p[idx] : 0.0;
    if (blockIdx.x == 0 && idx < K) {
        double m = elog_pi[0];
        for (int k = 1; k < K; ++k) m = fmax(m, elog_pi[k]);
        c[idx] = elog_pi[idx] - m;
    }
}

__device__ __forceinline__ uint8_t cmm_byte(double v, bool seen, int M, bool *bad)
{
    return vmp_cmm_byte_f64(v, seen, M, bad);
}
__device__ __forceinline__ uint8_t cmm_byte(int64_t v, bool seen, int M, bool *bad)
{
    return vmp_cmm_byte_i64(v, seen, M, bad);
}
__device__ __forceinline__ uint8_t cmm_byte(int32_t v, bool seen, int M, bool *bad)
{
    return vmp_cmm_byte_i64((int64_t)v, seen, M, bad);
}
__device__ __forceinline__ uint8_t cmm_byte(uint8_t v, bool seen, int M, bool *bad)
{
    return vmp_cmm_byte_i64((int64_t)v, seen, M, bad);
}

template <typename T>
__global__ void __launch_bounds__(VMP_CMM_NT)
cmm_pack_kernel(int64_t n, int M, const T *__restrict__ x, const uint8_t *__restrict__ mask,
                uint8_t *__restrict__ xb, int32_t *flag)
{
    const int64_t idx = (int64_t)blockIdx.x * VMP_CMM_NT + threadIdx.x;
    if (idx >= n) return;
    const bool seen = mask ? mask[idx] != 0 : true;
    bool bad = false;
    xb[idx] = cmm_byte(x[idx], seen, M, &bad);
    if (bad) *flag = 1;
}

template <int KP>
int32_t launch_pass(vmp_ctx *ctx, int64_t nc, const CmmArgs &a)
{
    const size_t lds = (size_t)vmp_cmm_lds_bytes(a.D, a.K, a.M);
    static std::once_flag raised[64];           // per instance and device; host threads may race
    if (lds > 48 * 1024) {
        hipError_t err = hipSuccess;
        std::call_once(raised[ctx->device & 63], [&] {
            err = hipFuncSetAttribute((const void *)cmm_pass_kernel<KP>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        });
        VMP_HIP_CHECK(ctx, err);
    }
    hipLaunchKernelGGL((cmm_pass_kernel<KP>), dim3((unsigned)nc), dim3(VMP_CMM_NT), lds,
                       ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // namespace

extern "C" {

int32_t vmp_cmm_limits(int32_t *max_K, int32_t *min_M, int32_t *max_M, int32_t *max_cells)
{
    if (!max_K || !min_M || !max_M || !max_cells) return VMP_ERR_INVALID;
    *max_K = VMP_CMM_MAX_K;
    *min_M = VMP_CMM_MIN_M;
    *max_M = VMP_CMM_MAX_M;
    *max_cells = VMP_CMM_MAX_CELLS;
    return VMP_OK;
}

int32_t vmp_cmm_plan(int64_t N, int32_t D, int32_t K, int32_t M, int64_t *chunk_rows,
                     int64_t *workspace_doubles)
{
    if (N < 0 || D < 1 || K < 1 || M < 1 || !chunk_rows || !workspace_doubles)
        return VMP_ERR_INVALID;
    if (!vmp_cmm_supported(D, K, M)) return VMP_ERR_UNSUPPORTED;
    *chunk_rows = vmp_cmm_chunk_rows(N, D, K, M);
    *workspace_doubles = vmp_cmm_chunks(N, D, K, M) * vmp_cmm_partial_doubles(D, K, M) + 1024;
    return VMP_OK;
}

int32_t vmp_cmm_pack(vmp_ctx *ctx, int64_t N, int32_t D, int32_t M, int32_t dtype, const void *x,
                     const uint8_t *mask, uint8_t *xb, int32_t *flag)
{
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && M >= 1 && dtype >= 0 && dtype <= 3,
                VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, M >= VMP_CMM_MIN_M && M <= VMP_CMM_MAX_M, VMP_ERR_UNSUPPORTED,
                "M = %d is outside the limits [%d, %d]", M, VMP_CMM_MIN_M, VMP_CMM_MAX_M);
    VMP_REQUIRE(ctx, flag && (N == 0 || (x && xb)), VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    if (N == 0) return VMP_OK;
    const int64_t n = N * D;
    const dim3 grid((unsigned)((n + VMP_CMM_NT - 1) / VMP_CMM_NT)), block(VMP_CMM_NT);
    if (dtype == 0)
        hipLaunchKernelGGL(cmm_pack_kernel<double>, grid, block, 0, ctx->stream, n, M,
                           (const double *)x, mask, xb, flag);
    else if (dtype == 1)
        hipLaunchKernelGGL(cmm_pack_kernel<int64_t>, grid, block, 0, ctx->stream, n, M,
                           (const int64_t *)x, mask, xb, flag);
    else if (dtype == 2)
        hipLaunchKernelGGL(cmm_pack_kernel<uint8_t>, grid, block, 0, ctx->stream, n, M,
                           (const uint8_t *)x, mask, xb, flag);
    else
        hipLaunchKernelGGL(cmm_pack_kernel<int32_t>, grid, block, 0, ctx->stream, n, M,
                           (const int32_t *)x, mask, xb, flag);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_cmm_tables(vmp_ctx *ctx, int32_t D, int32_t K, int32_t M, const double *elog_p,
                       const double *elog_pi, double *L, double *c)
{
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1 && M >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, vmp_cmm_supported(D, K, M), VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d, M = %d exceed the limits (K <= %d, %d <= M <= %d, %d cells)", D,
                K, M, VMP_CMM_MAX_K, VMP_CMM_MIN_M, VMP_CMM_MAX_M, VMP_CMM_MAX_CELLS);
    VMP_REQUIRE(ctx, elog_pi && L && c, VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int64_t MDK = (int64_t)M * D * K;
    hipLaunchKernelGGL(cmm_tables_kernel, dim3((unsigned)((MDK + VMP_CMM_NT - 1) / VMP_CMM_NT)),
                       dim3(VMP_CMM_NT), 0, ctx->stream, MDK, K, elog_p, elog_pi, L, c);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_cmm_pass(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, int32_t M, const uint8_t *xb,
                     const int32_t *labels, const double *L, const double *c, double *ws,
                     double *S, double *Nk, double *scal, double *r_out)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && K >= 1 && M >= 1, VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, vmp_cmm_supported(D, K, M), VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d, M = %d exceed the limits (K <= %d, %d <= M <= %d, %d cells)", D,
                K, M, VMP_CMM_MAX_K, VMP_CMM_MIN_M, VMP_CMM_MAX_M, VMP_CMM_MAX_CELLS);
    VMP_REQUIRE(ctx, L && c && ws && S && Nk && scal && (N == 0 || xb), VMP_ERR_INVALID,
                "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int64_t nc = vmp_cmm_chunks(N, D, K, M);
    const int64_t per = vmp_cmm_partial_doubles(D, K, M), MDK = (int64_t)M * D * K;
    if (nc > 0) {
        CmmArgs a = {N, vmp_cmm_chunk_rows(N, D, K, M), D, K, M, xb, labels, L, c, ws, r_out};
        int32_t rc;
        switch (vmp_cmm_kpad(K)) {
        case 16: rc = launch_pass<16>(ctx, nc, a); break;
        case 32: rc = launch_pass<32>(ctx, nc, a); break;
        default: rc = launch_pass<64>(ctx, nc, a); break;
        }
        if (rc != VMP_OK) return rc;
    }
    hipLaunchKernelGGL(cmm_combine_kernel, dim3((unsigned)((per + VMP_CMM_NT - 1) / VMP_CMM_NT)),
                       dim3(VMP_CMM_NT), 0, ctx->stream, nc, MDK, K, ws, S, Nk, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    double *dot_ws = ws + nc * per;
    int32_t rc = vmp_lda_dot(ctx, K, Nk, c, dot_ws, scal + 1);
    if (rc != VMP_OK) return rc;
    return vmp_lda_dot(ctx, MDK, S, L, dot_ws, scal + 2);
}

}  // extern "C"
