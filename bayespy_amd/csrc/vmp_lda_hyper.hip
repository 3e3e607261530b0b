// vmp_lda_hyper.hip -- what the latent-Dirichlet-allocation block needs to learn a concentration
//
// vmp_lda_concentration_stats: one pass over the parameters and <log> moments of rows x cols
// Dirichlet rows leaves S[c] = sum_rows elog[r, c] (the Dirichlets' message to their concentration)
// and qterm, the part of the node's lower-bound term that does not depend on the prior
// (vmp_lda_hyper_dev.h has the formulas, the layout and the order of every addition).  Both tables
// are read once; the work per element is one lgamma and a handful of error-free additions, since
// everything that enters qterm is kept as an unevaluated sum hi + lo until the last addition.
//
// The two memory forms of the block take one kernel: M memory rows of W <= 1024 contiguous doubles,
// a wavefront per chunk of memory rows, lane j holding the positions j + 64 i in R registers -- a row
// is R coalesced loads of 512 bytes per table, and up to R = 8 the next row is requested before the
// arithmetic of the present one.  The tall form (p_topic, D x K) sums alpha along the row and elog down the
// chunk; the transposed form (p_word as V x K) sums elog along the row, which is a finished S[c],
// and alpha down the chunk.  No atomics: chunk partials, then a combine in a fixed order.
//
// vmp_lda_prior_fill writes a cols vector into every row of a prior table in either form, so the
// Dirichlet kernels of vmp_lda.hip keep reading a full prior table.
#include "vmp_common.h"
#include "vmp_lda_hyper_dev.h"

namespace {

constexpr int LDAH_NT = 256;         // four wavefronts = four chunks per workgroup
constexpr int LDAH_FILL_MAX_BLOCKS = 4096;

__device__ __forceinline__ double wave_sum_bfly(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the butterfly of unevaluated sums: every lane ends with the same bits (vmp_dd_add_dd is symmetric)
__device__ __forceinline__ vmp_dd wave_sum_bfly_dd(vmp_dd v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const vmp_dd o = {__shfl_xor(v.hi, off, 64), __shfl_xor(v.lo, off, 64)};
        vmp_dd_add_dd(v, o);
    }
    return v;
}

template <int R>
__device__ __forceinline__ void load_row(double (&dst)[R], const double *__restrict__ row,
                                         const int (&kc)[R])
{
#pragma unroll
    for (int i = 0; i < R; ++i) dst[i] = row[kc[i]];
}

// TR: the transposed form.  S is written here in the transposed form only; the `down` partials are
// plain doubles in part_hi in the tall form (elog) and hi + lo in the transposed form (alpha).
template <int R, bool TR>
__global__ void __launch_bounds__(LDAH_NT)
lda_hyper_pass_kernel(int64_t M, int W, int T, int64_t nchunks, const double *__restrict__ alpha,
                      const double *__restrict__ elog, double *__restrict__ part_hi,
                      double *__restrict__ part_lo, double *__restrict__ q_hi,
                      double *__restrict__ q_lo, double *__restrict__ S)
{
    // the next memory row is requested before the arithmetic of the present one where the
    // registers allow it
    constexpr bool AHEAD = R <= 8;
    const int64_t c = ((int64_t)blockIdx.x * LDAH_NT + threadIdx.x) / VMP_LDA_HYPER_LANES;
    const int lane = threadIdx.x & (VMP_LDA_HYPER_LANES - 1);
    if (c >= nchunks) return;                    // whole wavefronts leave together
    bool act[R];
    int kc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        const int w = lane + VMP_LDA_HYPER_LANES * i;
        act[i] = w < W;
        kc[i] = act[i] ? w : W - 1;              // clamped into the row; dropped below
    }
    const int64_t m0 = c * T;
    const int64_t m1 = (m0 + T < M) ? m0 + T : M;
    double down[R], dlo[TR ? R : 1], a[R], e[R];
#pragma unroll
    for (int i = 0; i < R; ++i) down[i] = 0.0;
#pragma unroll
    for (int i = 0; i < (TR ? R : 1); ++i) dlo[i] = 0.0;
    vmp_dd q = {0.0, 0.0}, tot = {0.0, 0.0};
    if (AHEAD) {
        load_row<R>(a, alpha + m0 * W, kc);
        load_row<R>(e, elog + m0 * W, kc);
    }
    for (int64_t m = m0; m < m1; ++m) {
        double an[AHEAD ? R : 1], en[AHEAD ? R : 1];
        if constexpr (AHEAD) {
            const int64_t mn = (m + 1 < m1) ? m + 1 : m;
            load_row<R>(an, alpha + mn * W, kc);
            load_row<R>(en, elog + mn * W, kc);
        } else {
            load_row<R>(a, alpha + m * W, kc);
            load_row<R>(e, elog + m * W, kc);
        }
        if (!TR) q = {0.0, 0.0};                 // tall: a row's terms cancel inside the row
        vmp_dd asum = {0.0, 0.0};
        double esum = 0.0;
#pragma unroll
        for (int i = 0; i < R; ++i) {
            if (TR) {
                const double x = act[i] ? e[i] : 0.0;
                esum = (i == 0) ? x : esum + x;
            }
            if (act[i]) {
                vmp_lda_hyper_q_add(q, a[i], e[i]);
                if (TR) {
                    vmp_dd d = {down[i], dlo[TR ? i : 0]};
                    vmp_dd_add(d, a[i]);
                    down[i] = d.hi;
                    dlo[TR ? i : 0] = d.lo;
                } else {
                    down[i] += e[i];
                    vmp_dd_add(asum, a[i]);
                }
            }
        }
        if (TR) {
            esum = wave_sum_bfly(esum);
            if (lane == 0) S[m] = esum;
        } else {
            asum = wave_sum_bfly_dd(asum);
            vmp_dd row = wave_sum_bfly_dd(q);
            double lo;
            const double lg = vmp_lda_hyper_lgamma(asum.hi, asum.lo, &lo);
            vmp_dd_add(row, lg);
            row.lo += lo;
            vmp_dd_add_dd(tot, row);
        }
        if constexpr (AHEAD) {
#pragma unroll
            for (int i = 0; i < R; ++i) {
                a[i] = an[i];
                e[i] = en[i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < R; ++i)
        if (act[i]) {
            part_hi[c * W + lane + VMP_LDA_HYPER_LANES * i] = down[i];
            if (TR) part_lo[c * W + lane + VMP_LDA_HYPER_LANES * i] = dlo[TR ? i : 0];
        }
    if (TR) tot = wave_sum_bfly_dd(q);
    if (lane == 0) {
        q_hi[c] = tot.hi;
        q_lo[c] = tot.lo;
    }
}

// the `down` partials of 64 positions per workgroup: wavefront g adds its slice of the chunks in
// chunk order, then the slices are added in slice order.  Tall: out_hi = the total (S).  TR: the
// totals are row sums of alpha, hi + lo, and out_hi + out_lo = lgamma of them
template <bool TR>
__global__ void __launch_bounds__(VMP_LDA_HYPER_GROUPS * VMP_LDA_HYPER_LANES)
lda_hyper_cols_kernel(int64_t nchunks, int W, const double *__restrict__ part_hi,
                      const double *__restrict__ part_lo, double *__restrict__ out_hi,
                      double *__restrict__ out_lo)
{
    __shared__ double sh[VMP_LDA_HYPER_GROUPS][VMP_LDA_HYPER_LANES];
    __shared__ double sl[VMP_LDA_HYPER_GROUPS][VMP_LDA_HYPER_LANES];
    const int j = threadIdx.x & (VMP_LDA_HYPER_LANES - 1);
    const int g = threadIdx.x / VMP_LDA_HYPER_LANES;
    const int w = blockIdx.x * VMP_LDA_HYPER_LANES + j;
    const int64_t per = vmp_lda_hyper_slice(nchunks);
    const int64_t b = g * per;
    const int64_t e = (b + per < nchunks) ? b + per : nchunks;
    vmp_dd s = {0.0, 0.0};
    if (w < W)
        for (int64_t c = b; c < e; ++c) {
            if (TR) {
                const vmp_dd x = {part_hi[c * W + w], part_lo[c * W + w]};
                vmp_dd_add_dd(s, x);
            } else {
                s.hi += part_hi[c * W + w];
            }
        }
    sh[g][j] = s.hi;
    sl[g][j] = s.lo;
    __syncthreads();
    if (g == 0 && w < W) {
        vmp_dd t = {sh[0][j], sl[0][j]};
        for (int i = 1; i < VMP_LDA_HYPER_GROUPS; ++i) {
            if (TR) {
                const vmp_dd x = {sh[i][j], sl[i][j]};
                vmp_dd_add_dd(t, x);
            } else {
                t.hi += sh[i][j];
            }
        }
        if (TR) {
            double lo;
            out_hi[w] = vmp_lda_hyper_lgamma(t.hi, t.lo, &lo);
            out_lo[w] = lo;
        } else {
            out_hi[w] = t.hi;
        }
    }
}

// out[0] = hi + lo of the sum of the cnt unevaluated sums hi[i] + lo[i], in a fixed order
__global__ void __launch_bounds__(VMP_LDA_HYPER_RED_NT)
lda_hyper_sum_final_kernel(int64_t cnt, const double *__restrict__ hi,
                           const double *__restrict__ lo, double *__restrict__ out)
{
    __shared__ double rh[VMP_LDA_HYPER_RED_NT / 64], rl[VMP_LDA_HYPER_RED_NT / 64];
    vmp_dd v = {0.0, 0.0};
    for (int64_t i = threadIdx.x; i < cnt; i += VMP_LDA_HYPER_RED_NT) {
        const vmp_dd x = {hi[i], lo[i]};
        vmp_dd_add_dd(v, x);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const vmp_dd o = {__shfl_down(v.hi, off, 64), __shfl_down(v.lo, off, 64)};
        vmp_dd_add_dd(v, o);                     // valid in lane 0
    }
    if ((threadIdx.x & 63) == 0) {
        rh[threadIdx.x >> 6] = v.hi;
        rl[threadIdx.x >> 6] = v.lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        vmp_dd t = {rh[0], rl[0]};
        for (int i = 1; i < VMP_LDA_HYPER_RED_NT / 64; ++i) {
            const vmp_dd x = {rh[i], rl[i]};
            vmp_dd_add_dd(t, x);
        }
        out[0] = t.hi + t.lo;
    }
}

// prior[r * rs + c * cs] = a[c]; the index runs along the axis with the smaller stride
__global__ void __launch_bounds__(LDAH_NT)
lda_prior_fill_kernel(int64_t rows, int64_t cols, int64_t rs, int64_t cs,
                      const double *__restrict__ a, double *__restrict__ prior)
{
    const int64_t tot = rows * cols;
    const int64_t step = (int64_t)gridDim.x * LDAH_NT;
    for (int64_t idx = (int64_t)blockIdx.x * LDAH_NT + threadIdx.x; idx < tot; idx += step) {
        int64_t r, c;
        if (cs <= rs) {
            r = idx / cols;
            c = idx - r * cols;
        } else {
            c = idx / rows;
            r = idx - c * rows;
        }
        prior[r * rs + c * cs] = a[c];
    }
}

template <bool TR>
void launch_pass(vmp_ctx *ctx, int64_t M, int W, int T, int64_t nc, const double *alpha,
                 const double *elog, double *part, double *part_lo, double *q_hi, double *q_lo,
                 double *S)
{
    const int64_t waves_per_block = LDAH_NT / VMP_LDA_HYPER_LANES;
    const dim3 grid((unsigned)((nc + waves_per_block - 1) / waves_per_block)), block(LDAH_NT);
    switch (vmp_lda_hyper_regs(W)) {
    case 1:
        hipLaunchKernelGGL((lda_hyper_pass_kernel<1, TR>), grid, block, 0, ctx->stream, M, W, T, nc,
                           alpha, elog, part, part_lo, q_hi, q_lo, S);
        break;
    case 2:
        hipLaunchKernelGGL((lda_hyper_pass_kernel<2, TR>), grid, block, 0, ctx->stream, M, W, T, nc,
                           alpha, elog, part, part_lo, q_hi, q_lo, S);
        break;
    case 4:
        hipLaunchKernelGGL((lda_hyper_pass_kernel<4, TR>), grid, block, 0, ctx->stream, M, W, T, nc,
                           alpha, elog, part, part_lo, q_hi, q_lo, S);
        break;
    case 8:
        hipLaunchKernelGGL((lda_hyper_pass_kernel<8, TR>), grid, block, 0, ctx->stream, M, W, T, nc,
                           alpha, elog, part, part_lo, q_hi, q_lo, S);
        break;
    default:
        hipLaunchKernelGGL((lda_hyper_pass_kernel<16, TR>), grid, block, 0, ctx->stream, M, W, T,
                           nc, alpha, elog, part, part_lo, q_hi, q_lo, S);
        break;
    }
}

// 0: tall (row-major), 1: transposed, -1: neither
inline int hyper_form(int64_t rows, int64_t cols, int64_t rs, int64_t cs)
{
    if (cs == 1 && rs == cols && cols <= VMP_LDA_HYPER_MAX_W) return 0;
    if (rs == 1 && cs == rows && rows <= VMP_LDA_HYPER_MAX_W) return 1;
    return -1;
}

}  // namespace

extern "C" {

int32_t vmp_lda_concentration_stats_workspace(int64_t rows, int64_t cols, int64_t row_stride,
                                              int64_t col_stride, int64_t *workspace_doubles)
{
    if (rows < 0 || cols < 1 || row_stride < 1 || col_stride < 1 || !workspace_doubles)
        return VMP_ERR_INVALID;
    if (rows == 0) {
        *workspace_doubles = 1;
        return VMP_OK;
    }
    const int form = hyper_form(rows, cols, row_stride, col_stride);
    if (form < 0) return VMP_ERR_UNSUPPORTED;
    *workspace_doubles = form == 0 ? vmp_lda_hyper_ws_doubles(rows, (int)cols)
                                   : vmp_lda_hyper_ws_doubles(cols, (int)rows);
    return VMP_OK;
}

int32_t vmp_lda_concentration_stats(vmp_ctx *ctx, int64_t rows, int64_t cols, int64_t row_stride,
                                    int64_t col_stride, const double *alpha, const double *elog,
                                    double *ws, double *S, double *qterm)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && rows >= 0 && cols >= 1 && row_stride >= 1 && col_stride >= 1,
                VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, S && qterm && ws && (rows == 0 || (alpha && elog)), VMP_ERR_INVALID,
                "null argument");
    if (rows == 0) {
        VMP_HIP_CHECK(ctx, hipMemsetAsync(S, 0, sizeof(double) * cols, ctx->stream));
        VMP_HIP_CHECK(ctx, hipMemsetAsync(qterm, 0, sizeof(double), ctx->stream));
        return VMP_OK;
    }
    const int form = hyper_form(rows, cols, row_stride, col_stride);
    VMP_REQUIRE(ctx, form >= 0, VMP_ERR_UNSUPPORTED,
                "the table is neither row-major with cols <= %d nor transposed (row_stride == 1, "
                "col_stride == rows) with rows <= %d", VMP_LDA_HYPER_MAX_W, VMP_LDA_HYPER_MAX_W);
    const bool tr = form == 1;
    const int64_t M = tr ? cols : rows;
    const int W = (int)(tr ? rows : cols);
    const int T = vmp_lda_hyper_chunk_rows(M);
    const int64_t nc = vmp_lda_hyper_chunks(M);
    // scalars: [nc] chunk scalars then [W] lgamma of the row sums, a hi array and a lo array
    const int64_t ns = nc + W;
    double *s_hi = ws, *s_lo = ws + ns, *part = ws + 2 * ns, *part_lo = part + nc * W;
    const dim3 cgrid((unsigned)((W + VMP_LDA_HYPER_LANES - 1) / VMP_LDA_HYPER_LANES));
    const dim3 cblock(VMP_LDA_HYPER_GROUPS * VMP_LDA_HYPER_LANES);
    if (tr) {
        launch_pass<true>(ctx, M, W, T, nc, alpha, elog, part, part_lo, s_hi, s_lo, S);
        hipLaunchKernelGGL(lda_hyper_cols_kernel<true>, cgrid, cblock, 0, ctx->stream, nc, W, part,
                           part_lo, s_hi + nc, s_lo + nc);
        hipLaunchKernelGGL(lda_hyper_sum_final_kernel, dim3(1), dim3(VMP_LDA_HYPER_RED_NT), 0,
                           ctx->stream, ns, s_hi, s_lo, qterm);
    } else {
        launch_pass<false>(ctx, M, W, T, nc, alpha, elog, part, part_lo, s_hi, s_lo, nullptr);
        hipLaunchKernelGGL(lda_hyper_cols_kernel<false>, cgrid, cblock, 0, ctx->stream, nc, W, part,
                           part_lo, S, (double *)nullptr);
        hipLaunchKernelGGL(lda_hyper_sum_final_kernel, dim3(1), dim3(VMP_LDA_HYPER_RED_NT), 0,
                           ctx->stream, nc, s_hi, s_lo, qterm);
    }
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_lda_prior_fill(vmp_ctx *ctx, int64_t rows, int64_t cols, int64_t row_stride,
                           int64_t col_stride, const double *a, double *prior)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && rows >= 0 && cols >= 1 && row_stride >= 1 && col_stride >= 1,
                VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, rows == 0 || (a && prior), VMP_ERR_INVALID, "null argument");
    if (rows == 0) return VMP_OK;
    int64_t grid = (rows * cols + LDAH_NT - 1) / LDAH_NT;
    if (grid > LDAH_FILL_MAX_BLOCKS) grid = LDAH_FILL_MAX_BLOCKS;
    hipLaunchKernelGGL(lda_prior_fill_kernel, dim3((unsigned)grid), dim3(LDAH_NT), 0, ctx->stream,
                       rows, cols, row_stride, col_stride, a, prior);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
