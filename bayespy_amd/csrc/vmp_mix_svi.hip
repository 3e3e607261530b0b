// vmp_mix_svi.hip -- the global half of a stochastic-VI step of the fused count-mixture blocks
// (bayespy/demos/stochastic_inference.py on plans/bmm.py, binm.py, cmm.py, mmm.py, pmm.py)
//
// A mini-batch of N rows stands for mult times as many.  After the pass over the batch the
// parameter table of the block and the Dirichlet row of the mixing weights move along their natural
// gradients (vmp.py:432-440):
//
//     phi <- phi + scale (phi* - phi),      phi* = prior + mult * statistic
//
// with every optimum phi* taken from the statistics present at entry: the table reads `stat` / `cnt`,
// the weights read `Nk`, neither writes what the other reads.  The tables are at most 2^21 doubles
// and a step is bound by launches, so both nodes, their moments and their bound terms are ONE launch:
//
//   kind 0  Dirichlet rows, element (r, c) at r * row_stride + c * col_stride: a thread per row up to
//           64 columns, a workgroup per row above (the functions of vmp_table_dev.h, which
//           vmp_lda_dirichlet runs as well: mult = scale = 1 leaves its bits);
//   kind 1  Gamma pairs (rows, 2): a thread per element (vmp_pmm_lam_state of vmp_pmm_dev.h, which
//           vmp_pmm_update runs as well);
//   the weights row is one more workgroup, whose thread 0 owns the row.
//
// No floating-point atomics.  A workgroup of the table leaves one partial of the bound in `ws`; every
// workgroup draws a ticket, and the one that draws the last adds the partials in index order.  The
// ticket word stands behind the partials in `ws` and is cleared on the stream ahead of the launch.
// Nobody waits for anybody.  The grid is a function of
// (kind, nodes, rows, cols), so the bits of every output depend on the inputs and the shape only.
#include "vmp_common.h"
#include "vmp_table_dev.h"
#include "vmp_pmm_dev.h"

namespace {

constexpr int NT = VMP_TABLE_NT;
constexpr int MIX_MAX_K = 64;
constexpr int64_t MIX_MAX_COLS = 1024;          // the words of the multinomial block
constexpr int64_t MIX_MAX_ROWS = 65536;         // D K of the plate blocks
constexpr int64_t MIX_MAX_ELEMS = (int64_t)1 << 21;

struct MixArgs {
    int kind, nodes, per_element, K;
    int64_t rows, cols, rs, cs;
    int64_t nbt;                    // workgroups of the table
    const double *prior, *prior_b, *stat, *cnt;
    double *par, *mom;
    const double *prior_r, *Nk;
    double *alpha_r, *elog_r;
    double mult, scale;
    double *ws, *bound;
    unsigned int *ticket;
};

inline int64_t mix_table_blocks(int kind, int64_t rows, int64_t cols)
{
    if (kind == 0 && cols > VMP_TABLE_THREAD_COLS) return rows;
    return (rows + NT - 1) / NT;
}

__device__ __forceinline__ double mix_gamma_element(const MixArgs &a, int64_t e)
{
    const double a0 = a.prior[e], b0 = a.prior_b[e];
    const bool stats = a.stat && a.cnt;
    const double ms = stats ? a.mult * a.stat[e] : 0.0;
    const double mc = stats ? a.mult * (a.per_element ? a.cnt[e] : a.cnt[e % a.K]) : 0.0;
    double *par = a.par + 2 * e, *mom = a.mom + 2 * e;
    if (a.scale == 1.0)             // the optimum itself; the old parameters are not read
        return vmp_pmm_lam_state(a0, b0, a0 + ms, b0 + mc, ms, mc, par, mom);
    const double ao = par[0], bo = par[1];
    const double an = ao + a.scale * ((a0 + ms) - ao), bn = bo + a.scale * ((b0 + mc) - bo);
    return vmp_pmm_lam_state(a0, b0, an, bn, an - a0, bn - b0, par, mom);
}

__global__ void __launch_bounds__(NT) mix_natural_step_kernel(MixArgs a)
{
    __shared__ double red[NT / 64];
    __shared__ unsigned int drawn;
    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x;
    if (blk < a.nbt) {
        double L;
        if (a.kind == 0 && a.cols > VMP_TABLE_THREAD_COLS) {
            L = vmp_dirichlet_row_block<true, NT>(blk, a.cols, a.rs, a.cs, a.prior, a.stat, a.mult,
                                                  a.scale, a.par, a.mom, red);
        } else {
            const int64_t r = blk * NT + tid;
            L = 0.0;
            if (r < a.rows)
                L = a.kind == 0 ? vmp_dirichlet_row_thread<true>(r, (int)a.cols, a.rs, a.cs, a.prior,
                                                                 a.stat, a.mult, a.scale, a.par,
                                                                 a.mom)
                                : mix_gamma_element(a, r);
            L = block_sum<NT>(L, red);
        }
        if (tid == 0) a.ws[blk] = L;
    } else if (tid == 0) {
        // the weights: one Dirichlet row of K <= 64 contiguous columns
        a.bound[1] = vmp_dirichlet_row_thread<true>(0, a.K, a.K, 1, a.prior_r, a.Nk, a.mult,
                                                    a.scale, a.alpha_r, a.elog_r);
    }
    // the ticket: drain this workgroup's stores, release, draw; the last one acquires
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        drawn = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (drawn != gridDim.x - 1) return;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    if (!(a.nodes & 1)) return;
    // thread t adds the partials t, t + NT, ... in ascending order; then the fixed-order sum of the
    // workgroup.  The partials were written by other workgroups: read at agent scope.
    double v = 0.0;
    for (int64_t i = tid; i < a.nbt; i += NT)
        v += __hip_atomic_load(a.ws + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v = block_sum<NT>(v, red);
    if (tid == 0) a.bound[0] = v;
}

}  // namespace

extern "C" {

int32_t vmp_mix_natural_step_workspace(int32_t kind, int64_t rows, int64_t cols, int32_t K,
                                       int64_t *workspace_doubles)
{
    (void)K;
    if ((kind != 0 && kind != 1) || rows < 0 || cols < 1 || !workspace_doubles)
        return VMP_ERR_INVALID;
    const int64_t nb = mix_table_blocks(kind, rows, cols);
    *workspace_doubles = nb + 1;        // the partials and the ticket word
    return VMP_OK;
}

int32_t vmp_mix_natural_step(vmp_ctx *ctx, int32_t kind, int32_t nodes, int64_t rows, int64_t cols,
                             int64_t row_stride, int64_t col_stride, const double *prior,
                             const double *prior_b, const double *stat, const double *cnt,
                             int32_t per_element, double *par, double *mom, int32_t K,
                             const double *prior_r, const double *Nk, double *alpha_r,
                             double *elog_r, double mult, double scale, double *ws, double *bound)
{
    VMP_REQUIRE(ctx, ctx && (kind == 0 || kind == 1) && nodes >= 1 && nodes <= 3,
                VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, mult > 0.0 && scale == scale && mult == mult, VMP_ERR_INVALID,
                "mult must be positive, scale a number");
    VMP_REQUIRE(ctx, bound && ws, VMP_ERR_INVALID, "null argument");
    const bool table = (nodes & 1) != 0, weights = (nodes & 2) != 0;
    if (table) {
        VMP_REQUIRE(ctx, rows >= 0 && cols >= 1 && (per_element == 0 || per_element == 1),
                    VMP_ERR_INVALID, "bad arguments");
        if (kind == 0)
            VMP_REQUIRE(ctx, row_stride >= 1 && col_stride >= 1, VMP_ERR_INVALID, "bad strides");
        else
            VMP_REQUIRE(ctx, K >= 1 && (stat == nullptr) == (cnt == nullptr), VMP_ERR_INVALID,
                        "bad arguments");
        VMP_REQUIRE(ctx, rows == 0 || (prior && par && mom && (kind == 0 || prior_b)),
                    VMP_ERR_INVALID, "null argument");
    }
    if (weights) {
        VMP_REQUIRE(ctx, K >= 1, VMP_ERR_INVALID, "bad arguments");
        VMP_REQUIRE(ctx, prior_r && alpha_r && elog_r, VMP_ERR_INVALID, "null argument");
    }
    if (weights || (table && kind == 1))
        VMP_REQUIRE(ctx, K <= MIX_MAX_K, VMP_ERR_UNSUPPORTED, "K = %d above %d", K, MIX_MAX_K);
    if (table) {
        const bool fits = kind == 0 ? (cols <= MIX_MAX_COLS && rows <= MIX_MAX_ROWS
                                       && rows * cols <= MIX_MAX_ELEMS)
                                    : (cols == 2 && rows <= MIX_MAX_ROWS
                                       && (per_element || rows % K == 0));
        VMP_REQUIRE(ctx, fits, VMP_ERR_UNSUPPORTED,
                    "a table of %lld x %lld is beyond the mixture blocks", (long long)rows,
                    (long long)cols);
    }
    VMP_FLUSH_SMALL(ctx);
    MixArgs a;
    a.kind = kind;
    a.nodes = nodes;
    a.per_element = per_element;
    a.K = K;
    a.rows = table ? rows : 0;
    a.cols = cols;
    a.rs = row_stride;
    a.cs = col_stride;
    a.nbt = table ? mix_table_blocks(kind, rows, cols) : 0;
    a.prior = prior;
    a.prior_b = prior_b;
    a.stat = stat;
    a.cnt = cnt;
    a.par = par;
    a.mom = mom;
    a.prior_r = prior_r;
    a.Nk = Nk;
    a.alpha_r = alpha_r;
    a.elog_r = elog_r;
    a.mult = mult;
    a.scale = scale;
    a.ws = ws;
    a.bound = bound;
    a.ticket = reinterpret_cast<unsigned int *>(ws + a.nbt);
    const int64_t grid = a.nbt + (weights ? 1 : 0);
    if (grid == 0) {                // a table of no rows and nothing else: its bound term is zero
        VMP_HIP_CHECK(ctx, hipMemsetAsync(bound, 0, sizeof(double), ctx->stream));
        return VMP_OK;
    }
    VMP_HIP_CHECK(ctx, hipMemsetAsync(a.ticket, 0, sizeof(double), ctx->stream));
    hipLaunchKernelGGL(mix_natural_step_kernel, dim3((unsigned)grid), dim3(NT), 0, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
