// vmp_dgmm_svi.hip -- the global half of a stochastic-VI step of the two diagonal-Gaussian-mixture
// blocks (bayespy/demos/stochastic_inference.py on plans/dgmm.py and plans/dgmm_masked.py)
//
// A mini-batch of N rows stands for mult times as many.  After the pass over the batch the means, the
// precisions and the Dirichlet row of the mixing weights move along their natural gradients
// (vmp.py:432-440), every optimum from the state at entry:
//
//     phi <- phi + scale (phi* - phi)
//
// mu and tau are two tables, but element e = d K + k of the one couples only with element e of the
// other (vmp_dgmm_svi_dev.h): a thread owns element e of BOTH, reads the old moments and parameters
// of both into registers, forms both optima and stores both.  The weights row is one more
// workgroup, whose thread 0 owns the row (vmp_dirichlet_row_thread, as in vmp_mix_svi.hip); it
// reads N_k, which nobody writes.  So the whole step is ONE launch.
//
// No floating-point atomics.  A thread leaves the bound terms of its element in `ws` (the terms of
// mu, then those of tau); every workgroup draws a ticket, and the one that draws the last adds them
// by the rule of vmp_dgmm_dev.h: element e belongs to thread e % 256, which adds its elements in
// ascending order, and the 256 sums are halved eight times -- the order of vmp_dgmm_update, whose
// bound term mult = scale = 1 therefore leaves bit for bit.  The ticket word stands behind the
// terms in `ws` and is cleared on the stream ahead of the launch.  Nobody waits for anybody.  The
// grid is a function of (D, K, nodes), so the bits of every output depend on the inputs and the
// shape only.
#include "vmp_common.h"
#include "vmp_table_dev.h"
#include "vmp_dgmm_svi_dev.h"

namespace {

constexpr int NT = VMP_DGMM_NT;

struct DgmmSviArgs {
    int D, K, nodes, per_element;
    int64_t DK;
    int64_t nbt;                    // workgroups of the tables
    const double *m0, *beta0, *a0, *b0;
    const double *S1, *S2, *cnt;
    double *mu_par, *mu_mom, *tau_par, *tau_mom;
    const double *prior_r, *Nk;
    double *alpha_r, *elog_r;
    double mult, scale;
    double *ws, *bound;
    unsigned int *ticket;
};

// the terms ws[0 .. n) in the order of dgmm_update_kernel; they were written by other workgroups:
// read at agent scope
__device__ __forceinline__ double svi_bound_sum(const double *ws, int64_t n, double *bs, int tid)
{
    double t = 0.0;
    for (int64_t e = tid; e < n; e += NT)
        t += __hip_atomic_load(ws + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    bs[tid] = t;
    __syncthreads();
    block_halve_sum<NT>(bs, tid);
    return bs[0];
}

__global__ void __launch_bounds__(NT) dgmm_natural_step_kernel(DgmmSviArgs a)
{
    __shared__ double bs[NT];
    __shared__ unsigned int drawn;
    const int tid = threadIdx.x;
    const int64_t blk = blockIdx.x;
    if (blk < a.nbt) {
        const int64_t e = blk * NT + tid;
        if (e < a.DK) {
            const int stats = a.S1 && a.S2 && a.cnt;
            const double s1 = stats ? a.S1[e] : 0.0, s2 = stats ? a.S2[e] : 0.0;
            const double cnt = stats ? (a.per_element ? a.cnt[e] : a.cnt[e % a.K]) : 0.0;
            double Lmu = 0.0, Ltau = 0.0;
            vmp_dgmm_svi_element(a.nodes, a.per_element, stats, a.m0[e], a.beta0[e], a.a0[e],
                                 a.b0[e], s1, s2, cnt, a.mult, a.scale, a.mu_par + 2 * e,
                                 a.mu_mom + 2 * e, a.tau_par + 2 * e, a.tau_mom + 2 * e, &Lmu,
                                 &Ltau);
            if (a.nodes & VMP_DGMM_SVI_MU) a.ws[e] = Lmu;
            if (a.nodes & VMP_DGMM_SVI_TAU) a.ws[a.DK + e] = Ltau;
        }
    } else if (tid == 0) {
        // the weights: one Dirichlet row of K <= 64 contiguous columns
        a.bound[2] = vmp_dirichlet_row_thread<true>(0, a.K, a.K, 1, a.prior_r, a.Nk, a.mult,
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
    if (a.nodes & VMP_DGMM_SVI_MU) {
        const double v = svi_bound_sum(a.ws, a.DK, bs, tid);
        if (tid == 0) a.bound[0] = v;
    }
    if (a.nodes & VMP_DGMM_SVI_TAU) {
        const double v = svi_bound_sum(a.ws + a.DK, a.DK, bs, tid);
        if (tid == 0) a.bound[1] = v;
    }
}

}  // namespace

extern "C" {

int32_t vmp_dgmm_natural_step_workspace(int32_t D, int32_t K, int64_t *workspace_doubles)
{
    if (D < 1 || K < 1 || !workspace_doubles) return VMP_ERR_INVALID;
    if (K > VMP_DGMM_MAX_K || D > VMP_DGMM_MAX_D) return VMP_ERR_UNSUPPORTED;
    *workspace_doubles = 2 * (int64_t)D * K + 1;    // the terms of mu, of tau, the ticket word
    return VMP_OK;
}

int32_t vmp_dgmm_natural_step(vmp_ctx *ctx, int32_t D, int32_t K, int32_t nodes, const double *m0,
                              const double *beta0, const double *a0, const double *b0,
                              const double *S1, const double *S2, const double *cnt,
                              int32_t per_element, double *mu_par, double *mu_mom, double *tau_par,
                              double *tau_mom, const double *prior_r, const double *Nk,
                              double *alpha_r, double *elog_r, double mult, double scale, double *ws,
                              double *bound)
{
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1 && nodes >= 1 && nodes <= 7
                && (per_element == 0 || per_element == 1), VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, mult > 0.0 && scale == scale && mult == mult, VMP_ERR_INVALID,
                "mult must be positive, scale a number");
    int32_t max_k, max_d;
    vmp_dgmm_limits(&max_k, &max_d);
    VMP_REQUIRE(ctx, K <= max_k && D <= max_d, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, max_d, max_k);
    VMP_REQUIRE(ctx, bound && ws, VMP_ERR_INVALID, "null argument");
    const bool tables = (nodes & (VMP_DGMM_SVI_MU | VMP_DGMM_SVI_TAU)) != 0;
    const bool weights = (nodes & VMP_DGMM_SVI_WEIGHTS) != 0;
    if (tables) {
        VMP_REQUIRE(ctx, (S1 == nullptr) == (S2 == nullptr) && (S1 == nullptr) == (cnt == nullptr),
                    VMP_ERR_INVALID, "the statistics are given together or not at all");
        VMP_REQUIRE(ctx, mu_par && mu_mom && tau_par && tau_mom, VMP_ERR_INVALID, "null argument");
        if (nodes & VMP_DGMM_SVI_MU)
            VMP_REQUIRE(ctx, m0 && beta0, VMP_ERR_INVALID, "null argument");
        if (nodes & VMP_DGMM_SVI_TAU)
            VMP_REQUIRE(ctx, a0 && b0, VMP_ERR_INVALID, "null argument");
    }
    if (weights)
        VMP_REQUIRE(ctx, prior_r && alpha_r && elog_r, VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    DgmmSviArgs a;
    a.D = D;
    a.K = K;
    a.nodes = nodes;
    a.per_element = per_element;
    a.DK = (int64_t)D * K;
    a.nbt = tables ? (a.DK + NT - 1) / NT : 0;
    // the priors of a node that is not named are not looked at
    a.m0 = m0 ? m0 : a0;
    a.beta0 = beta0 ? beta0 : b0;
    a.a0 = a0 ? a0 : m0;
    a.b0 = b0 ? b0 : beta0;
    a.S1 = S1;
    a.S2 = S2;
    a.cnt = cnt;
    a.mu_par = mu_par;
    a.mu_mom = mu_mom;
    a.tau_par = tau_par;
    a.tau_mom = tau_mom;
    a.prior_r = prior_r;
    a.Nk = Nk;
    a.alpha_r = alpha_r;
    a.elog_r = elog_r;
    a.mult = mult;
    a.scale = scale;
    a.ws = ws;
    a.bound = bound;
    a.ticket = reinterpret_cast<unsigned int *>(ws + 2 * a.DK);
    const int64_t grid = a.nbt + (weights ? 1 : 0);
    VMP_HIP_CHECK(ctx, hipMemsetAsync(a.ticket, 0, sizeof(double), ctx->stream));
    hipLaunchKernelGGL(dgmm_natural_step_kernel, dim3((unsigned)grid), dim3(NT), 0, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
