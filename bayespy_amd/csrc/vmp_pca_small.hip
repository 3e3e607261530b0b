// vmp_pca_small.hip -- replicated-node updates of the fused PCA block (gfx950).
//
// W.update(), the replicated half of X.update(), tau.update(), alpha.update() and the
// lower bound work on K x K / D x K state only.  They are latency-, not throughput-bound,
// and at shard sizes of a million columns they decide the step time.  So the sequences a VB
// iteration produces -- (W, X-replicated) and (tau, alpha, lower bound) -- are ONE launch
// each: a single 256-thread workgroup runs the operations back to back (no launch gaps,
// state re-read from L2 by the same CU), small enough (< 64 KB LDS, one wavefront per SIMD)
// to run beside the streaming grid of vmp_pca_xpass, i.e. concurrently with the plate pass
// of the previous iteration.
//
// Reference formulas: gaussian.py:649-706 (GaussianARD phi / moments / cgf),
// dot.py:581 (message E4), gaussian.py:2344-2369 (WrapToGaussianGamma), gamma.py:116-160,
// expfamily.py:400-480 (lower bound), utils/linalg.py:31-223 (chol, chol_inv, chol_logdet).
#include "vmp_common.h"
#include "vmp_sweep.h"
#include "vmp_stop_rule.h"

#include <stdlib.h>
#include <string.h>
#include <type_traits>

namespace {


struct small_args {
    vmp_pca_layout L;
    int D, K;
    double n_total, x_prec, a0t, b0t, a0a, b0a;
    int has_mean;       // W has a constant non-zero prior mean mu (state[off_mu]); see op_update_w
};

// sum_d <(w_dk - mu_dk)^2> = Sww_kk - 2 sum_d mu_dk <w_dk> + sum_d mu_dk^2: what the Gamma message
// of the ARD prior (gaussian.py:2344-2369) and the bound term of W see of a non-zero prior mean;
// the two sums are kept in state[off_mstat] by op_update_w
__device__ inline double ww_centred(const small_args &a, const double *st, int k)
{
    const vmp_pca_layout &L = a.L;
    double v = st[L.off_Sww + k * L.KP + k];
    if (a.has_mean) v += st[L.off_mstat + L.KP + k] - 2.0 * st[L.off_mstat + k];
    return v;
}

// <x x^T> total statistic: n_total * Cov_X + sum_n <x><x>^T, symmetrised.
__device__ inline double sxx_total(const double *st, const vmp_pca_layout &L, double n_total,
                                   int i, int j)
{
    const double *S = st + L.off_S;
    const double m = 0.5 * (S[(L.DP + i) * L.KP + j] + S[(L.DP + j) * L.KP + i]);
    return n_total * st[L.off_CX + i * L.KP + j] + m;
}

// One shared copy of each special function (the fused kernels are instruction-fetch
// sensitive when they run beside the streaming pass: 21 KB of inlined code took longer to
// fetch than to execute).
__device__ __noinline__ double sf_lgamma(double x) { return vmp_lgamma(x); }
__device__ __noinline__ double sf_digamma(double x) { return vmp_digamma(x); }
__device__ __noinline__ double sf_log(double x) { return log(x); }

// In-place inverse of the SPD matrix in M (KP x (KP+1) in LDS, entries beyond n x n hold
// the identity) by pivot-free Gauss-Jordan sweeps, all KP^2 elements updated in parallel
// per pivot.  Replaces chol / chol_inv / chol_logdet (utils/linalg.py:31-63, :174-223).
template <int KP, int NTQ>
__device__ void gj_inverse(double *M, int n, double *logdet, int *bad)
{
    constexpr int LDM = KP + 1;
    constexpr int E = KP * KP / NTQ;
    const int tid = threadIdx.x;
    double ld = 0.0, prod = 1.0;
    int isbad = 0;
#pragma unroll 1
    for (int p = 0; p < n; ++p) {
        __syncthreads();
        const double piv = M[p * LDM + p];
        double ci[E], rj[E], me[E];
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTQ;
            const int i = e / KP, j = e % KP;
            ci[m] = M[i * LDM + p];
            rj[m] = M[p * LDM + j];
            me[m] = M[i * LDM + j];
        }
        if (!(piv > 0.0)) isbad = 1;
        // running log-determinant: fold the pivot product only when it leaves a safe range
        prod *= piv;
        if (!(prod < 1e120 && prod > 1e-120)) {
            ld += sf_log(prod);
            prod = 1.0;
        }
        const double d = fast_recip(piv);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTQ;
            const int i = e / KP, j = e % KP;
            double v;
            if (i == p) v = (j == p) ? d : rj[m] * d;
            else if (j == p) v = -ci[m] * d;
            else v = me[m] - ci[m] * rj[m] * d;
            M[i * LDM + j] = v;
        }
    }
    __syncthreads();
    if (tid == 0) {
        *logdet = ld + sf_log(prod);
        if (isbad) *bad = 1;
    }
    __syncthreads();
}

// The same inverse for KP <= 32 by ONE wavefront in registers (vmp_sweep.h: symmetric sweep with
// 4 x 4 pivot blocks on the matrix cores): no LDS traffic and no barriers between the pivots.
// gj_inverse above takes 2 barriers and 16 LDS accesses per pivot -- 14 of the 41 us of the fused
// W / X-prepare kernel per inverse when it runs alone, and 70+ us each beside the streaming grid of
// the plate pass, whose wavefronts keep the CU's LDS pipeline busy (measured with wall_clock64
// stamps at N = 1.25e6, the shard one of 8 ranks holds at the headline size).
// `side` is what wavefronts 1 .. 3 do meanwhile, between the two barriers.  Only pca_head_wide passes
// one.  The default, no_side, is empty, so that instantiation -- the one pca_head_body, the tails and
// every kernel that runs beside the pass use -- is the code from before the parameter existed (its
// kernels' register and LDS figures are unchanged).
struct no_side {
    __device__ __forceinline__ void operator()() const {}
};
template <int KP, class SIDE = no_side>
__device__ __forceinline__ void sweep_inverse(double *M, int n, double *logdet, int *bad,
                                              const SIDE &side = SIDE())
{
    static_assert(KP == 16 || KP == 32, "one 32 x 32 register tile set");
    constexpr int LDM = KP + 1;
    __syncthreads();
    if (threadIdx.x < 64) {
        const int l = threadIdx.x, l15 = l & 15, l4 = l >> 4;
        v4f64 T[2][2];
#pragma unroll
        for (int tr = 0; tr < 2; ++tr)
#pragma unroll
            for (int tc = 0; tc < 2; ++tc)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * tr + l4 + 4 * r, col = 16 * tc + l15;
                    T[tr][tc][r] = (row < KP && col < KP) ? M[row * LDM + col]
                                                          : (row == col ? 1.0 : 0.0);
                }
        double prod = 1.0, ld = 0.0;
        int isbad = 0;
        vmp_sweep::sweep_upto<0>(T, (n + 3) / 4, l15, l4, prod, ld, isbad);
#pragma unroll
        for (int tr = 0; tr < KP / 16; ++tr)
#pragma unroll
            for (int tc = 0; tc < KP / 16; ++tc)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * tr + l4 + 4 * r, col = 16 * tc + l15;
                    // rows / columns beyond n were not swept: they keep the identity
                    M[row * LDM + col] = (row < 4 * ((n + 3) / 4) && col < 4 * ((n + 3) / 4))
                                             ? -T[tr][tc][r] : T[tr][tc][r];
                }
        if (l == 0) {
            *logdet = vmp_sweep::sweep_logdet(prod, ld);
            if (isbad) *bad = 1;
        }
    } else {
        side();
    }
    __syncthreads();
}

// wall_clock64 stamps of the one-launch sweep (tune key "pca_sweep_stamps", tools/sweep_stamps.py):
// thread 0 keeps them in LDS and the workgroup that runs phase B copies them out at its end.  The
// default kernels are instantiated with stamps_off, which is empty.
enum { SP_ENTRY = 0, SP_LDS_FILLED, SP_SYX, SP_PXX, SP_TICKET, SP_ACQUIRE,
       SP_T_PARTIALS, SP_T_LOADS, SP_T_PXX, SP_T_BLOCKSUMS, SP_T_TAU_ALPHA, SP_T_BOUND, SP_T_RING,
       SP_H_LAMBDA, SP_H_INV1, SP_H_W, SP_H_SWW, SP_H_INV2, SP_H_A, SP_COUNT,
       // "pca_sweep_stamps" = 2: where the side wavefront stands (free words of the row)
       SP_S_STATE = SP_COUNT, SP_S_RING, SP_COUNT2 };
static_assert(SP_COUNT2 <= VMP_SWEEP_NSTAMP, "stamp row length");
struct stamps_off {
    __device__ __forceinline__ void operator()(int) const {}
    __device__ __forceinline__ void side(int) const {}
    __device__ __forceinline__ void drain() const {}
};
struct stamps_on {
    unsigned long long *t;      // LDS, VMP_SWEEP_NSTAMP words
    int level;                  // the value of "pca_sweep_stamps"
    __device__ __forceinline__ void operator()(int i) const
    {
        if (threadIdx.x == 0) t[i] = wall_clock64();
    }
    // a stamp of the side wavefront (its first lane), recorded at level 2 only
    __device__ __forceinline__ void side(int i) const
    {
        if (level >= 2 && threadIdx.x == 64) t[i] = wall_clock64();
    }
    // before a stamp that stands for "stored": the thread's stores have left
    __device__ __forceinline__ void drain() const { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

template <int KP, int NTQ>
struct small_lds {
    static constexpr int LDM = KP + 1;
    static constexpr int RB = (KP == 64) ? 16 : 32;   // row block of the D x K products
    double M[KP * LDM];
    double Sb[RB * LDM];
    double Wb[RB * LDM];
    double red[NTQ / 64 + 1];
    double logdet;
    int bad;
};

// W.update(): Lambda_W = diag<alpha> + <tau> Sxx ; Cov_W ; <W> = <tau> Syx Cov_W ;
// Sww = D Cov_W + W^T W.
template <int KP, int NTQ>
__device__ void op_update_w(const small_args &a, double *st, small_lds<KP, NTQ> &s)
{
    constexpr int LDM = KP + 1, RB = small_lds<KP, NTQ>::RB, E = KP * KP / NTQ;
    const vmp_pca_layout &L = a.L;
    const int tid = threadIdx.x, D = a.D, K = a.K;
    const double tau = st[L.off_tau + 2];
    // gaussian.py:656-670 (prior phi) + dot.py:581 (message E4)
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTQ;
        const int i = e / KP, j = e % KP;
        double v = (i == j) ? 1.0 : 0.0;
        if (i < K && j < K) {
            v = tau * sxx_total(st, L, a.n_total, i, j);
            if (i == j) v += st[L.off_alpha + 2 * KP + i];
        }
        s.M[i * LDM + j] = v;
    }
    gj_inverse<KP, NTQ>(s.M, K, &s.logdet, &s.bad);
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTQ;
        const int i = e / KP, j = e % KP;
        if (i < K && j < K) st[L.off_CW + i * KP + j] = s.M[i * LDM + j];
    }
    const double *Syx = st + L.off_S;
    double *W = st + L.off_W;
    double sw[E];
#pragma unroll
    for (int m = 0; m < E; ++m) sw[m] = 0.0;
    for (int r0 = 0; r0 < D; r0 += RB) {
        const int nr = (D - r0) < RB ? (D - r0) : RB;
        __syncthreads();
#pragma unroll 1
        for (int e = tid; e < RB * KP; e += NTQ) {
            const int r = e / KP, k = e % KP;
            double v = (r < nr && k < K) ? Syx[(r0 + r) * KP + k] : 0.0;
            // a non-zero prior mean: phi0_d = <tau> Syx[d] + <alpha> * mu_d (gaussian.py:656-670)
            if (a.has_mean && r < nr && k < K)
                v = tau * v + st[L.off_alpha + 2 * KP + k] * st[L.off_mu + (r0 + r) * KP + k];
            s.Sb[r * LDM + k] = v;
        }
        __syncthreads();
        // <w_d> = Cov_W phi0_d,  phi0_d = <tau> Syx[d]        (gaussian.py:694)
#pragma unroll 1
        for (int e = tid; e < RB * KP; e += NTQ) {
            const int r = e / KP, k = e % KP;
            double acc = 0.0;
            if (k < K)
#pragma unroll 4
                for (int j = 0; j < K; ++j) acc += s.Sb[r * LDM + j] * s.M[j * LDM + k];
            if (!a.has_mean) acc *= tau;
            s.Wb[r * LDM + k] = acc;
            if (r < nr && k < K) W[(r0 + r) * KP + k] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTQ;
            const int i = e / KP, j = e % KP;
            double acc = 0.0;
#pragma unroll 4
            for (int r = 0; r < RB; ++r) acc += s.Wb[r * LDM + i] * s.Wb[r * LDM + j];
            sw[m] += acc;
        }
    }
    // Sww = sum_d <w_d w_d^T> = D Cov_W + W^T W                (gaussian.py:695)
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTQ;
        const int i = e / KP, j = e % KP;
        if (i < K && j < K)
            st[L.off_Sww + i * KP + j] = (double)D * s.M[i * LDM + j] + sw[m];
    }
    if (tid == 0) st[L.off_scal + 0] = s.logdet;
    if (a.has_mean) {
        // sum_d mu_dk <w_dk> and sum_d mu_dk^2 for the Gamma message and the bound term of W
        __threadfence_block();
        __syncthreads();
        for (int k = tid; k < K; k += NTQ) {
            double m1 = 0.0, m2 = 0.0;
            for (int d = 0; d < D; ++d) {
                const double mu = st[L.off_mu + d * KP + k];
                m1 += mu * W[d * KP + k];
                m2 += mu * mu;
            }
            st[L.off_mstat + k] = m1;
            st[L.off_mstat + KP + k] = m2;
        }
    }
}

// X.update(), replicated half: Lambda_X = x_prec I + <tau> Sww ; Cov_X ; A = <tau> Cov_X W^T.
template <int KP, int NTQ>
__device__ void op_prepare_x(const small_args &a, double *st, small_lds<KP, NTQ> &s)
{
    constexpr int LDM = KP + 1, RB = small_lds<KP, NTQ>::RB, E = KP * KP / NTQ;
    const vmp_pca_layout &L = a.L;
    const int tid = threadIdx.x, D = a.D, K = a.K;
    const int DP = (int)L.DP;
    const double tau = st[L.off_tau + 2];
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTQ;
        const int i = e / KP, j = e % KP;
        double v = (i == j) ? 1.0 : 0.0;
        if (i < K && j < K) {
            v = tau * 0.5 * (st[L.off_Sww + i * KP + j] + st[L.off_Sww + j * KP + i]);
            if (i == j) v += a.x_prec;
        }
        s.M[i * LDM + j] = v;
    }
    gj_inverse<KP, NTQ>(s.M, K, &s.logdet, &s.bad);
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTQ;
        const int i = e / KP, j = e % KP;
        if (i < K && j < K) st[L.off_CX + i * KP + j] = s.M[i * LDM + j];
    }
    const double *W = st + L.off_W;
    for (int r0 = 0; r0 < D; r0 += RB) {
        const int nr = (D - r0) < RB ? (D - r0) : RB;
        __syncthreads();
#pragma unroll 1
        for (int e = tid; e < RB * KP; e += NTQ) {
            const int r = e / KP, k = e % KP;
            s.Wb[r * LDM + k] = (r < nr && k < K) ? W[(r0 + r) * KP + k] : 0.0;
        }
        __syncthreads();
        // A[k][d] = <tau> sum_j Cov_X[k][j] W[d][j]; r fastest => coalesced stores
#pragma unroll 1
        for (int e = tid; e < RB * KP; e += NTQ) {
            const int k = e / RB, r = e % RB;
            if (k < K && r < nr) {
                double acc = 0.0;
#pragma unroll 4
                for (int j = 0; j < K; ++j) acc += s.M[k * LDM + j] * s.Wb[r * LDM + j];
                st[L.off_A + (int64_t)k * DP + r0 + r] = tau * acc;
            }
        }
    }
    if (tid == 0) st[L.off_scal + 1] = s.logdet;
}

// sum_dn <(y_dn - f_dn)^2> = Syy - 2 sum(W o Syx) + sum(Sww o Sxx)
// (dot.py:355 E1 and dot.py:403 E2 collapsed to traces).
template <int NTQ>
__device__ double pca_residual(const small_args &a, const double *st, double *red)
{
    const vmp_pca_layout &L = a.L;
    const int tid = threadIdx.x, D = a.D, K = a.K;
    const int KP = (int)L.KP;
    double t1 = 0.0, t2 = 0.0;
    // padded entries of W are zero, so the D x KP blocks can be walked linearly
#pragma unroll 4
    for (int e = tid; e < D * KP; e += NTQ) t1 += st[L.off_W + e] * st[L.off_S + e];
    for (int e = tid; e < K * K; e += NTQ) {
        const int i = e / K, j = e - i * K;
        t2 += st[L.off_Sww + i * KP + j] * sxx_total(st, L, a.n_total, i, j);
    }
    t1 = block_sum<NTQ>(t1, red);
    t2 = block_sum<NTQ>(t2, red);
    return st[L.off_Syy] - 2.0 * t1 + t2;
}

template <int NTQ>
__device__ void op_update_tau(const small_args &a, double *st, double *red)
{
    const vmp_pca_layout &L = a.L;
    const double resid = pca_residual<NTQ>(a, st, red);
    if (threadIdx.x == 0) {
        // gamma.py:116-122 phi = [-b, a] with the message gaussian.py:2363-2369
        const double al = a.a0t + 0.5 * (double)a.D * a.n_total;
        const double be = a.b0t + 0.5 * resid;
        st[L.off_tau + 0] = al;
        st[L.off_tau + 1] = be;
        st[L.off_tau + 2] = al / be;                       // gamma.py:144
        st[L.off_tau + 3] = sf_digamma(al) - sf_log(be);     // gamma.py:145
        st[L.off_scal + 2] = resid;
        if (!(be > 0.0)) st[L.off_scal + 3] = (double)VMP_ERR_FLOATING;
    }
}

template <int NTQ>
__device__ void op_update_alpha(const small_args &a, double *st)
{
    const vmp_pca_layout &L = a.L;
    const int KP = (int)L.KP;
    for (int k = threadIdx.x; k < a.K; k += NTQ) {
        const double al = a.a0a + 0.5 * (double)a.D;
        const double be = a.b0a + 0.5 * ww_centred(a, st, k);
        st[L.off_alpha + 0 * KP + k] = al;
        st[L.off_alpha + 1 * KP + k] = be;
        st[L.off_alpha + 2 * KP + k] = al / be;
        st[L.off_alpha + 3 * KP + k] = sf_digamma(al) - sf_log(be);
    }
}

// E[log p - log q] of a Gamma(a,b) node with prior Gamma(a0,b0)
// (expfamily.py:400-480 with gamma.py:147,160).
__device__ inline double gamma_elbo(double a0, double b0, double a, double b, double x,
                                    double logx)
{
    const double g_p = a0 * sf_log(b0) - sf_lgamma(a0);
    const double g_q = a * sf_log(b) - sf_lgamma(a);
    return g_p - g_q + (b - b0) * x + (a0 - a) * logx;
}

template <int NTQ>
__device__ void op_lower_bound(const small_args &a, double *st, double *red)
{
    const vmp_pca_layout &L = a.L;
    const int tid = threadIdx.x, D = a.D, K = a.K;
    const int KP = (int)L.KP;
    const double resid = pca_residual<NTQ>(a, st, red);
    double trx = 0.0, sla = 0.0, saw = 0.0, lal = 0.0;
    // index K stands for the tau node: every Gamma term goes through one copy of the
    // special-function code (register pressure)
#pragma unroll 1
    for (int k = tid; k <= K; k += NTQ) {
        const bool is_tau = (k == K);
        const int64_t oa = is_tau ? L.off_tau : L.off_alpha + k;
        const int64_t sa = is_tau ? 1 : KP;
        const double al = st[oa], be = st[oa + sa], x = st[oa + 2 * sa], lx = st[oa + 3 * sa];
        const double g = gamma_elbo(is_tau ? a.a0t : a.a0a, is_tau ? a.b0t : a.b0a, al, be, x, lx);
        if (is_tau) {
            red[NTQ / 64] = g;
        } else {
            trx += sxx_total(st, L, a.n_total, k, k);
            sla += lx;
            saw += x * ww_centred(a, st, k);
            lal += g;
        }
    }
    trx = block_sum<NTQ>(trx, red);
    sla = block_sum<NTQ>(sla, red);
    saw = block_sum<NTQ>(saw, red);
    lal = block_sum<NTQ>(lal, red);
    if (tid == 0) {
        const double tau = st[L.off_tau + 2], logtau = st[L.off_tau + 3];
        const double Dd = (double)D, Kd = (double)K;
        const double LY = Dd * a.n_total * (-0.5 * sf_log(2.0 * M_PI) + 0.5 * logtau)
                          - 0.5 * tau * resid;
        const double LX = -0.5 * a.x_prec * trx
                          + a.n_total * (0.5 * Kd * sf_log(a.x_prec) - 0.5 * st[L.off_scal + 1]
                                         + 0.5 * Kd);
        const double LW = 0.5 * Dd * sla - 0.5 * saw + Dd * (-0.5 * st[L.off_scal + 0] + 0.5 * Kd);
        const double Lt = red[NTQ / 64];
        st[L.off_L + 0] = LY;
        st[L.off_L + 1] = LX;
        st[L.off_L + 2] = LW;
        st[L.off_L + 3] = Lt;
        st[L.off_L + 4] = lal;
        st[L.off_L + 5] = LY + LX + LW + Lt + lal;
        st[L.off_scal + 2] = resid;
    }
}

template <int KP, int NTQ, int OP>
__device__ __forceinline__ void run_op(const small_args &a, double *st, small_lds<KP, NTQ> &s)
{
    if constexpr (OP != 0) {
        // the previous operation's global writes are read back by this workgroup only
        __threadfence_block();
        __syncthreads();
    }
    if constexpr (OP == VMP_PCA_OP_W) op_update_w<KP, NTQ>(a, st, s);
    if constexpr (OP == VMP_PCA_OP_XPREP) op_prepare_x<KP, NTQ>(a, st, s);
    if constexpr (OP == VMP_PCA_OP_TAU) op_update_tau<NTQ>(a, st, s.red);
    if constexpr (OP == VMP_PCA_OP_ALPHA) op_update_alpha<NTQ>(a, st);
    if constexpr (OP == VMP_PCA_OP_ELBO) op_lower_bound<NTQ>(a, st, s.red);
}

// The operation sequence is a template parameter: straight-line code keeps the register
// footprint at the maximum over the operations instead of their union.
template <int KP, int NTQ, int O0, int O1, int O2>
__global__ void __launch_bounds__(NTQ)
pca_small_kernel(small_args a, double *st)
{
    __shared__ small_lds<KP, NTQ> s;
    __builtin_amdgcn_s_setprio(3);   // latency-critical: win issue arbitration on a shared CU
    if (threadIdx.x == 0) s.bad = 0;
    run_op<KP, NTQ, O0>(a, st, s);
    run_op<KP, NTQ, O1>(a, st, s);
    run_op<KP, NTQ, O2>(a, st, s);
    __syncthreads();
    if (threadIdx.x == 0 && s.bad) st[a.L.off_scal + 3] = (double)VMP_ERR_NOT_POSDEF;
}

// ---------------------------------------------------------------------------
// LDS-resident forms of the two sequences of a VB iteration, for K <= 32 and D <= 128.
//
// Beside the streaming grid every dependent global access of this workgroup queues behind
// the pass kernel's outstanding loads on the same CU (~10 us per round trip, measured), so
// the generic operations above -- a dozen round trips each -- take 100-200 us there.  These
// kernels fetch their whole working set in one batch, compute from LDS, and store at the end.
// ---------------------------------------------------------------------------
constexpr int FAST_D = 128;
constexpr int NTF = 256;

// the state block is a few hundred KB: 32-bit element offsets keep the index arithmetic
// of these kernels off the 64-bit VALU paths (registers)
struct lay32 {
    int DP, KP, off_S, off_Syy, off_tau, off_alpha, off_W, off_CW, off_Sww, off_CX, off_A,
        off_scal, off_L;
    __device__ explicit lay32(const vmp_pca_layout &l)
        : DP((int)l.DP), KP((int)l.KP), off_S((int)l.off_S), off_Syy((int)l.off_Syy),
          off_tau((int)l.off_tau), off_alpha((int)l.off_alpha), off_W((int)l.off_W),
          off_CW((int)l.off_CW), off_Sww((int)l.off_Sww), off_CX((int)l.off_CX),
          off_A((int)l.off_A), off_scal((int)l.off_scal), off_L((int)l.off_L) {}
};

// One wavefront, one 16 x 16 tile of C = A B from LDS operands with arbitrary strides
// (v_mfma_f64_16x16x4_f64; A(m,k) = As[m*am + k*ak], B(k,n) = Bs[k*bk + n*bn], kc % 4 == 0).
// Result layout: element (row = (lane>>4) + 4*reg, col = lane&15).
__device__ __forceinline__ v4f64 wave_tile_mma(const double *As, int am, int ak, const double *Bs,
                                               int bk, int bn, int kc)
{
    const int l = threadIdx.x & 63, l15 = l & 15, l4 = l >> 4;
    v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
    for (int q = 0; q < kc; q += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[l15 * am + (q + l4) * ak],
                                                   Bs[(q + l4) * bk + l15 * bn], acc, 0, 0, 0);
    return acc;
}

// (W.update(), X.update() replicated half)
// accumulate form of wave_tile_mma
__device__ __forceinline__ v4f64 wave_tile_mma_acc(v4f64 acc, const double *As, int am, int ak,
                                                   const double *Bs, int bk, int bn, int kc)
{
    const int l = threadIdx.x & 63, l15 = l & 15, l4 = l >> 4;
#pragma unroll 4
    for (int q = 0; q < kc; q += 4)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(As[l15 * am + (q + l4) * ak],
                                                   Bs[(q + l4) * bk + l15 * bn], acc, 0, 0, 0);
    return acc;
}

// (W.update(), X.update() replicated half)
//
// Placement beside the plate pass decides this kernel's latency at the multi-GPU shard size, and
// what decides the placement was measured (tools/timeline.sh, tools/experiments/
// placement_microbench.hip): beside three resident pass workgroups per CU (32 KB of
// LDS, 122 VGPRs each) a workgroup asking for 52 KB of LDS is not placed until the persistent grid
// drains, whatever its register count; one asking for 26 KB and <= 96 registers is placed at once.
// So the D x K operand is staged through ONE 32-row block (8.4 KB) instead of a D-row array
// (33.8 KB), the rows of sum y<x>^T are loaded only after the first sweep and the rows of <W> come
// back from global memory for the last product instead of waiting in registers, the inverses are
// inlined (no call, no scratch) and the file is compiled with the VGPR form of the MFMAs (Makefile):
// 25.6 KB, 96 VGPRs, no AGPRs, no scratch.
template <int KP>
__device__ __forceinline__ void pca_head_body(const small_args &a, double *st)
{
    constexpr int LDM = KP + 1, E = KP * KP / NTF, RB = 32;
    __shared__ double M[KP * LDM];          // Lambda_W -> Cov_W -> Lambda_X -> Cov_X
    __shared__ double T[KP * LDM];          // sum <x x^T> (shard sum) -> Sww
    __shared__ double SWb[RB * LDM];        // one row block: Syx rows -> <W> rows
    __shared__ double alm[KP];
    __shared__ double logdet;
    __shared__ int bad;
    constexpr int KT = KP / 16;
    constexpr int NB = FAST_D / RB;               // row blocks
    constexpr int NLB = RB * KP / NTF;            // loads per thread and row block
    constexpr int TPB = 2 * KT;                   // 16 x 16 tiles of a row block
    constexpr int WT = (TPB + 3) / 4;             // ... per wavefront
    constexpr int ST = (KT * KT + 3) / 4;         // tiles of Sww per wavefront
    const lay32 L(a.L);
    int tid = threadIdx.x;
    const int D = a.D, K = a.K;
    const int DP = (int)L.DP;
    const int nb = (D + RB - 1) / RB;
    __builtin_amdgcn_s_setprio(3);   // latency-critical: win issue arbitration on a shared CU
    if (tid == 0) bad = 0;
    // ---- one batch of loads ------------------------------------------------------------
    const double tau = st[L.off_tau + 2];
    {
        double cx[E], sx[E];
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            const int i = e / KP, j = e % KP;
            const bool in = (i < K && j < K);
            cx[m] = in ? st[L.off_CX + i * KP + j] : 0.0;
            sx[m] = in ? st[L.off_S + (L.DP + i) * KP + j] : 0.0;
        }
        if (tid < KP) alm[tid] = tid < K ? st[L.off_alpha + 2 * KP + tid] : 0.0;
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            M[(e / KP) * LDM + (e % KP)] = cx[m];
            T[(e / KP) * LDM + (e % KP)] = sx[m];
        }
    }
    __syncthreads();
    // ---- W: Lambda_W = diag<alpha> + <tau> Sxx  (gaussian.py:656-670, dot.py:581) -------
    {
        double lam[E];
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            const int i = e / KP, j = e % KP;
            double x = (i == j) ? 1.0 : 0.0;
            if (i < K && j < K) {
                x = tau * (a.n_total * M[i * LDM + j] + 0.5 * (T[i * LDM + j] + T[j * LDM + i]));
                if (i == j) x += alm[i];
            }
            lam[m] = x;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            M[(e / KP) * LDM + (e % KP)] = lam[m];
        }
    }
    asm volatile("" : "+v"(tid));     // nothing derived from the thread index stays live across the sweep
    sweep_inverse<KP>(M, K, &logdet, &bad);
    asm volatile("" : "+v"(tid));
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        const int i = e / KP, j = e % KP;
        if (i < K && j < K) st[L.off_CW + i * KP + j] = M[i * LDM + j];
    }
    if (tid == 0) st[L.off_scal + 0] = logdet;
    int w = tid >> 6, l15 = tid & 15, l4 = (tid & 63) >> 4;
    // <w_d> = <tau> Cov_W Syx[d]  (gaussian.py:694), one 32-row block at a time on the matrix cores;
    // Sww = D Cov_W + W^T W  (gaussian.py:695) accumulated over the blocks
    // rows of sum y<x>^T: one batch of loads, issued only now so that they do not occupy registers
    // during the sweep (the kernel must stay within ~90 VGPRs to be placed beside the plate pass)
    double v[NB][NLB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int m = 0; m < NLB; ++m) {
            const int e = tid + m * NTF;
            const int r = b * RB + e / KP, k = e % KP;
            v[b][m] = (r < D && k < K) ? st[L.off_S + r * KP + k] : 0.0;
        }
    v4f64 wt[WT];
    v4f64 sacc[ST];
#pragma unroll
    for (int t = 0; t < ST; ++t) sacc[t] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b < nb) {
#pragma unroll
            for (int m = 0; m < NLB; ++m) {
                const int e = tid + m * NTF;
                SWb[(e / KP) * LDM + (e % KP)] = v[b][m];
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < WT; ++t) {
                const int tile = w + 4 * t;
                if (tile < TPB)
                    wt[t] = wave_tile_mma(SWb + (tile / KT) * 16 * LDM, LDM, 1,
                                             M + (tile % KT) * 16, LDM, 1, KP);
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < WT; ++t) {
                const int tile = w + 4 * t;
                if (tile < TPB) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int lr = (tile / KT) * 16 + l4 + 4 * r, k = (tile % KT) * 16 + l15;
                        const double x = tau * wt[t][r];
                        SWb[lr * LDM + k] = x;
                        const int row = b * RB + lr;
                        if (row < D && k < K) st[L.off_W + row * KP + k] = x;
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < ST; ++t) {
                const int tile = w + 4 * t;
                if (tile < KT * KT)
                    sacc[t] = wave_tile_mma_acc(sacc[t], SWb + (tile / KT) * 16, 1, LDM,
                                                SWb + (tile % KT) * 16, LDM, 1, RB);
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int t = 0; t < ST; ++t) {
        const int tile = w + 4 * t;
        if (tile < KT * KT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = (tile / KT) * 16 + l4 + 4 * r, j = (tile % KT) * 16 + l15;
                const double sww = (double)D * M[i * LDM + j] + sacc[t][r];
                T[i * LDM + j] = sww;
                if (i < K && j < K) st[L.off_Sww + i * KP + j] = sww;
            }
        }
    }
    __syncthreads();
    // ---- X, replicated half: Lambda_X = x_prec I + <tau> Sww ; A = <tau> Cov_X W^T --------
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        const int i = e / KP, j = e % KP;
        double x = (i == j) ? 1.0 : 0.0;
        if (i < K && j < K) {
            x = tau * 0.5 * (T[i * LDM + j] + T[j * LDM + i]);
            if (i == j) x += a.x_prec;
        }
        M[i * LDM + j] = x;
    }
    asm volatile("" : "+v"(tid));
    sweep_inverse<KP>(M, K, &logdet, &bad);
    asm volatile("" : "+v"(tid));
    w = tid >> 6, l15 = tid & 15, l4 = (tid & 63) >> 4;
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        const int i = e / KP, j = e % KP;
        if (i < K && j < K) st[L.off_CX + i * KP + j] = M[i * LDM + j];
    }
    // A = <tau> Cov_X W^T : per row block (KP x 32) = (KP x KP)(KP x 32); the rows of <W> come back
    // from global memory (written above by this workgroup, ordered by the barriers since; these
    // addresses were not read before, so no stale line can be hit)
    double wv[NB][NLB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int m = 0; m < NLB; ++m) {
            const int e = tid + m * NTF;
            const int r = b * RB + e / KP, k = e % KP;
            wv[b][m] = (r < D && k < K) ? st[L.off_W + r * KP + k] : 0.0;
        }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b < nb) {
#pragma unroll
            for (int m = 0; m < NLB; ++m) {
                const int e = tid + m * NTF;
                SWb[(e / KP) * LDM + (e % KP)] = wv[b][m];
            }
            __syncthreads();
#pragma unroll
            for (int t = 0; t < WT; ++t) {
                const int tile = w + 4 * t;
                if (tile < TPB) {
                    const int tk = tile % KT, td = tile / KT;
                    const v4f64 acc = wave_tile_mma(M + tk * 16 * LDM, LDM, 1, SWb + td * 16 * LDM, 1,
                                                    LDM, KP);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int k = tk * 16 + l4 + 4 * r, d = b * RB + td * 16 + l15;
                        if (k < K && d < D) st[L.off_A + k * DP + d] = tau * acc[r];
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        st[L.off_scal + 1] = logdet;
        if (bad) st[L.off_scal + 3] = (double)VMP_ERR_NOT_POSDEF;
    }
}

template <int KP>
__global__ void __launch_bounds__(NTF, 5)       // 5 waves per SIMD: holds the allocator to 96 VGPRs
pca_head_fast_kernel(small_args a, double *st, const double *stop)
{
    // batched sweeps (vmp_pca_sweeps): an earlier sweep of the batch has stopped the loop
    if (stop && stop[VMP_SWEEP_STOP] != 0.0) return;
    pca_head_body<KP>(a, st);
}

// (tau.update(), alpha.update(), lower bound)
// GRAM: the messages to W of the Gram form, S = [G A^T ; A G A^T] (sum y <x>^T and
// sum <x><x>^T collapsed onto the constant Gram matrix), are formed HERE first -- G streamed through
// LDS in batches of GB rows, A resident -- instead of by pca_gram_stats_kernel + reduce_partials_kernel
// in front of this kernel: one launch of the replicated-node chain instead of three beside the plate
// pass (BASELINE config 2: the chain, not the pass, set the iteration time).
// SWEEP (vmp_pca_sweeps): one sweep of a batch that runs without the host.  The kernel first reads the
// stop word an earlier sweep may have set and returns at once if it is set; it adds the DP / 8
// partial sums of sum <x><x>^T itself, in the fixed order of reduce_partials_kernel (no launch of
// that kernel); and after the bound it writes the sweep's ring slot, evaluates the loop's stop
// rule (vmp_stop_rule.h) and leaves the stop word and the bound for the next sweep.
constexpr int GB = 32;            // rows of G per batch
constexpr int GRA = 8;            // rows of G per workgroup of the Gram statistics (one partial block)
constexpr int TAIL_PLAIN = 0, TAIL_GRAM = 1, TAIL_SWEEP = 2;
// LDS of the tail (a struct: pca_sweep_mid_kernel hands Cx, Sx, al and sc on to the next head)
template <int KP>
struct alignas(16) tail_lds {
    double Sw[KP * (KP + 1)];       // Sww
    double Cx[KP * (KP + 1)];       // Cov_X
    double Sx[KP * (KP + 1)];       // sum <x><x>^T (shard sum)
    double al[4 * KP];              // alpha: a, b, <alpha>, <log alpha>
    double sc[8];                   // tau a, b, mean, logmean ; Syy ; log|LW| ; log|LX|
    double red[NTF / 64 + 1];
    double stop;                    // SWEEP: the stop word this tail left, for its own workgroup
};
// (a multiple of 16 bytes: the dynamic LDS behind it is accessed 16 bytes at a time)
static_assert(sizeof(tail_lds<16>) % 16 == 0 && sizeof(tail_lds<32>) % 16 == 0, "tail_lds size");
template <int KP, int MODE>
__device__ __forceinline__ void pca_tail_body(const small_args &a, double *st, const vmp_sweep_tail *sw,
                                              tail_lds<KP> &s)
{
    constexpr bool GRAM = (MODE == TAIL_GRAM);
    constexpr int LDM = KP + 1, E = KP * KP / NTF;
    extern __shared__ __align__(16) double gl[];          // GRAM: A (KP x (DP+1)) | G batch (GB x (DP+1)) | S batch (GB x LDM)
    double *Sw = s.Sw, *Cx = s.Cx, *Sx = s.Sx, *al = s.al, *sc = s.sc, *red = s.red;
    const lay32 L(a.L);
    const int tid = threadIdx.x, D = a.D, K = a.K;
    if constexpr (MODE == TAIL_SWEEP) {
        if (!sw->first && sw->ctl[VMP_SWEEP_STOP] != 0.0) {
            if (tid == 0) {
                sw->slot[7] = 0.0;                     // not executed
                sw->ctl[VMP_SWEEP_SKIPPED] += 1.0;
            }
            return;
        }
    }
    __builtin_amdgcn_s_setprio(3);   // latency-critical: win issue arbitration on a shared CU
    double t1 = 0.0;
    double sxx[E];
#pragma unroll
    for (int m = 0; m < E; ++m) sxx[m] = 0.0;
    if constexpr (MODE == TAIL_SWEEP) {
        // sum <x><x>^T = sum_b P[b] in the order of reduce_partials_kernel (vmp_pca.hip): the same bits
        const int nb = sw->nb;
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            const double *p = sw->P + e;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int b = 0;
            for (; b + 3 < nb; b += 4) {
                s0 += p[b * (KP * KP)];
                s1 += p[(b + 1) * (KP * KP)];
                s2 += p[(b + 2) * (KP * KP)];
                s3 += p[(b + 3) * (KP * KP)];
            }
            for (; b < nb; ++b) s0 += p[b * (KP * KP)];
            sxx[m] = (s0 + s1) + (s2 + s3);
            st[L.off_S + L.DP * KP + e] = sxx[m];
        }
    }
    if constexpr (GRAM) {
        const int DP = L.DP, LA = DP + 1;
        double *As = gl, *Gs = As + KP * LA, *Ss = Gs + GB * LA;
        for (int e = tid; e < KP * DP; e += NTF) {
            const int k = e / DP, d = e - k * DP;
            As[k * LA + d] = (k < K && d < D) ? st[L.off_A + k * DP + d] : 0.0;
        }
        for (int r0 = 0; r0 < D; r0 += GB) {
            for (int e = tid; e < GB * DP; e += NTF) {
                const int r = e / DP, d = e - r * DP;
                Gs[r * LA + d] = (r0 + r < D && d < D) ? st[(int)a.L.off_G + (r0 + r) * DP + d] : 0.0;
            }
            __syncthreads();
            // Syx[r][k] = sum_d G[r][d] A[k][d]  (and sum W o Syx on the way)
#pragma unroll
            for (int m = 0; m < GB * KP / NTF; ++m) {
                const int e = tid + m * NTF;
                const int r = e / KP, k = e % KP;
                const double *gr = Gs + r * LA, *ar = As + k * LA;
                double s0 = 0.0, s1 = 0.0;
                for (int d = 0; d < D; d += 2) {
                    s0 += gr[d] * ar[d];
                    s1 += gr[d + 1] * ar[d + 1];        // (d + 1 <= DP - 1: zero padded)
                }
                const double sv = s0 + s1;
                Ss[r * LDM + k] = sv;
                if (r0 + r < D) {
                    st[L.off_S + (r0 + r) * KP + k] = sv;
                    if (k < K) t1 += st[L.off_W + (r0 + r) * KP + k] * sv;
                }
            }
            __syncthreads();
            // Sxx[k][k'] += sum_{r in batch} A[k][r] Syx[r][k']
#pragma unroll
            for (int m = 0; m < E; ++m) {
                const int e = tid + m * NTF;
                const int i = e / KP, j = e % KP;
                double s0 = 0.0;
#pragma unroll 8
                for (int r = 0; r < GB; ++r) s0 += As[i * LA + r0 + r] * Ss[r * LDM + j];
                sxx[m] += s0;
            }
            __syncthreads();
        }
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            const int i = e / KP, j = e % KP;
            st[L.off_S + (L.DP + i) * KP + j] = (i < K && j < K) ? sxx[m] : 0.0;
        }
    }
    // ---- one batch of loads ------------------------------------------------------------
    {
        double v0[E], v1[E], v2[E];
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            const int i = e / KP, j = e % KP;
            const bool in = (i < K && j < K);
            v0[m] = in ? st[L.off_Sww + i * KP + j] : 0.0;
            v1[m] = in ? st[L.off_CX + i * KP + j] : 0.0;
            if constexpr (MODE != TAIL_PLAIN) v2[m] = in ? sxx[m] : 0.0;
            else v2[m] = in ? st[L.off_S + (L.DP + i) * KP + j] : 0.0;
        }
        if (tid == 0) {
            sc[4] = st[L.off_Syy];
            sc[5] = st[L.off_scal + 0];
            sc[6] = st[L.off_scal + 1];
        }
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            const int i = e / KP, j = e % KP;
            Sw[i * LDM + j] = v0[m];
            Cx[i * LDM + j] = v1[m];
            Sx[i * LDM + j] = v2[m];
        }
    }
    // sum(W o Syx): padded entries of W are zero, so the D x KP blocks are walked linearly
    if constexpr (!GRAM) {
        const int n = D * KP;
#pragma unroll 1
        for (int e0 = 0; e0 < n; e0 += 8 * NTF) {
            double w[8], y[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int e = e0 + tid + m * NTF;
                w[m] = e < n ? st[L.off_W + e] : 0.0;
                y[m] = e < n ? st[L.off_S + e] : 0.0;
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) t1 += w[m] * y[m];
        }
    }
    __syncthreads();
    double t2 = 0.0, trx = 0.0;
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        const int i = e / KP, j = e % KP;
        const double sxx = a.n_total * Cx[i * LDM + j] + 0.5 * (Sx[i * LDM + j] + Sx[j * LDM + i]);
        t2 += Sw[i * LDM + j] * sxx;
        if (i == j) trx += sxx;
    }
    t1 = block_sum<NTF>(t1, red);
    t2 = block_sum<NTF>(t2, red);
    trx = block_sum<NTF>(trx, red);
    // (dot.py:355 E1 and dot.py:403 E2 collapsed to traces)
    const double resid = sc[4] - 2.0 * t1 + t2;
    // ---- tau (gamma.py:116-148 with the message gaussian.py:2363-2369), alpha -------------
    if (tid == 64) {
        const double ta = a.a0t + 0.5 * (double)D * a.n_total;
        const double tb = a.b0t + 0.5 * resid;
        sc[0] = ta;
        sc[1] = tb;
        sc[2] = ta / tb;
        sc[3] = sf_digamma(ta) - sf_log(tb);
        st[L.off_tau + 0] = ta;
        st[L.off_tau + 1] = tb;
        st[L.off_tau + 2] = sc[2];
        st[L.off_tau + 3] = sc[3];
        st[L.off_scal + 2] = resid;
        if (!(tb > 0.0)) st[L.off_scal + 3] = (double)VMP_ERR_FLOATING;
        // the status word as the host would read it after this kernel
        if constexpr (MODE == TAIL_SWEEP)
            sc[7] = !(tb > 0.0) ? (double)VMP_ERR_FLOATING : st[L.off_scal + 3];
        // tau's term of the bound, here and not after the barrier: this wavefront has nothing else
        // to do while wavefront 0 works on alpha
        red[NTF / 64] = gamma_elbo(a.a0t, a.b0t, ta, tb, sc[2], sc[3]);
    }
    // ---- lower bound (expfamily.py:400-480): the Gamma terms beside their updates ----------
    double sla = 0.0, saw = 0.0, lal = 0.0;
    if (tid < K) {
        const double aa = a.a0a + 0.5 * (double)D;
        const double ab = a.b0a + 0.5 * Sw[tid * LDM + tid];
        const double am = aa / ab, alg = sf_digamma(aa) - sf_log(ab);
        al[0 * KP + tid] = aa;
        al[1 * KP + tid] = ab;
        al[2 * KP + tid] = am;
        al[3 * KP + tid] = alg;
        st[L.off_alpha + 0 * KP + tid] = aa;
        st[L.off_alpha + 1 * KP + tid] = ab;
        st[L.off_alpha + 2 * KP + tid] = am;
        st[L.off_alpha + 3 * KP + tid] = alg;
        // alpha's terms do not need tau: they run while wavefront 1 is still on tau's digamma
        sla = alg;
        saw = am * Sw[tid * LDM + tid];
        lal = gamma_elbo(a.a0a, a.b0a, aa, ab, am, alg);
    }
    sla = block_sum<NTF>(sla, red);
    saw = block_sum<NTF>(saw, red);
    lal = block_sum<NTF>(lal, red);
    if (tid == 0) {
        const double tau = sc[2], logtau = sc[3];
        const double Dd = (double)D, Kd = (double)K;
        const double LY = Dd * a.n_total * (-0.5 * sf_log(2.0 * M_PI) + 0.5 * logtau)
                          - 0.5 * tau * resid;
        const double LX = -0.5 * a.x_prec * trx
                          + a.n_total * (0.5 * Kd * sf_log(a.x_prec) - 0.5 * sc[6] + 0.5 * Kd);
        const double LW = 0.5 * Dd * sla - 0.5 * saw + Dd * (-0.5 * sc[5] + 0.5 * Kd);
        const double Lt = red[NTF / 64];
        st[L.off_L + 0] = LY;
        st[L.off_L + 1] = LX;
        st[L.off_L + 2] = LW;
        st[L.off_L + 3] = Lt;
        st[L.off_L + 4] = lal;
        st[L.off_L + 5] = LY + LX + LW + Lt + lal;
        if constexpr (MODE == TAIL_SWEEP) {
            const double status = sc[7];
            double *slot = sw->slot;
            slot[0] = LY;
            slot[1] = LX;
            slot[2] = LW;
            slot[3] = Lt;
            slot[4] = lal;
            slot[5] = LY + LX + LW + Lt + lal;
            slot[6] = status;
            slot[7] = 1.0;                             // executed
            // the terms go through LDS: indexed by the order the host adds them in
            al[0] = LY;
            al[1] = LX;
            al[2] = LW;
            al[3] = Lt;
            al[4] = lal;
            const double Lb = vmp_bound_sum(al, sw->order, sw->norder);
            const double L0 = sw->first ? sw->l0 : sw->ctl[VMP_SWEEP_L];
            int stop = status != 0.0;
            if (sw->compare && vmp_stop_rule(Lb, L0, sw->tol)) stop = 1;
            sw->ctl[VMP_SWEEP_STOP] = stop ? 1.0 : 0.0;
            s.stop = stop ? 1.0 : 0.0;
            sw->ctl[VMP_SWEEP_L] = Lb;
            sw->ctl[VMP_SWEEP_EXECUTED] += 1.0;
        }
    }
}

template <int KP, bool GRAM>
__global__ void __launch_bounds__(NTF)
pca_tail_fast_kernel(small_args a, double *st)
{
    __shared__ tail_lds<KP> s;
    pca_tail_body<KP, GRAM ? TAIL_GRAM : TAIL_PLAIN>(a, st, nullptr, s);
}

template <int KP>
__global__ void __launch_bounds__(NTF)
pca_tail_sweep_kernel(small_args a, double *st, vmp_sweep_tail sw)
{
    __shared__ tail_lds<KP> s;
    pca_tail_body<KP, TAIL_SWEEP>(a, st, &sw, s);
}

// ---------------------------------------------------------------------------
// One launch per held sweep (vmp_pca_sweeps, sweeps 1 .. n-1 of a chunk).
//
// Phase A, every workgroup: the rows of sum y<x>^T of the sweep for one group of GRA rows of G, what
// pca_gram_stats_kernel (vmp_pca.hip) computes and bit for bit the same -- every output is its own
// chain of fused multiply-adds over d = 0 .. D-1, from zero, in ascending order.  The partial blocks
// of sum <x><x>^T that kernel also stores are not formed here: the tail of phase B forms the sum from
// the A this phase leaves in LDS (sweep_tail_wide).
// Every load of A and G is requested before the first LDS write; the rows of A are DP + 2 doubles
// apart, so that they take 16-byte LDS writes; and every thread of the 8 x KP block of Syx owns one
// output.  The 32 lanes of a half wavefront are 16 columns x 2 rows: 16 rows of A, 4 banks apart, and
// two broadcast rows of G.
// The chains run on v_mfma_f64_4x4x4_4b_f64, which adds its four products to C as a chain of fused
// multiply-adds over the k-slots in ascending order (tests/test_mfma_order_gpu.py) -- so d = 4 q +
// slot, C carried over q, is the scalar chain of every output bit for bit.  A wavefront owns 4 rows x
// 16 columns, as four 4 x 4 blocks (lane x + 4 b + 16 s: row x of G and column 4 b + x of the 16, both
// at d = 4 q + s; its result is row s, column 4 b + x).  Operands at d >= D are zero.
// ---------------------------------------------------------------------------
__host__ __device__ inline size_t gram_phase_a_wide_lds(int KP, int DP)
{
    return ((size_t)KP * (DP + 2) + (size_t)GRA * DP + (size_t)GRA * (KP + 1)) * sizeof(double);
}

template <int KP, class STAMP = stamps_off>
__device__ __forceinline__ void gram_phase_a_wide(const vmp_pca_layout &L, int D, int K, double *st,
                                                  double *lds, int blk, const STAMP &stamp = STAMP())
{
    constexpr int LDS_S = KP + 1, KT = KP / 16;
    constexpr int NA = KP * (FAST_D / 2) / NTF, NG = GRA * (FAST_D / 2) / NTF;
    const int DP = (int)L.DP, LA = DP + 2;
    const int DP2 = DP >> 1, sh = __builtin_ctz(DP2);       // DP = 32, 64 or 128
    double *As = lds;                    // KP x LA (rows >= K zero)
    double *Gs = As + KP * LA;           // GRA x DP
    double *Ss = Gs + GRA * DP;          // GRA x LDS_S
    const int tid = threadIdx.x;
    const int r0 = blk * GRA;
    const double *A = st + L.off_A;
    const double *G = st + L.off_G + (int64_t)r0 * DP;
    // (every load is unconditional, from a clamped address, and masked afterwards: behind a branch
    // each would be waited for before the next is requested)
    v2f64 av[NA], gv[NG];
#pragma unroll
    for (int m = 0; m < NA; ++m) {
        const int e = tid + m * NTF;                         // (beyond KP DP2 at DP < 128: row K - 1)
        const int k = e >> sh, c = (e & (DP2 - 1)) * 2;
        av[m] = *reinterpret_cast<const v2f64 *>(A + (k < K ? k : K - 1) * DP + c);
    }
#pragma unroll
    for (int m = 0; m < NG; ++m) {
        const int e = tid + m * NTF;
        gv[m] = *reinterpret_cast<const v2f64 *>(G + 2 * (e < GRA * DP2 ? e : GRA * DP2 - 1));
    }
#pragma unroll
    for (int m = 0; m < NA; ++m) {
        const int e = tid + m * NTF;
        const int k = e >> sh, c = (e & (DP2 - 1)) * 2;
        if (e < KP * DP2) *reinterpret_cast<v2f64 *>(As + k * LA + c) = k < K ? av[m] : v2f64{0.0, 0.0};
    }
#pragma unroll
    for (int m = 0; m < NG; ++m) {
        const int e = tid + m * NTF;
        if (e < GRA * DP2) *reinterpret_cast<v2f64 *>(Gs + 2 * e) = gv[m];
    }
    __syncthreads();
    stamp(SP_LDS_FILLED);
    // Syx[r][k] = sum_d G[r][d] A[k][d]: one output per thread
    {
        const int w = tid >> 6, l = tid & 63;
        if (w < 2 * KT) {
            const int k = (l & 15) + 16 * (w % KT), r = (l >> 4) + 4 * (w / KT);
            double s = 0.0;
            // (r - l / 16 is the first of the wavefront's 4 rows, l / 16 this lane's k-slot)
            const int sl = l >> 4;
            const double *gx = Gs + (r - sl + (l & 3)) * DP + sl, *ax = As + k * LA + sl;
            const int D4 = D & ~3;
            int d = 0;
            // eight k-steps at a time, their sixteen LDS reads requested before the first is used
            for (; d + 32 <= D4; d += 32) {
                double gq[8], aq[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    gq[q] = gx[d + 4 * q];
                    aq[q] = ax[d + 4 * q];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) s = __builtin_amdgcn_mfma_f64_4x4x4f64(gq[q], aq[q], s, 0, 0, 0);
            }
            for (; d < D4; d += 4) s = __builtin_amdgcn_mfma_f64_4x4x4f64(gx[d], ax[d], s, 0, 0, 0);
            // D % 4 != 0: the last step, its k-slots at d >= D zero (read in bounds -- D4 + 3 < DP --
            // and masked afterwards, not behind a branch)
            if (D4 < D) {
                const double g4 = gx[D4], a4 = ax[D4];
                const bool in = D4 + sl < D;
                s = __builtin_amdgcn_mfma_f64_4x4x4f64(in ? g4 : 0.0, in ? a4 : 0.0, s, 0, 0, 0);
            }
            // (the block also goes to Ss, which nothing reads since the partial blocks went: the store
            // stays so that the mid kernels remain the instruction streams that were measured)
            Ss[r * LDS_S + k] = s;
            if (r0 + r < D && k < K) st[L.off_S + (r0 + r) * KP + k] = s;
        }
    }
    __syncthreads();
    stamp(SP_SYX);
}

// phase A alone (tests: bitwise against pca_gram_stats_kernel)
template <int KP>
__global__ void __launch_bounds__(NTF)
pca_gram_wide_kernel(vmp_pca_layout L, int D, int K, double *st)
{
    extern __shared__ __align__(16) double gl[];
    gram_phase_a_wide<KP>(L, D, K, st, gl, blockIdx.x);
}

// Phase B, the workgroup that draws the last ticket: the tail of this sweep and, unless that tail
// stops the loop, the head of the next one.  The ticket is the counter form of the in-launch
// reduction: every workgroup drains its stores, lane 0 releases at agent scope and draws; the one
// that draws nb - 1 knows that every other workgroup's Syx rows are released, acquires
// once and reads them with plain loads.  A ticket is drawn once and nobody waits for anybody: the
// other workgroups return, so there is no order of dispatch in which the launch cannot finish.
// `ticket` is this sweep's own word, zero at the launch: vmp_pca_sweeps clears the words once, when
// it allocates them, and the workgroup that draws nb - 1 -- the only one of its launch that is still
// running, after every other draw -- stores 0 again.  The next launch that draws from the word is a
// later one on the same stream (the same sweep of a later chunk): launches of a stream run in
// order and each sees the stores of those before it, so it finds 0.  A launch that returns at
// entry because the loop has stopped draws nothing and leaves the 0 it found.
// This kernel never runs beside a latent pass (no pass is in flight during held sweeps), so the
// placement budget of pca_head_fast_kernel and pca_tail_sweep_kernel does not bind it.
//
// sweep_tail_wide is the tail of phase B: the values of pca_tail_body<KP, TAIL_SWEEP>, bit for bit, by
// the same expressions and the same order of sums, scheduled for a workgroup that has the CU to itself.
// Every load is issued at the start.  The rows of sum y<x>^T go on to the next head in SW (DP x (KP+1)
// doubles of LDS, columns >= K and rows >= D zero) instead of being loaded a second time there.
// No partial blocks of sum <x><x>^T were stored: the sum is formed here from the rows in SW and from
// the A that phase A of this workgroup left in LDS (AL, KP rows DP + 2 doubles apart) -- every group's
// partial a chain of fused multiply-adds from zero over its 8 rows in ascending order
// (pca_gram_stats_kernel), the partials added four at a time in the order of reduce_partials_kernel.
// The stop word is not read here: the launch read it at entry, and no workgroup of a launch writes it
// before the tail of that launch.
// The tail ends with what the next head reads -- resid, tau's a, b and mean, the status condition on
// b, alpha's a, b and mean -- and leaves <log tau>, <log alpha>, the bound, the ring slot and the stop
// rule to defer_side below, which one wavefront runs beside the head's first inverse.  resid and trx
// wait in red[0] and red[1].
template <int KP, class STAMP>
__device__ __forceinline__ void sweep_tail_wide(const small_args &a, double *st, const vmp_sweep_tail &sw,
                                                tail_lds<KP> &s, double *SW, const double *AL,
                                                const STAMP &stamp)
{
    constexpr int LDM = KP + 1, E = KP * KP / NTF, NW = FAST_D * KP / NTF;
    double *Sw = s.Sw, *Cx = s.Cx, *Sx = s.Sx, *al = s.al, *sc = s.sc, *red = s.red;
    const lay32 L(a.L);
    const int tid = threadIdx.x, D = a.D, K = a.K;
    __builtin_amdgcn_s_setprio(3);   // latency-critical: win issue arbitration on a shared CU
    double t1 = 0.0;
    // ---- one batch of loads: <W>, sum y<x>^T, Sww, Cov_X and the scalars ------------------
    double ww[NW], wy[NW], es0[E], es1[E];
    {
        const int n = D * KP;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int e = tid + j * NTF;
            ww[j] = e < n ? st[L.off_W + e] : 0.0;
            wy[j] = e < n ? st[L.off_S + e] : 0.0;
        }
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            const int i = e / KP, j = e % KP;
            const bool in = (i < K && j < K);
            es0[m] = in ? st[L.off_Sww + i * KP + j] : 0.0;
            es1[m] = in ? st[L.off_CX + i * KP + j] : 0.0;
        }
    }
    if (tid == 0) {
        sc[4] = st[L.off_Syy];
        sc[5] = st[L.off_scal + 0];
        sc[6] = st[L.off_scal + 1];
    }
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        const int i = e / KP, j = e % KP;
        Sw[i * LDM + j] = es0[m];
        Cx[i * LDM + j] = es1[m];
    }
    // sum(W o Syx): the products in the order of pca_tail_body's loop, which runs whole passes of 8
    // per thread; all DP rows go to SW (zero beyond D and K), which the sum over the DP / 8 groups
    // below walks and of which the head reads whole 32-row blocks
    {
        const int n = D * KP, jn = (n + 8 * NTF - 1) / (8 * NTF) * 8;
        const int nsw = L.DP * KP;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int e = tid + j * NTF;
            if (j < jn) t1 += ww[j] * wy[j];
            if (e < nsw) SW[(e / KP) * LDM + (e % KP)] = (e < n && e % KP < K) ? wy[j] : 0.0;
        }
    }
    __syncthreads();
    stamp(SP_T_LOADS);
    // sum <x><x>^T on v_mfma_f64_16x16x4_f64: a wavefront owns a 16 x 16 tile of outputs, a group's
    // partial is two instructions from zero -- rows 0..3 of the group in the four k-slots, then rows
    // 4..7, C carried -- and the instruction adds its four products to C as a chain of fused
    // multiply-adds in ascending slot order (tests/test_mfma_order_gpu.py): the chain of 8 of
    // pca_gram_stats_kernel.  Lane l: A operand A[16 ti + l % 16][8 b + 4 h + l / 16], B operand
    // Syx[8 b + 4 h + l / 16][16 tj + l % 16], results (16 ti + l / 16 + 4 reg, 16 tj + l % 16).
    {
        constexpr int KT = KP / 16;
        const int LA = L.DP + 2;
        const int w = tid >> 6, l15 = tid & 15, l4 = (tid & 63) >> 4;
        const int nb = sw.nb, nb4 = nb & ~3;
        if (w < KT * KT) {
            const int ti = w / KT, tj = w % KT;
            const double *ar = AL + (16 * ti + l15) * LA + l4;
            const double *sr = SW + l4 * LDM + 16 * tj + l15;
            const auto group = [&](int b) {
                v4f64 p = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int h = 0; h < GRA; h += 4)
                    p = __builtin_amdgcn_mfma_f64_16x16x4f64(ar[b * GRA + h], sr[(b * GRA + h) * LDM], p,
                                                             0, 0, 0);
                return p;
            };
            v4f64 acc[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
            for (int b = 0; b < nb4; b += 4) {
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] += group(b + q);
            }
#pragma unroll 1
            for (int b = nb4; b < nb; ++b) acc[0] += group(b);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 16 * ti + l4 + 4 * r, k2 = 16 * tj + l15;
                const bool in = (k < K && k2 < K);
                const double x = in ? (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]) : 0.0;
                st[L.off_S + (L.DP + k) * KP + k2] = x;
                Sx[k * LDM + k2] = x;
            }
        }
    }
    __syncthreads();
    stamp(SP_T_PXX);
    double t2 = 0.0, trx = 0.0;
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        const int i = e / KP, j = e % KP;
        const double sxx = a.n_total * Cx[i * LDM + j] + 0.5 * (Sx[i * LDM + j] + Sx[j * LDM + i]);
        t2 += Sw[i * LDM + j] * sxx;
        if (i == j) trx += sxx;
    }
    {
        // the three block_sums behind one barrier: the wave sums go to twelve words of their own (the
        // <log alpha> quarter of al, which this tail does not use and nothing has touched since the
        // barrier above) and every thread adds each four in the order of block_sum
        double *r3 = al + 3 * KP;
        static_assert(KP >= 3 * (NTF / 64), "twelve words");
        t1 = wave_sum(t1);
        t2 = wave_sum(t2);
        trx = wave_sum(trx);
        if ((tid & 63) == 0) {
            r3[tid >> 6] = t1;
            r3[NTF / 64 + (tid >> 6)] = t2;
            r3[2 * (NTF / 64) + (tid >> 6)] = trx;
        }
        __syncthreads();
        t1 = t2 = trx = 0.0;
#pragma unroll
        for (int i = 0; i < NTF / 64; ++i) {
            t1 += r3[i];
            t2 += r3[NTF / 64 + i];
            trx += r3[2 * (NTF / 64) + i];
        }
    }
    stamp(SP_T_BLOCKSUMS);
    // (dot.py:355 E1 and dot.py:403 E2 collapsed to traces)
    const double resid = sc[4] - 2.0 * t1 + t2;
    // ---- tau (gamma.py:116-148 with the message gaussian.py:2363-2369) and alpha: the means ----
    if (tid == 64) {
        const double ta = a.a0t + 0.5 * (double)D * a.n_total;
        const double tb = a.b0t + 0.5 * resid;
        sc[0] = ta;
        sc[1] = tb;
        sc[2] = ta / tb;
        red[0] = resid;
        red[1] = trx;
        st[L.off_tau + 0] = ta;
        st[L.off_tau + 1] = tb;
        st[L.off_tau + 2] = sc[2];
        st[L.off_scal + 2] = resid;
        if (!(tb > 0.0)) st[L.off_scal + 3] = (double)VMP_ERR_FLOATING;
    }
    if (tid < K) {
        const double aa = a.a0a + 0.5 * (double)D;
        const double ab = a.b0a + 0.5 * Sw[tid * LDM + tid];
        const double am = aa / ab;
        al[0 * KP + tid] = aa;
        al[1 * KP + tid] = ab;
        al[2 * KP + tid] = am;
        st[L.off_alpha + 0 * KP + tid] = aa;
        st[L.off_alpha + 1 * KP + tid] = ab;
        st[L.off_alpha + 2 * KP + tid] = am;
    }
    // the critical path leaves the tail here: <log tau>, <log alpha>, the bound and the ring slot are
    // the side wavefront's, so the three stamps that stand for them coincide
    stamp(SP_T_TAU_ALPHA);
    stamp(SP_T_BOUND);
    stamp(SP_T_RING);
}

// pca_head_wide is the head of the next sweep as phase B runs it: pca_head_body without the placement
// budget.  The D x K operand -- the rows of sum y<x>^T the tail left in SW, then the rows of <W> --
// stays in LDS whole (whole 32-row blocks of it, as many as pca_head_body walks), so W = tau Syx Cov_W,
// Sww and A = tau Cov_X W^T are one barrier-delimited phase each and nothing is loaded from global
// memory.  Per output the MFMA sequence is the one of pca_head_body: over q for a tile of W and A,
// over the rows in ascending order for a tile of Sww.  Stores are the same.
//
// SIDE (pca_sweep_mid_kernel only): what runs beside the FIRST inverse, and `stopw`, the LDS word it
// leaves the stop decision in.  Every thread reads that word behind the inverse's closing barrier and
// the workgroup returns on a stop before the head has stored anything: Lambda_W and its inverse were
// computed for nothing, in LDS and registers only.
//
// defer_side is that work: the part of the tail that no head reads (see sweep_tail_wide).
// Wavefront 1 runs it, wavefronts 2 and 3 idle.  Lanes < K take alpha's Gamma node k, the lanes from
// K on tau's (lane 32 is the one whose values are used), through the same instructions: one sf_log
// per lane, of b, which serves <log .> = digamma(a) - log b and the node's bound term.  Every other
// special function has arguments that do not change from sweep to sweep and comes from `sf`
// (vmp_ctx::sweep_sf, filled by pca_sweep_sf_kernel with the same sf_* functions): values only, the
// expressions around them are those of the tail and of gamma_elbo.  sla, saw and lal are non-zero in
// the lanes < K of one wavefront, so block_sum's result is 0.0 + that wavefront's wave_sum: the same
// butterfly on the same lane layout, and the same -0 + 0.
// It reads Sww's diagonal (ts.Sw), sc[0..2] and sc[4..6], alpha's a, b and mean (ts.al), resid and
// trx (red[0..1]): LDS the head does not write before the closing barrier (Lambda_W is built in
// ts.Cx from ts.Sx and the means).  It writes al[0..4], alpha's a, which nothing reads after it.
template <int KP, class STAMP>
struct defer_side {
    const small_args &a;
    double *st;
    const vmp_sweep_tail &sw;
    tail_lds<KP> &s;
    const double *sf;
    const STAMP &stamp;
    __device__ __forceinline__ void operator()() const
    {
        constexpr int LDM = KP + 1;
        if (threadIdx.x >= 128) return;
        const lay32 L(a.L);
        const int l = threadIdx.x - 64, D = a.D, K = a.K;
        const bool isa = l < K;
        const int k = isa ? l : 0;
        const double a0 = isa ? a.a0a : a.a0t, b0 = isa ? a.b0a : a.b0t;
        const double av = isa ? s.al[0 * KP + k] : s.sc[0];
        const double bv = isa ? s.al[1 * KP + k] : s.sc[1];
        const double mean = isa ? s.al[2 * KP + k] : s.sc[2];
        const double *c = sf + (isa ? VMP_SWEEP_SF_ALPHA : VMP_SWEEP_SF_TAU);
        const double dg = c[0], lga = c[1], lga0 = c[2], logb0 = c[3];
        const double logb = sf_log(bv);
        const double logx = dg - logb;
        // gamma_elbo with the values of its special functions
        const double g_p = a0 * logb0 - lga0;
        const double g_q = av * logb - lga;
        const double g = g_p - g_q + (bv - b0) * mean + (a0 - av) * logx;
        if (isa) st[L.off_alpha + 3 * KP + k] = logx;
        if (l == 32) st[L.off_tau + 3] = logx;
        stamp.side(SP_S_STATE);
        const double sla = 0.0 + wave_sum(isa ? logx : 0.0);
        const double saw = 0.0 + wave_sum(isa ? mean * s.Sw[k * LDM + k] : 0.0);
        const double lal = 0.0 + wave_sum(isa ? g : 0.0);
        const double logtau = __shfl(logx, 32, 64), Lt = __shfl(g, 32, 64);
        if (l == 0) {
            const double tau = s.sc[2], resid = s.red[0], trx = s.red[1];
            const double Dd = (double)D, Kd = (double)K;
            const double LY = Dd * a.n_total * (-0.5 * sf[VMP_SWEEP_SF_LOG2PI] + 0.5 * logtau)
                              - 0.5 * tau * resid;
            const double LX = -0.5 * a.x_prec * trx
                              + a.n_total * (0.5 * Kd * sf[VMP_SWEEP_SF_LOGXPREC] - 0.5 * s.sc[6] + 0.5 * Kd);
            const double LW = 0.5 * Dd * sla - 0.5 * saw + Dd * (-0.5 * s.sc[5] + 0.5 * Kd);
            st[L.off_L + 0] = LY;
            st[L.off_L + 1] = LX;
            st[L.off_L + 2] = LW;
            st[L.off_L + 3] = Lt;
            st[L.off_L + 4] = lal;
            st[L.off_L + 5] = LY + LX + LW + Lt + lal;
            // the status word as the host would read it after the tail
            const double status = !(s.sc[1] > 0.0) ? (double)VMP_ERR_FLOATING : st[L.off_scal + 3];
            double *slot = sw.slot;
            slot[0] = LY;
            slot[1] = LX;
            slot[2] = LW;
            slot[3] = Lt;
            slot[4] = lal;
            slot[5] = LY + LX + LW + Lt + lal;
            slot[6] = status;
            slot[7] = 1.0;                             // executed
            double *al = s.al;
            al[0] = LY;
            al[1] = LX;
            al[2] = LW;
            al[3] = Lt;
            al[4] = lal;
            const double Lb = vmp_bound_sum(al, sw.order, sw.norder);
            const double L0 = sw.first ? sw.l0 : sw.ctl[VMP_SWEEP_L];
            int stop = status != 0.0;
            if (sw.compare && vmp_stop_rule(Lb, L0, sw.tol)) stop = 1;
            sw.ctl[VMP_SWEEP_STOP] = stop ? 1.0 : 0.0;
            s.stop = stop ? 1.0 : 0.0;
            sw.ctl[VMP_SWEEP_L] = Lb;
            sw.ctl[VMP_SWEEP_EXECUTED] += 1.0;
        }
        stamp.side(SP_S_RING);
    }
};

template <int KP, class STAMP, class SIDE = no_side>
__device__ __forceinline__ void pca_head_wide(const small_args &a, double *st, double *M, double *T,
                                              const double *alm, double tau, double *SW,
                                              const STAMP &stamp, const SIDE &side = SIDE(),
                                              const double *stopw = nullptr)
{
    constexpr bool DEFER = !std::is_same<SIDE, no_side>::value;
    constexpr int LDM = KP + 1, E = KP * KP / NTF, KT = KP / 16;
    constexpr int WT = FAST_D / 16 * KT / 4;      // 16 x 16 tiles of the D x K operand per wavefront
    constexpr int ST = (KT * KT + 3) / 4;         // tiles of Sww per wavefront
    __shared__ double logdet;
    __shared__ int bad;
    const lay32 L(a.L);
    const int tid = threadIdx.x, D = a.D, K = a.K, DP = (int)L.DP;
    const int nr = (D + 31) / 32 * 32;            // rows of SW in use
    const int nt = nr / 16 * KT;                  // ... and its tiles
    const int w = tid >> 6, l15 = tid & 15, l4 = (tid & 63) >> 4;
    if (tid == 0) bad = 0;
    // ---- W: Lambda_W = diag<alpha> + <tau> Sxx ------------------------------------------
    {
        double lam[E];
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            const int i = e / KP, j = e % KP;
            double x = (i == j) ? 1.0 : 0.0;
            if (i < K && j < K) {
                x = tau * (a.n_total * M[i * LDM + j] + 0.5 * (T[i * LDM + j] + T[j * LDM + i]));
                if (i == j) x += alm[i];
            }
            lam[m] = x;
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < E; ++m) {
            const int e = tid + m * NTF;
            M[(e / KP) * LDM + (e % KP)] = lam[m];
        }
    }
    stamp(SP_H_LAMBDA);
    if constexpr (DEFER) {
        sweep_inverse<KP>(M, K, &logdet, &bad, side);
        // the side work has evaluated the stop rule: nothing of this head is in the state yet
        if (*stopw != 0.0) return;
    } else {
        sweep_inverse<KP>(M, K, &logdet, &bad);
    }
    stamp(SP_H_INV1);
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        const int i = e / KP, j = e % KP;
        if (i < K && j < K) st[L.off_CW + i * KP + j] = M[i * LDM + j];
    }
    if (tid == 0) st[L.off_scal + 0] = logdet;
    // <w_d> = <tau> Cov_W Syx[d]: every tile first, then the rows of <W> replace those of Syx
    v4f64 wt[WT];
#pragma unroll
    for (int t = 0; t < WT; ++t) {
        const int tile = w + 4 * t;
        if (tile < nt)
            wt[t] = wave_tile_mma(SW + (tile / KT) * 16 * LDM, LDM, 1, M + (tile % KT) * 16, LDM, 1, KP);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < WT; ++t) {
        const int tile = w + 4 * t;
        if (tile < nt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (tile / KT) * 16 + l4 + 4 * r, k = (tile % KT) * 16 + l15;
                const double x = tau * wt[t][r];
                SW[row * LDM + k] = x;
                if (row < D && k < K) st[L.off_W + row * KP + k] = x;
            }
        }
    }
    __syncthreads();
    stamp(SP_H_W);
    // Sww = D Cov_W + W^T W: one chain over the rows per tile
#pragma unroll
    for (int t = 0; t < ST; ++t) {
        const int tile = w + 4 * t;
        if (tile < KT * KT) {
            const v4f64 sacc = wave_tile_mma_acc(v4f64{0.0, 0.0, 0.0, 0.0}, SW + (tile / KT) * 16, 1, LDM,
                                                 SW + (tile % KT) * 16, LDM, 1, nr);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = (tile / KT) * 16 + l4 + 4 * r, j = (tile % KT) * 16 + l15;
                const double sww = (double)D * M[i * LDM + j] + sacc[r];
                T[i * LDM + j] = sww;
                if (i < K && j < K) st[L.off_Sww + i * KP + j] = sww;
            }
        }
    }
    __syncthreads();
    stamp(SP_H_SWW);
    // ---- X, replicated half: Lambda_X = x_prec I + <tau> Sww ; A = <tau> Cov_X W^T --------
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        const int i = e / KP, j = e % KP;
        double x = (i == j) ? 1.0 : 0.0;
        if (i < K && j < K) {
            x = tau * 0.5 * (T[i * LDM + j] + T[j * LDM + i]);
            if (i == j) x += a.x_prec;
        }
        M[i * LDM + j] = x;
    }
    // pca_head_body multiplies by the rows of <W> it loads back from the state, which are exactly
    // zero beyond D and K: wavefronts 1 .. 3 make SW so while wavefront 0 inverts
    const auto pad = [&]() {
        if (D == nr && K == KP) return;
        for (int e = tid - 64; e < nr * KP; e += NTF - 64)
            if (e / KP >= D || e % KP >= K) SW[(e / KP) * LDM + (e % KP)] = 0.0;
    };
    sweep_inverse<KP>(M, K, &logdet, &bad, pad);
    stamp(SP_H_INV2);
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        const int i = e / KP, j = e % KP;
        if (i < K && j < K) st[L.off_CX + i * KP + j] = M[i * LDM + j];
    }
#pragma unroll
    for (int t = 0; t < WT; ++t) {
        const int tile = w + 4 * t;
        if (tile < nt) {
            const int tk = tile % KT, td = tile / KT;
            const v4f64 acc = wave_tile_mma(M + tk * 16 * LDM, LDM, 1, SW + td * 16 * LDM, 1, LDM, KP);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = tk * 16 + l4 + 4 * r, d = td * 16 + l15;
                if (k < K && d < D) st[L.off_A + k * DP + d] = tau * acc[r];
            }
        }
    }
    if (tid == 0) {
        st[L.off_scal + 1] = logdet;
        if (bad) st[L.off_scal + 3] = (double)VMP_ERR_NOT_POSDEF;
    }
    stamp.drain();
    stamp(SP_H_A);
}

// the dynamic LDS of the one-launch sweep: A (phase A, kept for the tail) | the G rows and the Syx
// block of phase A, then the DP rows of SW | the ticket word, which gets 16 bytes of its own so that
// A survives the draw
__host__ __device__ inline size_t sweep_local_lds(int KP, int DP)
{
    return ((size_t)KP * (DP + 2) + (size_t)DP * (KP + 1) + 2) * sizeof(double);
}

template <int KP, class STAMP>
__device__ __forceinline__ void pca_sweep_mid_body(const small_args &a, double *st,
                                                   const vmp_sweep_tail &sw, unsigned int *ticket,
                                                   const double *sf, const STAMP &stamp)
{
    extern __shared__ __align__(16) double gl[];
    __shared__ tail_lds<KP> ts;
    const int tid = threadIdx.x;
    // an earlier sweep of the batch has stopped the loop: no ticket is drawn
    if (!sw.first && sw.ctl[VMP_SWEEP_STOP] != 0.0) {
        if (blockIdx.x == 0 && tid == 0) {
            sw.slot[7] = 0.0;                          // not executed
            sw.ctl[VMP_SWEEP_SKIPPED] += 1.0;
        }
        return;
    }
    stamp(SP_ENTRY);
    gram_phase_a_wide<KP, STAMP>(a.L, a.D, a.K, st, gl, blockIdx.x, stamp);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    stamp(SP_PXX);
    // SW lies behind A, over the G rows and the Syx block of phase A, the ticket word behind SW
    const int na = KP * ((int)a.L.DP + 2);
    double *SW = gl + na;
    unsigned int *word = reinterpret_cast<unsigned int *>(SW + (int)a.L.DP * (KP + 1));
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        *word = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (*word != gridDim.x - 1) return;
    stamp(SP_TICKET);
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        // every other workgroup of the launch has drawn: the word is this workgroup's alone, and it
        // goes back to 0 for the next launch that uses it (see above; also when the tail stops the loop)
        *ticket = 0u;
    }
    __syncthreads();
    stamp(SP_ACQUIRE);
    // (phase A's G rows and Syx block are read no more: their region is free for SW)
    sweep_tail_wide<KP>(a, st, sw, ts, SW, gl, stamp);
    __syncthreads();
    // the rest of the tail, the stop rule included, runs beside the head's first inverse; the head
    // reads ts.stop behind it, before its first store.  Cov_X, sum <x><x>^T, <alpha>, <tau> and the
    // Syx rows (in SW) go over in LDS
    const defer_side<KP, STAMP> side{a, st, sw, ts, sf, stamp};
    pca_head_wide<KP>(a, st, ts.Cx, ts.Sx, ts.al + 2 * KP, ts.sc[2], SW, stamp, side, &ts.stop);
}

// `sf`: the sweep-invariant special functions of the side wavefront (vmp_ctx::sweep_sf).  `P`, the
// partial blocks of the three-launch sweep, is not used; it keeps the argument block of the launch
// what it was.
template <int KP>
__global__ void __launch_bounds__(NTF)
pca_sweep_mid_kernel(small_args a, double *st, double *P, vmp_sweep_tail sw, unsigned int *ticket,
                     const double *sf)
{
    pca_sweep_mid_body<KP>(a, st, sw, ticket, sf, stamps_off());
}

// the same with wall_clock64 stamps ("pca_sweep_stamps"): `out` is this launch's row of
// VMP_SWEEP_NSTAMP words, written by the workgroup that ran phase B; `level` the key's value (2: the
// side wavefront stamps too)
template <int KP>
__global__ void __launch_bounds__(NTF)
pca_sweep_mid_stamped_kernel(small_args a, double *st, double *P, vmp_sweep_tail sw,
                             unsigned int *ticket, const double *sf, unsigned long long *out, int level)
{
    __shared__ unsigned long long stl[VMP_SWEEP_NSTAMP];
    if (threadIdx.x < VMP_SWEEP_NSTAMP) stl[threadIdx.x] = 0;
    __syncthreads();
    const stamps_on stamp{stl, level};
    pca_sweep_mid_body<KP>(a, st, sw, ticket, sf, stamp);
    // (a workgroup that did not run phase B leaves no tail stamp)
    if (threadIdx.x == 0 && stl[SP_T_LOADS] != 0)
        for (int i = 0; i < VMP_SWEEP_NSTAMP; ++i) out[i] = stl[i];
}

// The first head of a chunk (vmp_pca_sweeps, one-launch sweeps, no latent pass in flight): the
// wide head body in a launch of its own.  What the tail of a mid launch hands over in LDS -- Cov_X,
// sum <x><x>^T, <alpha>, <tau> and the rows of sum y<x>^T -- is loaded from the state, masked as
// pca_head_body masks its loads.
template <int KP>
__global__ void __launch_bounds__(NTF)
pca_head_wide_kernel(small_args a, double *st)
{
    constexpr int LDM = KP + 1, E = KP * KP / NTF, NW = FAST_D * KP / NTF;
    __shared__ __align__(16) double M[KP * LDM], T[KP * LDM], SW[FAST_D * LDM], alm[KP];
    const lay32 L(a.L);
    const int tid = threadIdx.x, D = a.D, K = a.K;
    const int n = D * KP, nsw = (D + 31) / 32 * 32 * KP;
    double cx[E], sx[E], wy[NW];
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        const int i = e / KP, j = e % KP;
        const bool in = (i < K && j < K);
        cx[m] = in ? st[L.off_CX + i * KP + j] : 0.0;
        sx[m] = in ? st[L.off_S + (L.DP + i) * KP + j] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const int e = tid + j * NTF;
        wy[j] = (e < n && e % KP < K) ? st[L.off_S + e] : 0.0;
    }
    const double tau = st[L.off_tau + 2];
    if (tid < KP) alm[tid] = tid < K ? st[L.off_alpha + 2 * KP + tid] : 0.0;
#pragma unroll
    for (int m = 0; m < E; ++m) {
        const int e = tid + m * NTF;
        M[(e / KP) * LDM + (e % KP)] = cx[m];
        T[(e / KP) * LDM + (e % KP)] = sx[m];
    }
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        const int e = tid + j * NTF;
        if (e < nsw) SW[(e / KP) * LDM + (e % KP)] = wy[j];
    }
    __syncthreads();
    pca_head_wide<KP>(a, st, M, T, alm, tau, SW, stamps_off());
}

// The special functions of the held sweeps whose arguments stay the same from sweep to sweep
// (vmp_ctx::sweep_sf, VMP_SWEEP_SF_*): one wavefront, a lane per value, through the sf_* functions the
// tails call -- the same code, so the bits a tail computes.
__global__ void __launch_bounds__(64)
pca_sweep_sf_kernel(small_args a, double *sf)
{
    const int l = threadIdx.x;
    if (l >= VMP_SWEEP_SF_LEN) return;
    const double ta = a.a0t + 0.5 * (double)a.D * a.n_total;
    const double aa = a.a0a + 0.5 * (double)a.D;
    double v;
    switch (l) {
    case VMP_SWEEP_SF_TAU + 0: v = sf_digamma(ta); break;
    case VMP_SWEEP_SF_TAU + 1: v = sf_lgamma(ta); break;
    case VMP_SWEEP_SF_TAU + 2: v = sf_lgamma(a.a0t); break;
    case VMP_SWEEP_SF_TAU + 3: v = sf_log(a.b0t); break;
    case VMP_SWEEP_SF_ALPHA + 0: v = sf_digamma(aa); break;
    case VMP_SWEEP_SF_ALPHA + 1: v = sf_lgamma(aa); break;
    case VMP_SWEEP_SF_ALPHA + 2: v = sf_lgamma(a.a0a); break;
    case VMP_SWEEP_SF_ALPHA + 3: v = sf_log(a.b0a); break;
    case VMP_SWEEP_SF_LOG2PI: v = sf_log(2.0 * M_PI); break;
    default: v = sf_log(a.x_prec); break;
    }
    sf[l] = v;
}

// The two fp64 matrix instructions on caller-supplied tiles, one wavefront, one instruction per
// tile (vmp_mfma_order_probe; tests/test_mfma_order_gpu.py reads the order of accumulation off the
// bits).  FORM 0: v_mfma_f64_16x16x4_f64, A 16 x 4, B 4 x 16, C and D 16 x 16, row-major.
// FORM 1: v_mfma_f64_4x4x4_4b_f64, four independent blocks, A[b][i][k], B[b][k][j], C and D [b][i][j].
template <int FORM>
__global__ void __launch_bounds__(64)
mfma_order_probe_kernel(int n, const double *A, const double *B, const double *C, double *Dm)
{
    const int l = threadIdx.x, lo = l & 15, k = l >> 4;
    for (int t = 0; t < n; ++t) {
        if constexpr (FORM == 0) {
            const double *Ct = C + (size_t)t * 256;
            double *Dt = Dm + (size_t)t * 256;
            v4f64 c;
#pragma unroll
            for (int r = 0; r < 4; ++r) c[r] = Ct[(k + 4 * r) * 16 + lo];
            const v4f64 d = __builtin_amdgcn_mfma_f64_16x16x4f64(A[(size_t)t * 64 + lo * 4 + k],
                                                                 B[(size_t)t * 64 + k * 16 + lo], c, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) Dt[(k + 4 * r) * 16 + lo] = d[r];
        } else {
            // lane x + 4 b + 16 k holds A[b][x][k] and B[b][k][x]; lane j + 4 b + 16 i holds D[b][i][j]
            const int x = l & 3, b = (l >> 2) & 3;
            const size_t o = (size_t)t * 64 + b * 16;
            Dm[o + k * 4 + x] = __builtin_amdgcn_mfma_f64_4x4x4f64(A[o + x * 4 + k], B[o + k * 4 + x],
                                                                   C[o + k * 4 + x], 0, 0, 0);
        }
    }
}

bool fast_small_enabled()
{
    static const int v = getenv("VMP_PCA_FAST_SMALL") ? atoi(getenv("VMP_PCA_FAST_SMALL")) : 1;
    return v != 0;
}

int32_t fill_small_args(vmp_ctx *ctx, small_args &a, int32_t D, int32_t K, int64_t n_total,
                        double x_prec, double a0t, double b0t, double a0a, double b0a)
{
    const int32_t rc = vmp_pca_get_layout(D, K, &a.L);
    VMP_REQUIRE(ctx, rc == VMP_OK, rc, "unsupported dims D=%d K=%d", D, K);
    a.D = D;
    a.K = K;
    a.n_total = (double)n_total;
    a.x_prec = x_prec;
    a.a0t = a0t; a.b0t = b0t; a.a0a = a0a; a.b0a = b0a;
    a.has_mean = 0;
    return VMP_OK;
}

template <int O0, int O1, int O2>
void launch_sequence(vmp_ctx *ctx, const small_args &a, double *state)
{
    // 256 threads (fits beside the streaming grid), except the K x K inverses of K > 32
    constexpr bool has_inverse = (O0 == VMP_PCA_OP_W || O0 == VMP_PCA_OP_XPREP ||
                                  O1 == VMP_PCA_OP_W || O1 == VMP_PCA_OP_XPREP);
    constexpr int NT64 = has_inverse ? 1024 : 256;
    if (a.L.KP == 16)
        hipLaunchKernelGGL((pca_small_kernel<16, 256, O0, O1, O2>), dim3(1), dim3(256), 0,
                           ctx->stream, a, state);
    else if (a.L.KP == 32)
        hipLaunchKernelGGL((pca_small_kernel<32, 256, O0, O1, O2>), dim3(1), dim3(256), 0,
                           ctx->stream, a, state);
    else
        hipLaunchKernelGGL((pca_small_kernel<64, NT64, O0, O1, O2>), dim3(1), dim3(NT64), 0,
                           ctx->stream, a, state);
}

int32_t launch_small(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                     double a0t, double b0t, double a0a, double b0a, int32_t nops,
                     const int32_t *ops, double *state, int32_t has_mean = 0)
{
    VMP_REQUIRE(ctx, ctx && state && ops, VMP_ERR_INVALID, "null argument");
    VMP_REQUIRE(ctx, nops >= 1 && nops <= VMP_PCA_MAX_OPS, VMP_ERR_INVALID,
                "between 1 and %d operations per call", VMP_PCA_MAX_OPS);
    small_args a;
    int32_t rc = vmp_pca_get_layout(D, K, &a.L);
    VMP_REQUIRE(ctx, rc == VMP_OK, rc, "unsupported dims D=%d K=%d", D, K);
    a.D = D;
    a.K = K;
    a.n_total = (double)n_total;
    a.x_prec = x_prec;
    a.a0t = a0t; a.b0t = b0t; a.a0a = a0a; a.b0a = b0a;
    a.has_mean = has_mean ? 1 : 0;
    for (int i = 0; i < nops; ++i) {
        const int op = ops[i];
        VMP_REQUIRE(ctx, op >= VMP_PCA_OP_W && op <= VMP_PCA_OP_ELBO, VMP_ERR_INVALID,
                    "unknown operation code %d", op);
        if (op == VMP_PCA_OP_XPREP || op == VMP_PCA_OP_ELBO)
            VMP_REQUIRE(ctx, x_prec > 0, VMP_ERR_INVALID, "x_prec must be positive");
        if (op == VMP_PCA_OP_TAU || op == VMP_PCA_OP_ELBO)
            VMP_REQUIRE(ctx, a0t > 0 && b0t > 0, VMP_ERR_INVALID,
                        "Gamma prior parameters must be positive");
        if (op == VMP_PCA_OP_ALPHA || op == VMP_PCA_OP_ELBO)
            VMP_REQUIRE(ctx, a0a > 0 && b0a > 0, VMP_ERR_INVALID,
                        "Gamma prior parameters must be positive");
    }
    // greedy: the two sequences a VB iteration produces are single launches (LDS-resident
    // forms when K <= 32 and D <= 128; VMP_PCA_FAST_SMALL=0 disables them), anything else
    // falls back to one launch per operation
    const bool fast_enabled = fast_small_enabled();
    // (the LDS-resident forms are built for the zero prior mean of the demo model)
    const bool fast = fast_enabled && a.L.KP <= 32 && D <= FAST_D && !a.has_mean;
    // the Gram-form messages to W of the latest latent pass may still be pending (vmp_pca.hip
    // run_xpass): the LDS-resident tail kernel forms them itself when it comes first, anything
    // else has them formed now
    bool gram_here = false;
    if (ctx->gram_pending) {
        const bool tail_first = nops >= 3 && ops[0] == VMP_PCA_OP_TAU && ops[1] == VMP_PCA_OP_ALPHA
                                && ops[2] == VMP_PCA_OP_ELBO;
        if (fast && tail_first && ctx->gram_state == state && ctx->gram_D == D && ctx->gram_K == K) {
            gram_here = true;
            ctx->gram_pending = 0;
        } else {
            rc = vmp_pca_ensure_gram(ctx);
            if (rc != VMP_OK) return rc;
        }
    }
    int i = 0;
    while (i < nops) {
        const int o0 = ops[i], o1 = i + 1 < nops ? ops[i + 1] : 0, o2 = i + 2 < nops ? ops[i + 2] : 0;
        if (o0 == VMP_PCA_OP_W && o1 == VMP_PCA_OP_XPREP) {
            if (fast && a.L.KP == 16)
                hipLaunchKernelGGL(pca_head_fast_kernel<16>, dim3(1), dim3(NTF), 0, ctx->stream, a,
                                   state, (const double *)nullptr);
            else if (fast)
                hipLaunchKernelGGL(pca_head_fast_kernel<32>, dim3(1), dim3(NTF), 0, ctx->stream, a,
                                   state, (const double *)nullptr);
            else
                launch_sequence<VMP_PCA_OP_W, VMP_PCA_OP_XPREP, 0>(ctx, a, state);
            i += 2;
        } else if (o0 == VMP_PCA_OP_TAU && o1 == VMP_PCA_OP_ALPHA && o2 == VMP_PCA_OP_ELBO) {
            if (fast && gram_here) {
                // S = [G A^T; A G A^T] of the latest pass is formed by the tail kernel itself
                const size_t lds = ((size_t)(a.L.KP + GB) * (a.L.DP + 1) + (size_t)GB * (a.L.KP + 1))
                                   * sizeof(double);
                static bool raised[64] = {false};
                const int dev = ctx->device & 63;
                if (!raised[dev]) {
                    VMP_HIP_CHECK(ctx, hipFuncSetAttribute(
                        (const void *)pca_tail_fast_kernel<16, true>,
                        hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
                    VMP_HIP_CHECK(ctx, hipFuncSetAttribute(
                        (const void *)pca_tail_fast_kernel<32, true>,
                        hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
                    raised[dev] = true;
                }
                if (a.L.KP == 16)
                    hipLaunchKernelGGL((pca_tail_fast_kernel<16, true>), dim3(1), dim3(NTF), lds,
                                       ctx->stream, a, state);
                else
                    hipLaunchKernelGGL((pca_tail_fast_kernel<32, true>), dim3(1), dim3(NTF), lds,
                                       ctx->stream, a, state);
                gram_here = false;
            } else if (fast && a.L.KP == 16)
                hipLaunchKernelGGL((pca_tail_fast_kernel<16, false>), dim3(1), dim3(NTF), 0,
                                   ctx->stream, a, state);
            else if (fast)
                hipLaunchKernelGGL((pca_tail_fast_kernel<32, false>), dim3(1), dim3(NTF), 0,
                                   ctx->stream, a, state);
            else
                launch_sequence<VMP_PCA_OP_TAU, VMP_PCA_OP_ALPHA, VMP_PCA_OP_ELBO>(ctx, a, state);
            i += 3;
        } else {
            switch (o0) {
            case VMP_PCA_OP_W: launch_sequence<VMP_PCA_OP_W, 0, 0>(ctx, a, state); break;
            case VMP_PCA_OP_XPREP: launch_sequence<VMP_PCA_OP_XPREP, 0, 0>(ctx, a, state); break;
            case VMP_PCA_OP_TAU: launch_sequence<VMP_PCA_OP_TAU, 0, 0>(ctx, a, state); break;
            case VMP_PCA_OP_ALPHA: launch_sequence<VMP_PCA_OP_ALPHA, 0, 0>(ctx, a, state); break;
            default: launch_sequence<VMP_PCA_OP_ELBO, 0, 0>(ctx, a, state); break;
            }
            i += 1;
        }
        VMP_HIP_CHECK(ctx, hipGetLastError());
    }
    return VMP_OK;
}

}  // namespace

int32_t vmp_pca_sweep_covered(int32_t D, int32_t K)
{
    vmp_pca_layout L;
    if (vmp_pca_get_layout(D, K, &L) != VMP_OK) return VMP_PCA_SWEEPS_NOT_BUILT;
    return (fast_small_enabled() && L.KP <= 32 && D <= FAST_D) ? VMP_OK : VMP_PCA_SWEEPS_NOT_BUILT;
}

int32_t vmp_pca_launch_sweep_head(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                                  double a0t, double b0t, double a0a, double b0a, double *state,
                                  const double *stop)
{
    small_args a;
    const int32_t rc = fill_small_args(ctx, a, D, K, n_total, x_prec, a0t, b0t, a0a, b0a);
    if (rc != VMP_OK) return rc;
    if (a.L.KP == 16)
        hipLaunchKernelGGL(pca_head_fast_kernel<16>, dim3(1), dim3(NTF), 0, ctx->stream, a, state, stop);
    else
        hipLaunchKernelGGL(pca_head_fast_kernel<32>, dim3(1), dim3(NTF), 0, ctx->stream, a, state, stop);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_pca_launch_sweep_tail(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                                  double a0t, double b0t, double a0a, double b0a, double *state,
                                  const vmp_sweep_tail &t)
{
    small_args a;
    const int32_t rc = fill_small_args(ctx, a, D, K, n_total, x_prec, a0t, b0t, a0a, b0a);
    if (rc != VMP_OK) return rc;
    if (a.L.KP == 16)
        hipLaunchKernelGGL(pca_tail_sweep_kernel<16>, dim3(1), dim3(NTF), 0, ctx->stream, a, state, t);
    else
        hipLaunchKernelGGL(pca_tail_sweep_kernel<32>, dim3(1), dim3(NTF), 0, ctx->stream, a, state, t);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

// the dynamic LDS of phase A (at most 43 KB) beside 35 KB of static LDS needs the limit raised
template <typename F>
static int32_t raise_lds_once(vmp_ctx *ctx, F *k16, F *k32, bool *raised)
{
    const int dev = ctx->device & 63;
    if (raised[dev]) return VMP_OK;
    VMP_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k16,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    VMP_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)k32,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    raised[dev] = true;
    return VMP_OK;
}

int32_t vmp_pca_launch_gram_fast(vmp_ctx *ctx, int32_t D, int32_t K, double *state)
{
    vmp_pca_layout L;
    const int32_t rc = vmp_pca_get_layout(D, K, &L);
    VMP_REQUIRE(ctx, rc == VMP_OK, rc, "unsupported dims D=%d K=%d", D, K);
    VMP_REQUIRE(ctx, L.KP <= 32 && D <= FAST_D, VMP_ERR_UNSUPPORTED,
                "the fast Gram statistics cover K <= 32, D <= %d", FAST_D);
    VMP_REQUIRE(ctx, ((uintptr_t)state % 16) == 0, VMP_ERR_INVALID, "state must be 16-byte aligned");
    static bool raised[64] = {false};
    const int32_t rr = raise_lds_once(ctx, pca_gram_wide_kernel<16>, pca_gram_wide_kernel<32>, raised);
    if (rr != VMP_OK) return rr;
    const int nb = (int)(L.DP / GRA);
    const size_t lds = gram_phase_a_wide_lds((int)L.KP, (int)L.DP);
    if (L.KP == 16)
        hipLaunchKernelGGL(pca_gram_wide_kernel<16>, dim3(nb), dim3(NTF), lds, ctx->stream, L, D, K,
                           state);
    else
        hipLaunchKernelGGL(pca_gram_wide_kernel<32>, dim3(nb), dim3(NTF), lds, ctx->stream, L, D, K,
                           state);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

// one instantiation of the one-launch sweep; `stamps` (null: the default kernel) is the launch's row
template <int KP>
static int32_t launch_mid(vmp_ctx *ctx, const small_args &a, double *state, double *P,
                          const vmp_sweep_tail &t, unsigned int *ticket, unsigned long long *stamps,
                          int stamp_level)
{
    VMP_REQUIRE(ctx, ctx->sweep_sf, VMP_ERR_INVALID,
                "the one-launch sweep needs vmp_pca_sweep_constants first");
    static bool raised[2][64] = {{false}};
    const int dev = ctx->device & 63, s = stamps ? 1 : 0;
    if (!raised[s][dev]) {
        const void *f = stamps ? (const void *)pca_sweep_mid_stamped_kernel<KP>
                               : (const void *)pca_sweep_mid_kernel<KP>;
        VMP_HIP_CHECK(ctx, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               96 * 1024));
        raised[s][dev] = true;
    }
    // (A beside the DP rows of SW: 67 KB at KP = 32, DP = 128)
    const size_t lds = sweep_local_lds((int)a.L.KP, (int)a.L.DP);
    const dim3 nb((unsigned)(a.L.DP / GRA));
    if (stamps)
        hipLaunchKernelGGL(pca_sweep_mid_stamped_kernel<KP>, nb, dim3(NTF), lds, ctx->stream, a, state,
                           P, t, ticket, (const double *)ctx->sweep_sf, stamps, stamp_level);
    else
        hipLaunchKernelGGL(pca_sweep_mid_kernel<KP>, nb, dim3(NTF), lds, ctx->stream, a, state, P, t,
                           ticket, (const double *)ctx->sweep_sf);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_pca_launch_sweep_mid(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                                 double a0t, double b0t, double a0a, double b0a, double *state,
                                 double *P, const vmp_sweep_tail &t, unsigned int *ticket,
                                 unsigned long long *stamps, int32_t stamp_level)
{
    small_args a;
    const int32_t rc = fill_small_args(ctx, a, D, K, n_total, x_prec, a0t, b0t, a0a, b0a);
    if (rc != VMP_OK) return rc;
    if (a.L.KP == 16) return launch_mid<16>(ctx, a, state, P, t, ticket, stamps, stamp_level);
    return launch_mid<32>(ctx, a, state, P, t, ticket, stamps, stamp_level);
}

int32_t vmp_pca_sweep_constants(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                                double a0t, double b0t, double a0a, double b0a)
{
    small_args a;
    const int32_t rc = fill_small_args(ctx, a, D, K, n_total, x_prec, a0t, b0t, a0a, b0a);
    if (rc != VMP_OK) return rc;
    const double key[7] = {a0t, b0t, a0a, b0a, (double)D, (double)n_total, x_prec};
    if (ctx->sweep_sf && ctx->sweep_sf_valid && memcmp(key, ctx->sweep_sf_key, sizeof(key)) == 0)
        return VMP_OK;
    if (!ctx->sweep_sf) VMP_HIP_CHECK(ctx, hipMalloc(&ctx->sweep_sf, VMP_SWEEP_SF_LEN * sizeof(double)));
    // on the stream, ahead of the chunk that reads the values and behind every launch that read the old ones
    ctx->sweep_sf_valid = 0;
    hipLaunchKernelGGL(pca_sweep_sf_kernel, dim3(1), dim3(64), 0, ctx->stream, a, ctx->sweep_sf);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    memcpy(ctx->sweep_sf_key, key, sizeof(key));
    ctx->sweep_sf_valid = 1;
    return VMP_OK;
}

int32_t vmp_pca_launch_sweep_head_wide(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total,
                                       double x_prec, double a0t, double b0t, double a0a, double b0a,
                                       double *state)
{
    small_args a;
    const int32_t rc = fill_small_args(ctx, a, D, K, n_total, x_prec, a0t, b0t, a0a, b0a);
    if (rc != VMP_OK) return rc;
    if (a.L.KP == 16)
        hipLaunchKernelGGL(pca_head_wide_kernel<16>, dim3(1), dim3(NTF), 0, ctx->stream, a, state);
    else
        hipLaunchKernelGGL(pca_head_wide_kernel<32>, dim3(1), dim3(NTF), 0, ctx->stream, a, state);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

extern "C" {

int32_t vmp_mfma_order_probe(vmp_ctx *ctx, int32_t form, int32_t ntiles, const double *A,
                             const double *B, const double *C, double *D)
{
    VMP_REQUIRE(ctx, ctx && A && B && C && D, VMP_ERR_INVALID, "null argument");
    VMP_REQUIRE(ctx, form == 0 || form == 1, VMP_ERR_INVALID, "form %d (0 or 1)", form);
    VMP_REQUIRE(ctx, ntiles >= 1 && ntiles <= (1 << 20), VMP_ERR_INVALID, "ntiles %d out of range",
                ntiles);
    if (form == 0)
        hipLaunchKernelGGL(mfma_order_probe_kernel<0>, dim3(1), dim3(64), 0, ctx->stream, ntiles, A, B, C, D);
    else
        hipLaunchKernelGGL(mfma_order_probe_kernel<1>, dim3(1), dim3(64), 0, ctx->stream, ntiles, A, B, C, D);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_pca_small_ops(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                          double a0_tau, double b0_tau, double a0_alpha, double b0_alpha,
                          int32_t nops, const int32_t *ops, double *state)
{
    return launch_small(ctx, D, K, n_total, x_prec, a0_tau, b0_tau, a0_alpha, b0_alpha, nops, ops,
                        state);
}

int32_t vmp_pca_small_ops_mean(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                               double a0_tau, double b0_tau, double a0_alpha, double b0_alpha,
                               int32_t nops, const int32_t *ops, int32_t has_mean, double *state)
{
    return launch_small(ctx, D, K, n_total, x_prec, a0_tau, b0_tau, a0_alpha, b0_alpha, nops, ops,
                        state, has_mean);
}

int32_t vmp_pca_update_w(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double *state)
{
    const int32_t op = VMP_PCA_OP_W;
    return launch_small(ctx, D, K, n_total, 0.0, 0.0, 0.0, 0.0, 0.0, 1, &op, state);
}

int32_t vmp_pca_prepare_x(vmp_ctx *ctx, int32_t D, int32_t K, double x_prec, double *state)
{
    const int32_t op = VMP_PCA_OP_XPREP;
    return launch_small(ctx, D, K, 0, x_prec, 0.0, 0.0, 0.0, 0.0, 1, &op, state);
}

int32_t vmp_pca_update_tau(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double a0,
                           double b0, double *state)
{
    const int32_t op = VMP_PCA_OP_TAU;
    return launch_small(ctx, D, K, n_total, 0.0, a0, b0, 0.0, 0.0, 1, &op, state);
}

int32_t vmp_pca_update_alpha(vmp_ctx *ctx, int32_t D, int32_t K, double a0, double b0,
                             double *state)
{
    const int32_t op = VMP_PCA_OP_ALPHA;
    return launch_small(ctx, D, K, 0, 0.0, 0.0, 0.0, a0, b0, 1, &op, state);
}

int32_t vmp_pca_lower_bound(vmp_ctx *ctx, int32_t D, int32_t K, int64_t n_total, double x_prec,
                            double a0_tau, double b0_tau, double a0_alpha, double b0_alpha,
                            double *state)
{
    const int32_t op = VMP_PCA_OP_ELBO;
    return launch_small(ctx, D, K, n_total, x_prec, a0_tau, b0_tau, a0_alpha, b0_alpha, 1, &op,
                        state);
}

}  // extern "C"
