// vmp_hmm_fused.hip -- the chain pass of the fused hidden-Markov-model block
//
//     a0 = Dirichlet(c);  A = Dirichlet(c, plates=(K,));  Z = CategoricalMarkovChain(a0, A, states=T)
//     Y = Mixture(Z, Gaussian, mu, Lambda);  Y.observe(y)                (doc/source/examples/hmm.rst)
//
// The generic engine builds logP (B, T-1, K, K) = <log A> + emission log-likelihoods, lets
// vmp_alpha_beta_recursion (vmp_hmm.hip) read it twice and write zz of the same shape, and sums zz
// over the plates for the messages.  This pass reads y_t (D doubles) and keeps la_t (K doubles)
// per step; xi_t exists only in the registers of the lane that adds it to its column of sum xi.
// The recursion, its log-domain form and the order of every addition: vmp_hmm_fused_dev.h.
//
// Lane mapping (that of alpha_beta_kernel): KP lanes per chain, lane j owns column j, 64 / KP
// chains share a wavefront, one wavefront per workgroup.  Where things live:
//   registers  the column of sum xi (KP doubles) and the exponentials p_i of the current step
//              (KP doubles) -- both indexed by unrolled loops only;
//   LDS        <log A> and its transpose (2 KP^2), the emission coefficients (NF x KP, <= 23 KB),
//              the feature accumulators (NF x 64: a lane's own row of T, <= 23 KB), the la / u
//              vectors and the features of the step.
// Forward and the lb row sums are runtime loops over K; only the xi loop is unrolled over KP.
//
// No atomics: a workgroup owns a fixed range of chains and leaves one partial;
// hmmf_combine_kernel adds the partials in workgroup order.
#include "vmp_common.h"
#include "vmp_hmm_fused_dev.h"

namespace {

struct HmmfArgs {
    int64_t B, cpw;
    int T, D, K, NF, ldc;
    const double *Y;          // B x T x D
    const double *C;          // K x ldc compact coefficients, or null (no emission term)
    const double *la0;        // K
    const double *lA;         // K x K
    const int32_t *labels;    // B x T, or null
    double *aw;               // B x T x K forward state
    double *part;             // workgroups x vmp_hmmf_partial_doubles
    double *gamma, *z0, *zz;  // optional outputs
    const uint8_t *mask;      // B x T, 1 = observed (the MASKED instances only)
};

template <int KP>
__device__ __forceinline__ double grp_max(double v)
{
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

template <int KP>
__device__ __forceinline__ double grp_sum(double v)
{
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the value of lane (j, group g) added over the groups in group order; valid in lanes < KP
template <int KP>
__device__ __forceinline__ double across_groups(double v, int lane)
{
    double t = v;
#pragma unroll
    for (int g = 1; g < 64 / KP; ++g) t += __shfl(v, (lane & (KP - 1)) + g * KP, 64);
    return t;
}

// MASKED: a step with mask[b, t] == 0 has e = 0 and adds nothing to the feature sums or to
// sum gamma . e, and its y is never read; a chain without an observed step adds nothing to any sum.
// Lane groups hold chains with different masks, so the mask only selects values and skips a lane's
// own accumulation: every fence and shuffle stays in wavefront-uniform control flow.
//
// The MASKED instances are asked for 3, 3, 3, 2, 1, 1 wavefronts per SIMD at KP = 2 ... 64, those
// of their unmasked twins but for KP = 2: left alone, KP = 8 takes 169 registers, one more than
// three wavefronts allow; KP = 2 at the four of its twin would need scratch memory.
template <int KP, bool MASKED>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(
    MASKED ? (KP <= 8 ? 3 : KP == 16 ? 2 : 1) : 1)))
void hmmf_pass_kernel(HmmfArgs a)
{
    extern __shared__ double hmmf_lds[];
    constexpr int G = 64 / KP;
    const int T = a.T, D = a.D, K = a.K, NF = a.NF;
    double *As = hmmf_lds;                 // [i * KP + j]
    double *ATs = As + KP * KP;            // [j * KP + i]
    double *Cs = ATs + KP * KP;            // [f * KP + j]
    double *facc = Cs + NF * KP;           // [f * 64 + lane]
    double *vec = facc + NF * 64;          // [lane] = la of (group, i)
    double *uvec = vec + 64;               // [lane] = u of (group, j)
    double *ys = uvec + 64;                // [g * 9 + d], ys[g * 9 + D] = 1
    double *phis = ys + G * 9;             // [g * NF + f]
    int *fa = (int *)(phis + G * NF);      // factors of feature f
    int *fb = fa + VMP_HMMF_MAX_NF + 3;
    const int lane = threadIdx.x, grp = lane / KP, j = lane % KP;
    const bool act = j < K;

    for (int e = lane; e < KP * KP; e += 64) {
        const int i = e / KP, c = e % KP;
        const double v = (i < K && c < K) ? a.lA[i * K + c] : -INFINITY;
        As[e] = v;
        ATs[c * KP + i] = v;
    }
    for (int e = lane; e < NF * KP; e += 64) {
        const int f = e / KP, c = e % KP;
        Cs[e] = (a.C && c < K) ? a.C[(int64_t)c * a.ldc + f] : 0.0;
    }
    for (int e = lane; e < NF * 64; e += 64) facc[e] = 0.0;
    for (int f = lane; f < NF; f += 64) vmp_hmmf_feature(D, f, &fa[f], &fb[f]);
    if (j == 0) ys[grp * 9 + D] = 1.0;
    lds_fence();

    double *myv = vec + grp * KP, *myu = uvec + grp * KP;
    double *myy = ys + grp * 9, *myphi = phis + grp * NF;
    const double *Acol = As + j, *ATcol = ATs + j, *Ccol = Cs + j;
    const double la0 = act ? a.la0[j] : -INFINITY;

    double xi[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) xi[i] = 0.0;
    double z0acc = 0.0, logZ = 0.0, ge = 0.0;

    // features of y_t of this group's chain into myphi; returns this lane's e_t[j].  A masked
    // step (o false) loads zeros in place of y_t and returns 0.
    auto features = [&](const double *yt, bool o) -> double {
        if constexpr (MASKED) {
            for (int d = j; d < D; d += KP) myy[d] = o ? yt[d] : 0.0;
        } else {
            for (int d = j; d < D; d += KP) myy[d] = yt[d];
        }
        lds_fence();
        for (int f = j; f < NF; f += KP) myphi[f] = myy[fa[f]] * myy[fb[f]];
        lds_fence();
        const double e = a.C ? vmp_hmmf_emit(Ccol, KP, myphi, NF) : 0.0;
        if constexpr (MASKED) return vmp_hmmf_observed_or_zero(o, e);
        return e;
    };
    // a lane's own sums: no fence and no shuffle in here, so a masked step may skip it
    auto accumulate = [&](double g, double e, bool o) {
        if (MASKED && !o) return;
        if (g != 0.0) ge += g * e;
        for (int f = 0; f < NF; ++f) facc[f * 64 + lane] += g * myphi[f];
    };

    const int64_t c_begin = (int64_t)blockIdx.x * a.cpw;
    const int64_t c_end = (c_begin + a.cpw < a.B) ? c_begin + a.cpw : a.B;
    for (int64_t c0 = c_begin; c0 < c_end; c0 += G) {
        const int64_t c = c0 + grp;
        const bool live = c < c_end;
        const int64_t cc = live ? c : c_begin;
        const double wlive = live ? 1.0 : 0.0;
        const bool store = live && act;
        const double *Yc = a.Y + cc * (int64_t)T * D;
        // the chain's weight: 0 past the end of the range and, MASKED, without an observed step
        const uint8_t *mrow = MASKED ? a.mask + cc * (int64_t)T : nullptr;
        double wchain = wlive;
        if constexpr (MASKED) {
            int any = 0;
            for (int t = j; t < T; t += KP) any |= mrow[t];
#pragma unroll
            for (int m = 1; m < KP; m <<= 1) any |= __shfl_xor(any, m, 64);
            if (any == 0) wchain = 0.0;
        }
        const double w = wchain;
        auto obs = [&](int t) -> bool { return MASKED ? mrow[t] != 0 : true; };

        if (a.labels) {
            // fixed states: gamma and xi are one-hot, log Z = 0
            const int32_t *lab = a.labels + cc * (int64_t)T;
            int prev = -1;
            for (int t = 0; t < T; ++t) {
                const int cur = lab[t];
                const bool o = obs(t);
                features(Yc + (int64_t)t * D, o);
                const double g = (j == cur) ? 1.0 : 0.0;
                accumulate(g * w, 0.0, o);
                if (t == 0) {
                    z0acc += g * w;
                    if (a.z0 && store) a.z0[cc * K + j] = g;
                } else {
#pragma unroll
                    for (int i = 0; i < KP; ++i) {
                        const double x = (i == prev) ? g : 0.0;
                        xi[i] += x * w;
                        if (a.zz && store && i < K)
                            a.zz[((cc * (int64_t)(T - 1) + (t - 1)) * K + i) * K + j] = x;
                    }
                }
                if (a.gamma && store) a.gamma[(cc * (int64_t)T + t) * K + j] = g;
                prev = cur;
                lds_fence();
            }
            continue;
        }

        double *aw = a.aw + cc * (int64_t)T * K;
        // ---- forward ---------------------------------------------------------------------------
        double la = la0 + features(Yc, obs(0));
        if (!act) la = -INFINITY;
        if (store) aw[j] = la;
        for (int n = 1; n < T; ++n) {
            myv[j] = la;
            const double e = features(Yc + (int64_t)n * D, obs(n));      // fences the LDS writes
            double m, s;
            vmp_hmmf_column(myv, Acol, KP, K, &m, &s);
            const double q = act ? m + log(s) + e : -INFINITY;
            const double M = grp_max<KP>(q);
            const double S = grp_sum<KP>(vmp_hmmf_exp_shift(q, M));
            const double cn = M + log(S);
            logZ += cn * w;
            la = q - cn;
            if (store) aw[(int64_t)n * K + j] = la;
            lds_fence();
        }
        // the backward sweep reads la values stored by other lanes of this wavefront
        __threadfence_block();
        // ---- backward --------------------------------------------------------------------------
        double lb = 0.0;
        double la_next = la;
        for (int n = T - 2; n >= 0; --n) {
            const double lan = act ? aw[(int64_t)n * K + j] : -INFINITY;
            const bool o = obs(n + 1);
            const double e = features(Yc + (int64_t)(n + 1) * D, o);
            const double gl = act ? la_next + lb : -INFINITY;
            const double M = grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, M);
            const double gamma = ex / grp_sum<KP>(ex);
            myv[j] = lan;
            myu[j] = act ? e + lb : -INFINITY;
            lds_fence();
            double m = -INFINITY;
#pragma unroll
            for (int i = 0; i < KP; ++i) m = fmax(m, myv[i] + Acol[i * KP]);
            double p[KP];
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                p[i] = vmp_hmmf_exp_shift(myv[i] + Acol[i * KP], m);
                s += p[i];
            }
            const double r = vmp_hmmf_ratio(gamma, s);
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                const double x = p[i] * r;
                xi[i] += x * w;
                if (a.zz && store && i < K)
                    a.zz[((cc * (int64_t)(T - 1) + n) * K + i) * K + j] = x;
            }
            accumulate(gamma * w, e, o);
            if (a.gamma && store) a.gamma[(cc * (int64_t)T + n + 1) * K + j] = gamma;
            // lb_n[i] on lane i: the row of <log A> is a column of its transpose
            double mr, sr;
            vmp_hmmf_column(myu, ATcol, KP, K, &mr, &sr);
            const double lbn = act ? mr + log(sr) : -INFINITY;
            lb = lbn - grp_max<KP>(lbn);
            la_next = lan;
            lds_fence();
        }
        {
            const bool o = obs(0);
            const double e = features(Yc, o);
            const double gl = act ? la_next + lb : -INFINITY;
            const double M = grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, M);
            const double gamma = ex / grp_sum<KP>(ex);
            z0acc += gamma * w;
            accumulate(gamma * w, e, o);
            if (a.gamma && store) a.gamma[cc * (int64_t)T * K + j] = gamma;
            if (a.z0 && store) a.z0[cc * K + j] = gamma;
            lds_fence();
        }
    }

    // ---- the partial of this workgroup: groups in group order -----------------------------------
    const int64_t per = vmp_hmmf_partial_doubles(D, K);
    double *part = a.part + (int64_t)blockIdx.x * per;
    const double z0s = across_groups<KP>(z0acc, lane);
    if (lane < K) part[lane] = z0s;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        const double v = across_groups<KP>(xi[i], lane);
        if (i < K && lane < K) part[K + i * K + lane] = v;
    }
    lds_fence();
    if (lane < K) {
        double *pf = part + K + K * K + (int64_t)lane * NF;
        for (int f = 0; f < NF; ++f) {
            double t = 0.0;
            for (int g = 0; g < G; ++g) t += facc[f * 64 + g * KP + lane];
            pf[f] = t;
        }
    }
    // log Z is the same in every lane of a group; gamma . e is a lane's own share
    double zs = 0.0, gs = 0.0;
    for (int g = 0; g < G; ++g) zs += __shfl(logZ, g * KP, 64);
    for (int l = 0; l < 64; ++l) gs += __shfl(ge, l, 64);
    if (lane == 0) {
        part[per - 2] = zs;
        part[per - 1] = gs;
    }
}

// one thread per element of a partial: the workgroups in order; the feature sums go from the
// compact order to rows [1, y, y y^T] of length FS = 1 + D + D^2 (vmp_gmm_layout's T)
__global__ void __launch_bounds__(256)
hmmf_combine_kernel(int64_t nw, int D, int K, const double *__restrict__ part,
                    double *__restrict__ z0sum, double *__restrict__ xisum,
                    double *__restrict__ Tst, double *__restrict__ scal)
{
    const int64_t per = vmp_hmmf_partial_doubles(D, K);
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    double v = 0.0;
    for (int64_t w = 0; w < nw; ++w) v += part[w * per + e];
    const int NF = vmp_hmmf_nfeat(D), FS = 1 + D + D * D;
    if (e < K) {
        z0sum[e] = v;
    } else if (e < K + (int64_t)K * K) {
        xisum[e - K] = v;
    } else if (e < per - 2) {
        const int r = (int)(e - K - (int64_t)K * K);
        const int k = r / NF, f = r - k * NF;
        int pa, pb;
        vmp_hmmf_feature(D, f, &pa, &pb);
        double *Tk = Tst + (int64_t)k * FS;
        if (pb < D) {
            Tk[1 + D + pa * D + pb] = v;
            Tk[1 + D + pb * D + pa] = v;
        } else if (pa < D) {
            Tk[1 + pa] = v;
        } else {
            Tk[0] = v;
        }
    } else {
        scal[e - (per - 2)] = v;
    }
}

template <int KP, bool MASKED>
int32_t launch_pass(vmp_ctx *ctx, int64_t nw, const HmmfArgs &a)
{
    constexpr int G = 64 / KP;
    const size_t lds = (size_t)(2 * KP * KP + a.NF * KP + a.NF * 64 + 128 + G * 9 + G * a.NF)
                           * sizeof(double) + 2 * (VMP_HMMF_MAX_NF + 3) * sizeof(int);
    static bool raised[64] = {false};
    const int dev = ctx->device & 63;
    if (lds > 48 * 1024 && !raised[dev]) {
        VMP_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)hmmf_pass_kernel<KP, MASKED>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               160 * 1024));
        raised[dev] = true;
    }
    hipLaunchKernelGGL((hmmf_pass_kernel<KP, MASKED>), dim3((unsigned)nw), dim3(64), lds, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

template <bool MASKED>
int32_t launch_pass_kpad(vmp_ctx *ctx, int64_t nw, const HmmfArgs &a)
{
    switch (vmp_hmmf_kpad(a.K)) {
    case 2: return launch_pass<2, MASKED>(ctx, nw, a);
    case 4: return launch_pass<4, MASKED>(ctx, nw, a);
    case 8: return launch_pass<8, MASKED>(ctx, nw, a);
    case 16: return launch_pass<16, MASKED>(ctx, nw, a);
    case 32: return launch_pass<32, MASKED>(ctx, nw, a);
    default: return launch_pass<64, MASKED>(ctx, nw, a);
    }
}

}  // namespace

extern "C" {

int32_t vmp_hmm_fused_limits(int32_t *max_K, int32_t *max_D)
{
    if (!max_K || !max_D) return VMP_ERR_INVALID;
    *max_K = VMP_HMMF_MAX_K;
    *max_D = VMP_HMMF_MAX_D;
    return VMP_OK;
}

int32_t vmp_hmm_fused_plan(int64_t B, int32_t T, int32_t D, int32_t K, int64_t *chains_per_wg,
                           int64_t *workspace_doubles)
{
    if (B < 0 || T < 2 || D < 1 || K < 1 || !chains_per_wg || !workspace_doubles)
        return VMP_ERR_INVALID;
    if (K > VMP_HMMF_MAX_K || D > VMP_HMMF_MAX_D) return VMP_ERR_UNSUPPORTED;
    *chains_per_wg = vmp_hmmf_chains_per_wg(B, D, K);
    *workspace_doubles = vmp_hmmf_workspace_doubles(B, T, D, K);
    return VMP_OK;
}

int32_t vmp_hmm_fused_pass_masked(vmp_ctx *ctx, int64_t B, int32_t T, int32_t D, int32_t K,
                                  const double *Y, const double *C, int32_t ldc,
                                  const double *elog_a0, const double *elog_A,
                                  const int32_t *labels, const uint8_t *mask, double *ws,
                                  double *z0sum, double *xisum, double *Tstat, double *scal,
                                  double *gamma, double *z0, double *zz)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, B >= 0 && T >= 2 && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_HMMF_MAX_K && D <= VMP_HMMF_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_HMMF_MAX_D, VMP_HMMF_MAX_K);
    const int NF = vmp_hmmf_nfeat(D);
    VMP_REQUIRE(ctx, !C || ldc >= NF, VMP_ERR_INVALID, "ldc = %d is below the %d features", ldc, NF);
    VMP_REQUIRE(ctx, ctx && elog_a0 && elog_A && ws && z0sum && xisum && Tstat && scal
                     && (B == 0 || Y), VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int64_t nw = vmp_hmmf_wgs(B, D, K);
    const int64_t per = vmp_hmmf_partial_doubles(D, K);
    double *part = ws + B * (int64_t)T * K;
    if (nw > 0) {
        HmmfArgs a = {B, vmp_hmmf_chains_per_wg(B, D, K), T, D, K, NF, ldc, Y, C, elog_a0,
                      elog_A, labels, ws, part, gamma, z0, zz, mask};
        const int32_t rc = mask ? launch_pass_kpad<true>(ctx, nw, a)
                                : launch_pass_kpad<false>(ctx, nw, a);
        if (rc != VMP_OK) return rc;
    }
    hipLaunchKernelGGL(hmmf_combine_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0,
                       ctx->stream, nw, D, K, part, z0sum, xisum, Tstat, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    double *dot_ws = part + nw * per;
    int32_t rc = vmp_lda_dot(ctx, K, z0sum, elog_a0, dot_ws, scal + 2);
    if (rc != VMP_OK) return rc;
    return vmp_lda_dot(ctx, (int64_t)K * K, xisum, elog_A, dot_ws, scal + 3);
}

int32_t vmp_hmm_fused_pass(vmp_ctx *ctx, int64_t B, int32_t T, int32_t D, int32_t K,
                           const double *Y, const double *C, int32_t ldc, const double *elog_a0,
                           const double *elog_A, const int32_t *labels, double *ws,
                           double *z0sum, double *xisum, double *Tstat, double *scal,
                           double *gamma, double *z0, double *zz)
{
    return vmp_hmm_fused_pass_masked(ctx, B, T, D, K, Y, C, ldc, elog_a0, elog_A, labels, nullptr,
                                     ws, z0sum, xisum, Tstat, scal, gamma, z0, zz);
}

}  // extern "C"
