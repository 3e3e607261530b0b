// vmp_hmm_cat.hip -- the chain pass of the fused hidden-Markov-model block with categorical
// emissions (the discrete HMM of doc/source/examples/hmm.rst, first half)
//
//     Z = CategoricalMarkovChain(a0, A, states=T);  Y = Mixture(Z, Categorical, P);  Y.observe(y)
//
// The recursion, its log-domain form, the lane mapping and the order of every addition are those
// of the Gaussian pass (vmp_hmm_fused.hip) and are stated once, in vmp_hmm_fused_dev.h, whose
// per-step functions this file calls.  One kernel text for both families was tried first
// (hmmf_pass_kernel templated on the type of its arguments, the emission side in
// `if constexpr` branches): the Gaussian instances kept their occupancy, accumulator registers and
// zero scratch, but the vector registers of five of the twelve moved (unmasked KP = 4, 8, 16:
// 135 -> 131, 157 -> 150, 210 -> 199; masked KP = 8, 16: 159 -> 161, 208 -> 210).
// By the rule set for this change a moved figure keeps the Gaussian kernel text exactly as it
// was, so the categorical pass is a kernel of its own; only the emission side differs:
//   emission   e_t[j] = elogPt[y_t * K + j]: one load per lane and step from the word-major
//              table (M x K doubles, <= 64 KB, resident in L2).  No features, no LDS staging and
//              none of the fences that go with them.  A masked step has e = 0 and reads neither
//              y_t nor the table; so does a step whose word is outside [0, M)
//              (vmp_hmmf_cat_observed): such a word never becomes an address.
//   counts     S[m][j] = sum over the observed (b, t) with y = m of gamma_{b,t}[j]: one private
//              histogram per lane in LDS, sacc[m * 64 + lane] -- the bank depends on the lane
//              alone, so the update is conflict-free, and lane groups that hold different chains
//              and meet the same word never share an address: no LDS atomic, and the bits depend
//              on the inputs and (B, T, M, K) only.
// LDS: <log A> and its transpose (2 KP^2 doubles), the histograms (64 M doubles) and the la / u
// vectors (128 doubles) and, at KP = 64, half of the lane's column of sum xi (2048 doubles); at
// KP = 64, M = 128 that is 145 KB of the 160 KB of a CU.
//
// No atomics: a workgroup (one wavefront) owns a fixed range of chains and leaves one partial;
// hmmc_combine_kernel adds the partials in workgroup order.
#include <mutex>

#include "vmp_common.h"
#include "vmp_hmm_fused_dev.h"

namespace {

struct HmmcArgs {
    int64_t B, cpw;
    int T, M, K;
    const int32_t *y;         // B x T words
    const double *P;          // M x K <log P>, word-major, or null (no emission term)
    const double *la0;        // K
    const double *lA;         // K x K
    const int32_t *labels;    // B x T, or null
    const uint8_t *mask;      // B x T, 1 = observed, or null
    double *aw;               // B x T x K forward state
    double *part;             // workgroups x vmp_hmmf_cat_partial_doubles
    double *gamma, *z0, *zz;  // optional outputs
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

// entries of a lane's column of sum xi that are held in registers (the others: LDS)
constexpr int hmmc_xi_regs(int KP) { return KP < 64 ? KP : 32; }

// dynamic LDS of the pass in doubles
constexpr size_t hmmc_lds_doubles(int KP, int M)
{
    return (size_t)2 * KP * KP + (size_t)M * 64 + 128 + (size_t)(KP - hmmc_xi_regs(KP)) * 64;
}

// The mask and the range check only select values and skip a lane's own accumulation: lane groups
// hold chains with different masks and words, and every fence and shuffle stays in
// wavefront-uniform control flow.
template <int KP>
__global__ __launch_bounds__(64) void hmmc_pass_kernel(HmmcArgs a)
{
    extern __shared__ double hmmc_lds[];
    constexpr int G = 64 / KP, XR = hmmc_xi_regs(KP);
    const int T = a.T, M = a.M, K = a.K;
    double *As = hmmc_lds;                 // [i * KP + j]
    double *ATs = As + KP * KP;            // [j * KP + i]
    double *sacc = ATs + KP * KP;          // [m * 64 + lane]
    double *vec = sacc + (size_t)M * 64;   // [lane] = la of (group, i)
    double *uvec = vec + 64;               // [lane] = u of (group, j)
    double *xil = uvec + 64;               // [(i - XR) * 64 + lane], KP - XR rows
    const int lane = threadIdx.x, grp = lane / KP, j = lane % KP;
    const bool act = j < K;

    for (int e = lane; e < KP * KP; e += 64) {
        const int i = e / KP, c = e % KP;
        const double v = (i < K && c < K) ? a.lA[i * K + c] : -INFINITY;
        As[e] = v;
        ATs[c * KP + i] = v;
    }
    for (int e = lane; e < M * 64; e += 64) sacc[e] = 0.0;
    for (int e = lane; e < (KP - XR) * 64; e += 64) xil[e] = 0.0;
    lds_fence();

    double *myv = vec + grp * KP, *myu = uvec + grp * KP;
    const double *Acol = As + j, *ATcol = ATs + j;
    const double la0 = act ? a.la0[j] : -INFINITY;

    // the lane's column of sum xi: XR entries in registers and, at KP = 64, the other 32 in LDS
    // (xil[(i - XR) * 64 + lane], conflict-free): with all 64 in registers beside the 64
    // exponentials of a step that instance needs 404 bytes of scratch memory per lane
    double xi[XR];
#pragma unroll
    for (int i = 0; i < XR; ++i) xi[i] = 0.0;
    auto xi_add = [&](int i, double v) {       // i is a constant of an unrolled loop
        if (i < XR) xi[i < XR ? i : 0] += v;
        else xil[(i - XR) * 64 + lane] += v;
    };
    double z0acc = 0.0, logZ = 0.0, ge = 0.0;

    const int64_t c_begin = (int64_t)blockIdx.x * a.cpw;
    const int64_t c_end = (c_begin + a.cpw < a.B) ? c_begin + a.cpw : a.B;
    for (int64_t c0 = c_begin; c0 < c_end; c0 += G) {
        const int64_t c = c0 + grp;
        const bool live = c < c_end;
        const int64_t cc = live ? c : c_begin;
        const bool store = live && act;
        const int32_t *yrow = a.y + cc * (int64_t)T;
        const uint8_t *mrow = a.mask ? a.mask + cc * (int64_t)T : nullptr;
        // the chain's weight: 0 past the end of the range and without an observed step
        double w = live ? 1.0 : 0.0;
        if (mrow) {
            int any = 0;
            for (int t = j; t < T; t += KP) any |= mrow[t];
#pragma unroll
            for (int m = 1; m < KP; m <<= 1) any |= __shfl_xor(any, m, 64);
            if (any == 0) w = 0.0;
        }
        // the word of step t, or -1 where the step is masked or the word is out of range
        auto word = [&](int t) -> int {
            if (mrow && mrow[t] == 0) return -1;
            const int32_t v = yrow[t];
            return vmp_hmmf_cat_observed(true, v, M) ? v : -1;
        };
        // this lane's e_t[j]
        auto emit = [&](int wd) -> double {
            return (wd >= 0 && a.P && act) ? a.P[(int64_t)wd * K + j] : 0.0;
        };
        // a lane's own sums: no fence and no shuffle in here
        auto accumulate = [&](double g, double e, int wd) {
            if (wd < 0) return;
            if (g != 0.0) ge += g * e;
            sacc[wd * 64 + lane] += g;
        };

        if (a.labels) {
            // fixed states: gamma and xi are one-hot, log Z = 0
            const int32_t *lab = a.labels + cc * (int64_t)T;
            int prev = -1;
            for (int t = 0; t < T; ++t) {
                const int cur = lab[t];
                const double g = (j == cur) ? 1.0 : 0.0;
                accumulate(g * w, 0.0, word(t));
                if (t == 0) {
                    z0acc += g * w;
                    if (a.z0 && store) a.z0[cc * K + j] = g;
                } else {
#pragma unroll
                    for (int i = 0; i < KP; ++i) {
                        const double x = (i == prev) ? g : 0.0;
                        xi_add(i, x * w);
                        if (a.zz && store && i < K)
                            a.zz[((cc * (int64_t)(T - 1) + (t - 1)) * K + i) * K + j] = x;
                    }
                }
                if (a.gamma && store) a.gamma[(cc * (int64_t)T + t) * K + j] = g;
                prev = cur;
            }
            continue;
        }

        double *aw = a.aw + cc * (int64_t)T * K;
        // ---- forward ---------------------------------------------------------------------------
        double la = la0 + emit(word(0));
        if (!act) la = -INFINITY;
        if (store) aw[j] = la;
        for (int n = 1; n < T; ++n) {
            myv[j] = la;
            const double e = emit(word(n));
            lds_fence();
            double m, s;
            vmp_hmmf_column(myv, Acol, KP, K, &m, &s);
            const double q = act ? m + log(s) + e : -INFINITY;
            const double Mx = grp_max<KP>(q);
            const double S = grp_sum<KP>(vmp_hmmf_exp_shift(q, Mx));
            const double cn = Mx + log(S);
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
            const int wd = word(n + 1);
            const double e = emit(wd);
            const double gl = act ? la_next + lb : -INFINITY;
            const double Mx = grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, Mx);
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
                xi_add(i, x * w);
                if (a.zz && store && i < K)
                    a.zz[((cc * (int64_t)(T - 1) + n) * K + i) * K + j] = x;
            }
            accumulate(gamma * w, e, wd);
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
            const int wd = word(0);
            const double e = emit(wd);
            const double gl = act ? la_next + lb : -INFINITY;
            const double Mx = grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, Mx);
            const double gamma = ex / grp_sum<KP>(ex);
            z0acc += gamma * w;
            accumulate(gamma * w, e, wd);
            if (a.gamma && store) a.gamma[cc * (int64_t)T * K + j] = gamma;
            if (a.z0 && store) a.z0[cc * K + j] = gamma;
        }
    }

    // ---- the partial of this workgroup: groups in group order -----------------------------------
    const int64_t per = vmp_hmmf_cat_partial_doubles(M, K);
    double *part = a.part + (int64_t)blockIdx.x * per;
    const double z0s = across_groups<KP>(z0acc, lane);
    if (lane < K) part[lane] = z0s;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        const double own = i < XR ? xi[i < XR ? i : 0] : xil[(i < XR ? 0 : i - XR) * 64 + lane];
        const double v = across_groups<KP>(own, lane);
        if (i < K && lane < K) part[K + i * K + lane] = v;
    }
    lds_fence();
    if (lane < K) {
        double *ps = part + K + K * K + lane;
        for (int m = 0; m < M; ++m) {
            double t = 0.0;
            for (int g = 0; g < G; ++g) t += sacc[m * 64 + g * KP + lane];
            ps[(int64_t)m * K] = t;
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

// one thread per element of a partial: the workgroups in order; the counts stay word-major
__global__ void __launch_bounds__(256)
hmmc_combine_kernel(int64_t nw, int M, int K, const double *__restrict__ part,
                    double *__restrict__ z0sum, double *__restrict__ xisum,
                    double *__restrict__ S, double *__restrict__ scal)
{
    const int64_t per = vmp_hmmf_cat_partial_doubles(M, K);
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per) return;
    double v = 0.0;
    for (int64_t w = 0; w < nw; ++w) v += part[w * per + e];
    const int64_t oS = K + (int64_t)K * K;
    if (e < K) {
        z0sum[e] = v;
    } else if (e < oS) {
        xisum[e - K] = v;
    } else if (e < per - 2) {
        S[e - oS] = v;
    } else {
        scal[e - (per - 2)] = v;
    }
}

template <int KP>
int32_t launch_pass(vmp_ctx *ctx, int64_t nw, const HmmcArgs &a)
{
    const size_t lds = hmmc_lds_doubles(KP, a.M) * sizeof(double);
    static std::once_flag raised[64];           // per instance and device; host threads may race
    if (lds > 48 * 1024) {
        hipError_t err = hipSuccess;
        std::call_once(raised[ctx->device & 63], [&] {
            err = hipFuncSetAttribute((const void *)hmmc_pass_kernel<KP>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        });
        VMP_HIP_CHECK(ctx, err);
    }
    hipLaunchKernelGGL((hmmc_pass_kernel<KP>), dim3((unsigned)nw), dim3(64), lds, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // namespace

extern "C" {

int32_t vmp_hmm_fused_cat_limits(int32_t *max_K, int32_t *max_M)
{
    if (!max_K || !max_M) return VMP_ERR_INVALID;
    *max_K = VMP_HMMF_MAX_K;
    *max_M = VMP_HMMF_MAX_M;
    return VMP_OK;
}

int32_t vmp_hmm_fused_cat_plan(int64_t B, int32_t T, int32_t M, int32_t K, int64_t *chains_per_wg,
                               int64_t *workspace_doubles)
{
    if (B < 0 || T < 2 || M < 1 || K < 1 || !chains_per_wg || !workspace_doubles)
        return VMP_ERR_INVALID;
    if (K > VMP_HMMF_MAX_K || M > VMP_HMMF_MAX_M) return VMP_ERR_UNSUPPORTED;
    *chains_per_wg = vmp_hmmf_cat_chains_per_wg(B, M, K);
    *workspace_doubles = vmp_hmmf_cat_workspace_doubles(B, T, M, K);
    return VMP_OK;
}

int32_t vmp_hmm_fused_pass_categorical(vmp_ctx *ctx, int64_t B, int32_t T, int32_t M, int32_t K,
                                       const int32_t *y, const double *elogPt,
                                       const double *elog_a0, const double *elog_A,
                                       const int32_t *labels, const uint8_t *mask, double *ws,
                                       double *z0sum, double *xisum, double *S, double *scal,
                                       double *gamma, double *z0, double *zz)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, B >= 0 && T >= 2 && M >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_HMMF_MAX_K && M <= VMP_HMMF_MAX_M, VMP_ERR_UNSUPPORTED,
                "M = %d, K = %d exceed the limits (%d, %d)", M, K, VMP_HMMF_MAX_M, VMP_HMMF_MAX_K);
    VMP_REQUIRE(ctx, ctx && elog_a0 && elog_A && ws && z0sum && xisum && S && scal
                     && (B == 0 || y), VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int64_t nw = vmp_hmmf_cat_wgs(B, M, K);
    const int64_t per = vmp_hmmf_cat_partial_doubles(M, K);
    double *part = ws + B * (int64_t)T * K;
    if (nw > 0) {
        HmmcArgs a = {B, vmp_hmmf_cat_chains_per_wg(B, M, K), T, M, K, y, elogPt, elog_a0, elog_A,
                      labels, mask, ws, part, gamma, z0, zz};
        int32_t rc;
        switch (vmp_hmmf_kpad(K)) {
        case 2: rc = launch_pass<2>(ctx, nw, a); break;
        case 4: rc = launch_pass<4>(ctx, nw, a); break;
        case 8: rc = launch_pass<8>(ctx, nw, a); break;
        case 16: rc = launch_pass<16>(ctx, nw, a); break;
        case 32: rc = launch_pass<32>(ctx, nw, a); break;
        default: rc = launch_pass<64>(ctx, nw, a); break;
        }
        if (rc != VMP_OK) return rc;
    }
    hipLaunchKernelGGL(hmmc_combine_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0,
                       ctx->stream, nw, M, K, part, z0sum, xisum, S, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    double *dot_ws = part + nw * per;
    int32_t rc = vmp_lda_dot(ctx, K, z0sum, elog_a0, dot_ws, scal + 2);
    if (rc != VMP_OK) return rc;
    return vmp_lda_dot(ctx, (int64_t)K * K, xisum, elog_A, dot_ws, scal + 3);
}

}  // extern "C"
