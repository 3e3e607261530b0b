// vmp_hmm_seg.hip -- the segmented chain stage of the fused hidden-Markov-model block: the pass of
// vmp_hmm_wide.hip, parallel over time for few long chains.
//
// vmp_hmm_wide_pass walks a chain with 2 (T - 1) dependent steps on one lane group.  Here the
// chain is cut into segments of L transitions (vmp_hmm_seg_dev.h: the formulas, who owns what, the
// order of the additions):
//
//   hmms_transfer_kernel  log W_s[i, :] for every (chain, segment, start state i): KP lanes are one
//                         (segment, start state), lane j owns column j; the start states of a
//                         segment are neighbours in a workgroup and read the same e_t
//   hmms_scan_kernel      la at the segment starts, lb at the segment ends, log Z and the weight of
//                         the chain: one lane group per chain, S steps each way, log W_s of the step
//                         to come requested before the arithmetic of the present one
//   hmms_sweep_kernel     the loops of hmmw_chain_kernel inside every segment, started from the
//                         stored la and lb; four wavefronts share <log A> and its transpose in LDS
//
// The emission table, the statistics and the combine kernel are those of vmp_hmm_wide.hip, called
// through vmp_hmm_wide_dev.h.  With fixed labels the pass IS vmp_hmm_wide_pass.
#include "vmp_common.h"
#include "vmp_hmm_seg_dev.h"

namespace {

struct HmmsArgs {
    int64_t B, S, ipw;        // chains, segments of a chain, items of a workgroup of the sweep
    int T, K, L;
    const double *E;          // B T x KP, or null (no emission term)
    const double *la0, *lA;
    const uint8_t *mask;
    double *W;                // B S K x KP: log W less the segment's sum b
    double *laB, *lbB;        // B S x KP: la at the segment start, lb at the segment end
    double *seg;              // B S x 2: any step observed, sum b
    double *chain;            // B x 2: weight, weighted log Z
    double *aw;               // B x T x K: la on the way forward, gamma on the way back
    double *part;
    double *gamma, *z0, *zz;
};

template <int KP>
__device__ __forceinline__ double hmms_grp_max(double v)
{
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

template <int KP>
__device__ __forceinline__ double hmms_grp_sum(double v)
{
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the value of lane (j, group g) added over the groups in group order; valid in lanes < KP
template <int KP>
__device__ __forceinline__ double hmms_across_groups(double v, int lane)
{
    double t = v;
#pragma unroll
    for (int g = 1; g < 64 / KP; ++g) t += __shfl(v, (lane & (KP - 1)) + g * KP, 64);
    return t;
}

// ---- stage 1: the transfer of every (chain, segment, start state) ---------------------------------
// LDS: <log A> once per workgroup and one vector per lane group.  Item = (chain S + segment) K + i,
// 256 / KP consecutive items per round, so the groups of a round sit in at most two segments next
// to each other and read the same rows of E (one address per wavefront, the other wavefronts
// from the vector cache).  A group runs its own number of steps; nothing is exchanged between
// groups.
template <int KP>
__global__ __launch_bounds__(256) void hmms_transfer_kernel(HmmsArgs a)
{
    extern __shared__ double hmms_lds[];
    constexpr int GW = 256 / KP;
    const int T = a.T, K = a.K, L = a.L;
    double *As = hmms_lds;                 // [i * KP + j]
    double *vec = As + KP * KP;            // [thread] = v of (group, i)
    const int tid = threadIdx.x, grp = tid / KP, j = tid % KP;
    const bool act = j < K;
    for (int e = tid; e < KP * KP; e += 256) {
        const int i = e / KP, c = e % KP;
        As[e] = (i < K && c < K) ? a.lA[i * K + c] : -INFINITY;
    }
    __syncthreads();
    double *myv = vec + grp * KP;
    const double *Acol = As + j;
    const int64_t nitem = a.B * a.S * K;
    for (int64_t it0 = (int64_t)blockIdx.x * GW; it0 < nitem; it0 += (int64_t)gridDim.x * GW) {
        const int64_t it = it0 + grp;
        if (it >= nitem) continue;                     // the whole group leaves
        const int i = (int)(it % K);
        const int64_t bs = it / K, cc = bs / a.S;
        const int s = (int)(bs % a.S);
        const int n0 = s * L, n1 = (n0 + L < T - 1) ? n0 + L : T - 1;
        const double *Ec = a.E ? a.E + cc * (int64_t)T * KP + j : nullptr;
        auto emit = [&](int t) -> double { return Ec ? Ec[(int64_t)t * KP] : 0.0; };
        const uint8_t *mrow = a.mask ? a.mask + cc * (int64_t)T : nullptr;
        int any = (mrow && s == 0) ? mrow[0] : 0;
        double v = (j == i) ? 0.0 : -INFINITY;
        double scale = 0.0, bsum = 0.0;
        double e_next = emit(n0 + 1);
        for (int n = n0 + 1; n <= n1; ++n) {
            const double e = e_next;
            if (n < n1) e_next = emit(n + 1);
            if (mrow) any |= mrow[n];
            myv[j] = v;
            lds_fence();
            double m, sm;
            vmp_hmmf_column(myv, Acol, KP, K, &m, &sm);
            double b = hmms_grp_max<KP>(act ? e : -INFINITY);
            if (b == -INFINITY) b = 0.0;
            const double q = act ? m + log(sm) + (e - b) : -INFINITY;
            const double M = hmms_grp_max<KP>(q);
            const double Sm = hmms_grp_sum<KP>(vmp_hmmf_exp_shift(q, M));
            const double cn = M + log(Sm);
            // nothing reachable from i: the row of W stays -inf, no NaN from -inf - -inf
            if (M != -INFINITY) scale += cn;
            v = (q == -INFINITY) ? -INFINITY : q - cn;
            bsum += b;
            lds_fence();
        }
        a.W[(bs * K + i) * KP + j] = (v == -INFINITY) ? -INFINITY : scale + v;
        if (i == 0 && j == 0) {
            a.seg[bs * 2] = (!mrow || any != 0) ? 1.0 : 0.0;
            a.seg[bs * 2 + 1] = bsum;
        }
    }
}

// ---- stage 2: the boundary scan ---------------------------------------------------------------------
// One wavefront, 64 / KP chains.  Forward, lane j holds column j of log W_s (KP registers), the
// column of the next segment is requested first; backward it holds row j.
template <int KP>
__global__ __launch_bounds__(64) void hmms_scan_kernel(HmmsArgs a)
{
    __shared__ double vec[64];
    constexpr int G = 64 / KP;
    const int T = a.T, K = a.K;
    const int64_t S = a.S;
    const int lane = threadIdx.x, grp = lane / KP, j = lane % KP;
    const bool act = j < K;
    const int64_t cc = (int64_t)blockIdx.x * G + grp;
    if (cc >= a.B) return;                             // the whole group leaves
    double *myv = vec + grp * KP;
    const double *seg = a.seg + cc * S * 2;
    int any = 0;
    for (int64_t s = j; s < S; s += KP) any |= seg[s * 2] != 0.0 ? 1 : 0;
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) any |= __shfl_xor(any, m, 64);
    const double w = any ? 1.0 : 0.0;

    const double *Wc = a.W + cc * S * K * KP;
    double la = act ? a.la0[j] + (a.E ? a.E[cc * (int64_t)T * KP + j] : 0.0) : -INFINITY;
    double logZ = 0.0;
    double wn[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) wn[i] = i < K ? Wc[(int64_t)i * KP + j] : -INFINITY;
    for (int64_t s = 0; s < S; ++s) {
        double wc[KP];
#pragma unroll
        for (int i = 0; i < KP; ++i) wc[i] = wn[i];
        if (s + 1 < S) {
#pragma unroll
            for (int i = 0; i < KP; ++i)
                if (i < K) wn[i] = Wc[((s + 1) * K + i) * KP + j];
        }
        a.laB[(cc * S + s) * KP + j] = la;
        myv[j] = la;
        lds_fence();
        double m = -INFINITY;
#pragma unroll
        for (int i = 0; i < KP; ++i) m = fmax(m, myv[i] + wc[i]);
        double sm = 0.0;
#pragma unroll
        for (int i = 0; i < KP; ++i) sm += vmp_hmmf_exp_shift(myv[i] + wc[i], m);
        const double q = act ? m + log(sm) : -INFINITY;
        const double M = hmms_grp_max<KP>(q);
        const double Sm = hmms_grp_sum<KP>(vmp_hmmf_exp_shift(q, M));
        const double cn = M + log(Sm);
        logZ += (cn + seg[s * 2 + 1]) * w;
        la = q - cn;
        lds_fence();
    }
    // backward: row min(j, K - 1) keeps the padded lanes inside W; their lb is never used
    const int jr = act ? j : K - 1;
    double lb = act ? 0.0 : -INFINITY;
#pragma unroll
    for (int c = 0; c < KP; ++c) wn[c] = Wc[((S - 1) * K + jr) * KP + c];
    for (int64_t s = S - 1; s >= 0; --s) {
        a.lbB[(cc * S + s) * KP + j] = lb;
        if (s == 0) break;
        double wc[KP];
#pragma unroll
        for (int c = 0; c < KP; ++c) wc[c] = wn[c];
        // the row of the segment before this one is what the step after this one reads
#pragma unroll
        for (int c = 0; c < KP; ++c) wn[c] = Wc[((s - 1) * K + jr) * KP + c];
        myv[j] = act ? lb : -INFINITY;
        lds_fence();
        double m = -INFINITY;
#pragma unroll
        for (int c = 0; c < KP; ++c) m = fmax(m, wc[c] + myv[c]);
        double sm = 0.0;
#pragma unroll
        for (int c = 0; c < KP; ++c) sm += vmp_hmmf_exp_shift(wc[c] + myv[c], m);
        const double lbn = act ? m + log(sm) : -INFINITY;
        lb = lbn - hmms_grp_max<KP>(lbn);
        lds_fence();
    }
    if (j == 0) {
        a.chain[cc * 2] = w;
        a.chain[cc * 2 + 1] = logZ;
    }
}

// ---- stage 3: the sweep inside every segment --------------------------------------------------------
// The recursion, the lane mapping and the order inside a step of hmmw_chain_kernel.  Registers: the
// column of sum xi and the exponentials of the step (KP doubles each); LDS: <log A>, its transpose
// and the la / u vectors of the four wavefronts; the partial of the workgroup is added up in the
// place of <log A> once every wavefront is done with it.
template <int KP>
__global__ __launch_bounds__(64 * VMP_HMMS_WAVES) void hmms_sweep_kernel(HmmsArgs a)
{
    extern __shared__ double hmms_lds[];
    constexpr int G = 64 / KP, WV = VMP_HMMS_WAVES;
    const int T = a.T, K = a.K, L = a.L;
    const int64_t S = a.S;
    double *As = hmms_lds;                 // [i * KP + j]
    double *ATs = As + KP * KP;            // [j * KP + i]
    double *vec = ATs + KP * KP;           // [thread] = la of (wavefront, group, i)
    double *uvec = vec + 64 * WV;          // [thread] = u of (wavefront, group, j)
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane / KP, j = lane % KP;
    const bool act = j < K;
    for (int e = tid; e < KP * KP; e += 64 * WV) {
        const int i = e / KP, c = e % KP;
        const double v = (i < K && c < K) ? a.lA[i * K + c] : -INFINITY;
        As[e] = v;
        ATs[c * KP + i] = v;
    }
    __syncthreads();
    double *myv = vec + wave * 64 + grp * KP, *myu = uvec + wave * 64 + grp * KP;
    const double *Acol = As + j, *ATcol = ATs + j;

    double xi[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) xi[i] = 0.0;
    double z0acc = 0.0, logZ = 0.0, ge = 0.0;

    const int64_t nitem = a.B * S;
    const int64_t i_begin = (int64_t)blockIdx.x * a.ipw;
    const int64_t i_end = (i_begin + a.ipw < nitem) ? i_begin + a.ipw : nitem;
    for (int64_t it0 = i_begin + wave * G; it0 < i_end; it0 += WV * G) {
        const int64_t it = it0 + grp;
        if (it >= i_end) continue;                     // the whole group leaves
        const int64_t cc = it / S;
        const int s = (int)(it % S);
        const int n0 = s * L, n1 = (n0 + L < T - 1) ? n0 + L : T - 1;
        const double w = a.chain[cc * 2];
        double *aw = a.aw + cc * (int64_t)T * K;
        const double *Ec = a.E ? a.E + cc * (int64_t)T * KP + j : nullptr;
        auto emit = [&](int t) -> double { return Ec ? Ec[(int64_t)t * KP] : 0.0; };
        // ---- forward from la at n0: e of step n + 1 is requested before the arithmetic of step n
        const double la_start = a.laB[it * KP + j];
        double la = la_start;
        double e_next = emit(n0 + 1);
        for (int n = n0 + 1; n <= n1; ++n) {
            const double e = e_next;
            if (n < n1) e_next = emit(n + 1);
            myv[j] = la;
            lds_fence();
            double m, sm;
            vmp_hmmf_column(myv, Acol, KP, K, &m, &sm);
            const double q = act ? m + log(sm) + e : -INFINITY;
            const double M = hmms_grp_max<KP>(q);
            const double Sm = hmms_grp_sum<KP>(vmp_hmmf_exp_shift(q, M));
            la = q - (M + log(Sm));
            if (act) aw[(int64_t)n * K + j] = la;
            lds_fence();
        }
        // ---- backward from lb at n1: gamma_{n+1} goes where la_{n+1} stood; la_n and e_{n+1} of
        // the step to come are requested first.  aw[n K + j], n0 < n <= n1, was written by this
        // lane; la at n0 is the stored boundary value. -------------------------------------------
        double lb = a.lbB[it * KP + j];
        double la_next = la;
        double e = emit(n1);
        double lan = (n1 - 1 > n0) ? (act ? aw[(int64_t)(n1 - 1) * K + j] : -INFINITY) : la_start;
        for (int n = n1 - 1; n >= n0; --n) {
            double e_prev = 0.0, lan_prev = -INFINITY;
            if (n > n0) {
                e_prev = emit(n);
                lan_prev = (n - 1 > n0) ? (act ? aw[(int64_t)(n - 1) * K + j] : -INFINITY) : la_start;
            }
            const double gl = act ? la_next + lb : -INFINITY;
            const double M = hmms_grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, M);
            const double gamma = ex / hmms_grp_sum<KP>(ex);
            myv[j] = lan;
            myu[j] = act ? e + lb : -INFINITY;
            lds_fence();
            double m = -INFINITY;
#pragma unroll
            for (int i = 0; i < KP; ++i) m = fmax(m, myv[i] + Acol[i * KP]);
            double p[KP];
            double sm = 0.0;
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                p[i] = vmp_hmmf_exp_shift(myv[i] + Acol[i * KP], m);
                sm += p[i];
            }
            const double r = vmp_hmmf_ratio(gamma, sm);
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                const double x = p[i] * r;
                xi[i] += x * w;
                if (a.zz && act && i < K)
                    a.zz[((cc * (int64_t)(T - 1) + n) * K + i) * K + j] = x;
            }
            if (gamma * w != 0.0) ge += gamma * w * e;
            if (act) aw[(int64_t)(n + 1) * K + j] = gamma;
            if (a.gamma && act) a.gamma[(cc * (int64_t)T + n + 1) * K + j] = gamma;
            double mr, sr;
            vmp_hmmf_column(myu, ATcol, KP, K, &mr, &sr);
            const double lbn = act ? mr + log(sr) : -INFINITY;
            lb = lbn - hmms_grp_max<KP>(lbn);
            la_next = lan;
            lan = lan_prev;
            e = e_prev;
            lds_fence();
        }
        if (s == 0) {
            // step 0 and log Z of the chain belong to its first segment
            e = emit(0);
            const double gl = act ? la_next + lb : -INFINITY;
            const double M = hmms_grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, M);
            const double gamma = ex / hmms_grp_sum<KP>(ex);
            z0acc += gamma * w;
            if (gamma * w != 0.0) ge += gamma * w * e;
            if (act) aw[j] = gamma;
            if (a.gamma && act) a.gamma[cc * (int64_t)T * K + j] = gamma;
            if (a.z0 && act) a.z0[cc * K + j] = gamma;
            logZ += a.chain[cc * 2 + 1];
        }
    }

    // ---- the partial of this workgroup: groups in group order, wavefronts in wavefront order ----
    const int64_t per = vmp_hmmw_chain_partial_doubles(K);
    double *red = hmms_lds;                 // per <= 2 KP KP + 2: inside <log A> and the vectors
    __syncthreads();                        // every wavefront is done with <log A>
    for (int wv = 0; wv < WV; ++wv) {
        if (wave == wv) {
            const double z0s = hmms_across_groups<KP>(z0acc, lane);
            if (lane < K) red[lane] = wv ? red[lane] + z0s : z0s;
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                const double v = hmms_across_groups<KP>(xi[i], lane);
                if (i < K && lane < K) red[K + i * K + lane] = wv ? red[K + i * K + lane] + v : v;
            }
            // log Z is the same in every lane of a group; gamma . e is a lane's own share
            double zs = 0.0, gs = 0.0;
            for (int g = 0; g < G; ++g) zs += __shfl(logZ, g * KP, 64);
            for (int l = 0; l < 64; ++l) gs += __shfl(ge, l, 64);
            if (lane == 0) {
                red[per - 2] = wv ? red[per - 2] + zs : zs;
                red[per - 1] = wv ? red[per - 1] + gs : gs;
            }
        }
        __syncthreads();
    }
    double *part = a.part + (int64_t)blockIdx.x * per;
    for (int64_t e = tid; e < per; e += 64 * WV) part[e] = red[e];
}

template <int KP>
int32_t launch_seg(vmp_ctx *ctx, int64_t nws, const HmmsArgs &a)
{
    const size_t lds1 = (size_t)(KP * KP + 256) * sizeof(double);
    const size_t lds3 = (size_t)(2 * KP * KP + 128 * VMP_HMMS_WAVES) * sizeof(double);
    static bool raised[64] = {false};
    const int dev = ctx->device & 63;
    if (lds3 > 48 * 1024 && !raised[dev]) {
        VMP_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)hmms_sweep_kernel<KP>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               160 * 1024));
        raised[dev] = true;
    }
    const int64_t rounds = (a.B * a.S * a.K + 256 / KP - 1) / (256 / KP);
    const int64_t g1 = rounds < VMP_HMMS_MAX_TRANSFER_WGS ? rounds : VMP_HMMS_MAX_TRANSFER_WGS;
    hipLaunchKernelGGL((hmms_transfer_kernel<KP>), dim3((unsigned)g1), dim3(256), lds1, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    const int64_t g2 = (a.B + 64 / KP - 1) / (64 / KP);
    hipLaunchKernelGGL((hmms_scan_kernel<KP>), dim3((unsigned)g2), dim3(64), 0, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL((hmms_sweep_kernel<KP>), dim3((unsigned)nws), dim3(64 * VMP_HMMS_WAVES), lds3,
                       ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // namespace

extern "C" {

int32_t vmp_hmm_seg_limits(int32_t *max_K, int32_t *max_D)
{
    if (!max_K || !max_D) return VMP_ERR_INVALID;
    *max_K = VMP_HMMS_MAX_K;
    *max_D = VMP_HMMS_MAX_D;
    return VMP_OK;
}

int32_t vmp_hmm_seg_plan(int64_t B, int32_t T, int32_t D, int32_t K, int32_t seg_len,
                         int32_t *seg_len_used, int64_t *workspace_doubles)
{
    if (B < 0 || T < 2 || D < 1 || K < 1 || seg_len < 0 || !seg_len_used || !workspace_doubles)
        return VMP_ERR_INVALID;
    if (K > VMP_HMMS_MAX_K || D > VMP_HMMS_MAX_D) return VMP_ERR_UNSUPPORTED;
    if (seg_len == 0) {
        const int tuned = vmp_tune_get("hmm_seg_len", 0);
        if (tuned > 0) seg_len = tuned;
    }
    *seg_len_used = vmp_hmms_clamp_len(B, T, K, seg_len);
    *workspace_doubles = vmp_hmms_workspace_doubles(B, T, D, K, *seg_len_used);
    return VMP_OK;
}

int32_t vmp_hmm_seg_pass(vmp_ctx *ctx, int64_t B, int32_t T, int32_t D, int32_t K,
                         const double *Y, const double *C, int32_t ldc, const double *elog_a0,
                         const double *elog_A, const int32_t *labels, const uint8_t *mask,
                         double *ws, double *z0sum, double *xisum, double *Tstat, double *scal,
                         double *gamma, double *z0, double *zz, int32_t seg_len)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, B >= 0 && T >= 2 && D >= 1 && K >= 1 && seg_len >= 0, VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_HMMS_MAX_K && D <= VMP_HMMS_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_HMMS_MAX_D, VMP_HMMS_MAX_K);
    const int NF = vmp_hmmf_nfeat(D);
    VMP_REQUIRE(ctx, !C || ldc >= NF, VMP_ERR_INVALID, "ldc = %d is below the %d features", ldc, NF);
    VMP_REQUIRE(ctx, ctx && elog_a0 && elog_A && ws && z0sum && xisum && Tstat && scal
                     && (B == 0 || Y), VMP_ERR_INVALID, "null argument");
    // fixed states: the one-hot path of the wide pass, and its bits (the workspace covers it)
    if (labels)
        return vmp_hmm_wide_pass(ctx, B, T, D, K, Y, C, ldc, elog_a0, elog_A, labels, mask, ws,
                                 z0sum, xisum, Tstat, scal, gamma, z0, zz);
    VMP_FLUSH_SMALL(ctx);
    int32_t L = 0;
    int64_t wsd = 0;
    int32_t rc = vmp_hmm_seg_plan(B, T, D, K, seg_len, &L, &wsd);
    if (rc != VMP_OK) return rc;
    const int KP = vmp_hmmf_kpad(K);
    const int64_t R = B * (int64_t)T, S = vmp_hmms_segments(T, L), BS = B * S;
    const int64_t nws = vmp_hmms_sweep_wgs(B, T, K, L), nwr = vmp_hmmw_row_wgs(R, D, K);
    const int64_t per = vmp_hmmw_chain_partial_doubles(K);
    double *E = ws, *aw = E + R * KP, *cpart = aw + R * K, *spart = cpart + nws * per;
    double *dot_ws = spart + nwr * (int64_t)K * NF;
    double *W = dot_ws + 1024, *laB = W + BS * K * KP, *lbB = laB + BS * KP, *seg = lbB + BS * KP;
    double *chain = seg + 2 * BS;
    if (R > 0) {
        if (C) {
            rc = vmp_hmmw_emit(ctx, R, D, K, Y, C, ldc, mask, E);
            if (rc != VMP_OK) return rc;
        }
        HmmsArgs sa = {B, S, vmp_hmms_items_per_wg(B, T, K, L), T, K, L, C ? E : nullptr, elog_a0,
                       elog_A, mask, W, laB, lbB, seg, chain, aw, cpart, gamma, z0, zz};
        switch (KP) {
        case 2: rc = launch_seg<2>(ctx, nws, sa); break;
        case 4: rc = launch_seg<4>(ctx, nws, sa); break;
        case 8: rc = launch_seg<8>(ctx, nws, sa); break;
        case 16: rc = launch_seg<16>(ctx, nws, sa); break;
        case 32: rc = launch_seg<32>(ctx, nws, sa); break;
        default: rc = launch_seg<64>(ctx, nws, sa); break;
        }
        if (rc != VMP_OK) return rc;
        rc = vmp_hmmw_stats(ctx, R, D, K, Y, aw, mask, spart);
        if (rc != VMP_OK) return rc;
    }
    return vmp_hmmw_combine(ctx, nws, nwr, D, K, cpart, spart, elog_a0, elog_A, dot_ws, z0sum,
                            xisum, Tstat, scal);
}

}  // extern "C"
