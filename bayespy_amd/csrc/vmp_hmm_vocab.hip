// vmp_hmm_vocab.hip -- the large-vocabulary pass of the fused hidden-Markov-model block with
// categorical emissions: the discrete HMM of vmp_hmm_cat.hip for vocabularies of up to 65536 words
//
//     Z = CategoricalMarkovChain(a0, A, states=T);  Y = Mixture(Z, Categorical, P);  Y.observe(y)
//
// vmp_hmm_cat.hip stops at M = 128 because every lane keeps a count histogram of M doubles in LDS.
// Here the count is taken out of the chain kernel, and nothing a workgroup owns grows with M:
//   hmmv_chain_kernel<KP>  the recursion alone -- the lane mapping, the arithmetic (through the
//        functions of vmp_hmm_fused_dev.h), the mask rules and the order of every addition of
//        hmmc_pass_kernel.  The emission e_t[j] = elogPt[y_t * K + j] is a gather from a table of
//        up to 32 MB that lives in L2 / Infinity Cache, so its latency is kept off the dependent
//        chain: in both directions the word of step n +- 2 and the table row of step n +- 1 (and,
//        on the way back, la of step n - 1) are requested before the exp / log arithmetic of
//        step n.  A masked step and a step whose word is outside [0, M) read neither word nor row.
//        gamma_t overwrites la_t in the (B, T, K) workspace.  A workgroup (one wavefront) leaves
//        K + K^2 + 2 doubles.  LDS: <log A>, its transpose, the la / u vectors and, at KP = 64,
//        entries 32 .. 63 of each lane's column of sum xi.
//   hmmv_count_kernel<KP>  S from the in-place gamma over the word layout: one lane group per
//        chunk, lane j adds one contiguous row of K doubles per entry (vmp_hmm_vocab_dev.h: the
//        walk, heads and tails).
//   hmmv_combine_kernel    the chain partials in workgroup order; per word the tail and heads of
//        its chunks in chunk order, zeros for a word that does not occur.
// No atomics, no scratch memory in any instance.
#include <mutex>

#include "vmp_common.h"
#include "vmp_hmm_vocab_dev.h"

namespace {

struct HmmvArgs {
    int64_t B, cpw;
    int T, M, K;
    const int32_t *y;         // B x T words
    const double *P;          // M x K <log P>, word-major, or null (no emission term)
    const double *la0;        // K
    const double *lA;         // K x K
    const int32_t *labels;    // B x T, or null
    const uint8_t *mask;      // B x T, 1 = observed, or null
    double *aw;               // B x T x K: la on the way forward, gamma when the kernel ends
    double *part;             // workgroups x vmp_hmmv_partial_doubles
    double *gamma, *z0, *zz;  // optional outputs
};

template <int KP>
__device__ __forceinline__ double hmmv_grp_max(double v)
{
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

template <int KP>
__device__ __forceinline__ double hmmv_grp_sum(double v)
{
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the value of lane (j, group g) added over the groups in group order; valid in lanes < KP
template <int KP>
__device__ __forceinline__ double hmmv_across_groups(double v, int lane)
{
    double t = v;
#pragma unroll
    for (int g = 1; g < 64 / KP; ++g) t += __shfl(v, (lane & (KP - 1)) + g * KP, 64);
    return t;
}

// entries of a lane's column of sum xi that are held in registers (the others: LDS)
constexpr int hmmv_xi_regs(int KP) { return KP < 64 ? KP : 32; }

constexpr size_t hmmv_lds_doubles(int KP)
{
    return (size_t)2 * KP * KP + 128 + (size_t)(KP - hmmv_xi_regs(KP)) * 64;
}

// The mask and the range check only select values and skip a lane's own accumulation: lane groups
// hold chains with different masks and words, and every fence and shuffle stays in
// wavefront-uniform control flow.
template <int KP>
__global__ __launch_bounds__(64) void hmmv_chain_kernel(HmmvArgs a)
{
    extern __shared__ double hmmv_lds[];
    constexpr int G = 64 / KP, XR = hmmv_xi_regs(KP);
    const int T = a.T, M = a.M, K = a.K;
    double *As = hmmv_lds;                 // [i * KP + j]
    double *ATs = As + KP * KP;            // [j * KP + i]
    double *vec = ATs + KP * KP;           // [lane] = la of (group, i)
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
    for (int e = lane; e < (KP - XR) * 64; e += 64) xil[e] = 0.0;
    lds_fence();

    double *myv = vec + grp * KP, *myu = uvec + grp * KP;
    const double *Acol = As + j, *ATcol = ATs + j;
    const double la0 = act ? a.la0[j] : -INFINITY;

    // the lane's column of sum xi: XR entries in registers and, at KP = 64, the other 32 in LDS
    // (conflict-free: the bank depends on the lane alone)
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
        double *aw = a.aw + cc * (int64_t)T * K;

        if (a.labels) {
            // fixed states: gamma and xi are one-hot, log Z = 0; gamma goes to the workspace for
            // the count kernel
            const int32_t *lab = a.labels + cc * (int64_t)T;
            int prev = -1;
            for (int t = 0; t < T; ++t) {
                const int cur = lab[t];
                const double g = (j == cur) ? 1.0 : 0.0;
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
                if (store) aw[(int64_t)t * K + j] = g;
                if (a.gamma && store) a.gamma[(cc * (int64_t)T + t) * K + j] = g;
                prev = cur;
            }
            continue;
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

        // ---- forward: the row of step n + 1 and the word of step n + 2 are requested before the
        // arithmetic of step n --------------------------------------------------------------------
        double la = la0 + emit(word(0));
        if (!act) la = -INFINITY;
        if (store) aw[j] = la;
        double e_next = emit(word(1));
        int wd_next = T > 2 ? word(2) : -1;             // the word of step n + 1 inside the loop
        for (int n = 1; n < T; ++n) {
            const double e = e_next;
            e_next = emit(wd_next);                     // -1 past the end: nothing is read
            wd_next = n + 2 < T ? word(n + 2) : -1;
            myv[j] = la;
            lds_fence();
            double m, s;
            vmp_hmmf_column(myv, Acol, KP, K, &m, &s);
            const double q = act ? m + log(s) + e : -INFINITY;
            const double Mx = hmmv_grp_max<KP>(q);
            const double S = hmmv_grp_sum<KP>(vmp_hmmf_exp_shift(q, Mx));
            const double cn = Mx + log(S);
            logZ += cn * w;
            la = q - cn;
            if (store) aw[(int64_t)n * K + j] = la;
            lds_fence();
        }
        // ---- backward: gamma_{n+1} goes where la_{n+1} stood.  Step n needs the word and row of
        // step n + 1 and la_n; the row of step n, la_{n-1} and the word of step n - 1 are requested
        // first.  aw[n K + j] was written by this lane. ---------------------------------------------
        double lb = 0.0;
        double la_next = la;
        int wd = word(T - 1);
        double e = emit(wd);
        int wd_prev = word(T - 2);
        double lan = act ? aw[(int64_t)(T - 2) * K + j] : -INFINITY;
        for (int n = T - 2; n >= 0; --n) {
            const double e_prev = emit(wd_prev);
            int wd_pp = -1;
            double lan_prev = -INFINITY;
            if (n > 0) {
                wd_pp = word(n - 1);
                if (act) lan_prev = aw[(int64_t)(n - 1) * K + j];
            }
            const double gl = act ? la_next + lb : -INFINITY;
            const double Mx = hmmv_grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, Mx);
            const double gamma = ex / hmmv_grp_sum<KP>(ex);
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
            if (wd >= 0 && gamma * w != 0.0) ge += gamma * w * e;
            if (store) aw[(int64_t)(n + 1) * K + j] = gamma;
            if (a.gamma && store) a.gamma[(cc * (int64_t)T + n + 1) * K + j] = gamma;
            // lb_n[i] on lane i: the row of <log A> is a column of its transpose
            double mr, sr;
            vmp_hmmf_column(myu, ATcol, KP, K, &mr, &sr);
            const double lbn = act ? mr + log(sr) : -INFINITY;
            lb = lbn - hmmv_grp_max<KP>(lbn);
            la_next = lan;
            lan = lan_prev;
            wd = wd_prev;
            wd_prev = wd_pp;
            e = e_prev;
            lds_fence();
        }
        {
            const double gl = act ? la_next + lb : -INFINITY;
            const double Mx = hmmv_grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, Mx);
            const double gamma = ex / hmmv_grp_sum<KP>(ex);
            z0acc += gamma * w;
            if (wd >= 0 && gamma * w != 0.0) ge += gamma * w * e;
            if (store) aw[j] = gamma;
            if (a.gamma && store) a.gamma[cc * (int64_t)T * K + j] = gamma;
            if (a.z0 && store) a.z0[cc * K + j] = gamma;
        }
    }

    // ---- the partial of this workgroup: groups in group order -----------------------------------
    const int64_t per = vmp_hmmv_partial_doubles(K);
    double *part = a.part + (int64_t)blockIdx.x * per;
    const double z0s = hmmv_across_groups<KP>(z0acc, lane);
    if (lane < K) part[lane] = z0s;
    lds_fence();
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        const double own = i < XR ? xi[i < XR ? i : 0] : xil[(i < XR ? 0 : i - XR) * 64 + lane];
        const double v = hmmv_across_groups<KP>(own, lane);
        if (i < K && lane < K) part[K + i * K + lane] = v;
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

constexpr int HMMV_NT = 256;

// one lane group per chunk; lanes j >= K have no column and leave (no shuffle in the walk)
template <int KP>
__global__ void __launch_bounds__(HMMV_NT)
hmmv_count_kernel(int64_t nchunks, int CH, int64_t n_obs, int M, int K,
                  const int32_t *__restrict__ order, const int32_t *__restrict__ off,
                  const double *__restrict__ gam, double *__restrict__ S,
                  double *__restrict__ head, double *__restrict__ tail)
{
    const int64_t c = ((int64_t)blockIdx.x * HMMV_NT + threadIdx.x) / KP;
    const int j = threadIdx.x & (KP - 1);
    if (c >= nchunks || j >= K) return;
    vmp_hmmv_walk_chunk(c, CH, n_obs, M, K, j, order, off, gam, S, head, tail);
}

// thread e < per: element e of the chain partials, the workgroups in order; thread per + m K + k:
// element (m, k) of S
__global__ void __launch_bounds__(HMMV_NT)
hmmv_combine_kernel(int64_t nw, int M, int K, int CH, int64_t n_obs,
                    const double *__restrict__ part, const int32_t *__restrict__ off,
                    const double *__restrict__ head, const double *__restrict__ tail,
                    double *__restrict__ z0sum, double *__restrict__ xisum, double *S,
                    double *__restrict__ scal)
{
    const int64_t per = vmp_hmmv_partial_doubles(K);
    const int64_t e = (int64_t)blockIdx.x * HMMV_NT + threadIdx.x;
    if (e >= per + (int64_t)M * K) return;
    if (e >= per) {
        const int64_t idx = e - per;
        vmp_hmmv_combine_word((int)(idx / K), (int)(idx % K), CH, K, n_obs, off, head, tail, S);
        return;
    }
    double v = 0.0;
    for (int64_t w = 0; w < nw; ++w) v += part[w * per + e];
    if (e < K) z0sum[e] = v;
    else if (e < per - 2) xisum[e - K] = v;
    else scal[e - (per - 2)] = v;
}

template <int KP>
int32_t launch_vocab(vmp_ctx *ctx, int64_t nw, const HmmvArgs &a, int64_t nchunks, int CH,
                     int64_t n_obs, const int32_t *order, const int32_t *off, double *S,
                     double *head, double *tail)
{
    const size_t lds = hmmv_lds_doubles(KP) * sizeof(double);
    static std::once_flag raised[64];           // per instance and device; host threads may race
    if (lds > 48 * 1024) {
        hipError_t err = hipSuccess;
        std::call_once(raised[ctx->device & 63], [&] {
            err = hipFuncSetAttribute((const void *)hmmv_chain_kernel<KP>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        });
        VMP_HIP_CHECK(ctx, err);
    }
    hipLaunchKernelGGL((hmmv_chain_kernel<KP>), dim3((unsigned)nw), dim3(64), lds, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    if (nchunks > 0) {
        const int64_t blocks = (nchunks * KP + HMMV_NT - 1) / HMMV_NT;
        hipLaunchKernelGGL((hmmv_count_kernel<KP>), dim3((unsigned)blocks), dim3(HMMV_NT), 0,
                           ctx->stream, nchunks, CH, n_obs, a.M, a.K, order, off, a.aw, S, head,
                           tail);
        VMP_HIP_CHECK(ctx, hipGetLastError());
    }
    return VMP_OK;
}

}  // namespace

extern "C" {

int32_t vmp_hmm_vocab_limits(int32_t *max_K, int32_t *max_M)
{
    if (!max_K || !max_M) return VMP_ERR_INVALID;
    *max_K = VMP_HMMF_MAX_K;
    *max_M = VMP_HMMV_MAX_M;
    return VMP_OK;
}

int32_t vmp_hmm_vocab_plan(int64_t B, int32_t T, int32_t M, int32_t K, int64_t n_obs,
                           int64_t *chains_per_wg, int32_t *chunk_entries,
                           int64_t *workspace_doubles)
{
    if (B < 0 || T < 2 || M < 1 || K < 1 || B * (int64_t)T >= ((int64_t)1 << 31) || n_obs < 0
        || n_obs > B * (int64_t)T || !chains_per_wg || !chunk_entries || !workspace_doubles)
        return VMP_ERR_INVALID;
    if (K > VMP_HMMF_MAX_K || M > VMP_HMMV_MAX_M) return VMP_ERR_UNSUPPORTED;
    *chains_per_wg = vmp_hmmv_chains_per_wg(B, K);
    *chunk_entries = vmp_hmmv_chunk_entries(n_obs, K);
    *workspace_doubles = vmp_hmmv_workspace_doubles(B, T, K, n_obs);
    return VMP_OK;
}

int32_t vmp_hmm_vocab_pass(vmp_ctx *ctx, int64_t B, int32_t T, int32_t M, int32_t K,
                           const int32_t *y, const double *elogPt, const double *elog_a0,
                           const double *elog_A, const int32_t *labels, const uint8_t *mask,
                           int64_t n_obs, const int32_t *order, const int32_t *word_offsets,
                           double *ws, double *z0sum, double *xisum, double *S, double *scal,
                           double *gamma, double *z0, double *zz)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, B >= 0 && T >= 2 && M >= 1 && K >= 1 && B * (int64_t)T < ((int64_t)1 << 31)
                     && n_obs >= 0 && n_obs <= B * (int64_t)T, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_HMMF_MAX_K && M <= VMP_HMMV_MAX_M, VMP_ERR_UNSUPPORTED,
                "M = %d, K = %d exceed the limits (%d, %d)", M, K, VMP_HMMV_MAX_M, VMP_HMMF_MAX_K);
    VMP_REQUIRE(ctx, ctx && elog_a0 && elog_A && ws && z0sum && xisum && S && scal
                     && (B == 0 || y) && (n_obs == 0 || (order && word_offsets)),
                VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int64_t nw = vmp_hmmv_wgs(B, K);
    const int64_t per = vmp_hmmv_partial_doubles(K);
    const int CH = vmp_hmmv_chunk_entries(n_obs, K);
    const int64_t nchunks = vmp_hmmv_chunks(n_obs, K);
    double *part = ws + B * (int64_t)T * K;
    double *head = part + nw * per, *tail = head + nchunks * K;
    double *dot_ws = head + 2 * vmp_hmmv_max_chunks(n_obs, K) * K;
    if (nw > 0) {
        HmmvArgs a = {B, vmp_hmmv_chains_per_wg(B, K), T, M, K, y, elogPt, elog_a0, elog_A,
                      labels, mask, ws, part, gamma, z0, zz};
        int32_t rc;
        switch (vmp_hmmf_kpad(K)) {
        case 2: rc = launch_vocab<2>(ctx, nw, a, nchunks, CH, n_obs, order, word_offsets, S, head, tail); break;
        case 4: rc = launch_vocab<4>(ctx, nw, a, nchunks, CH, n_obs, order, word_offsets, S, head, tail); break;
        case 8: rc = launch_vocab<8>(ctx, nw, a, nchunks, CH, n_obs, order, word_offsets, S, head, tail); break;
        case 16: rc = launch_vocab<16>(ctx, nw, a, nchunks, CH, n_obs, order, word_offsets, S, head, tail); break;
        case 32: rc = launch_vocab<32>(ctx, nw, a, nchunks, CH, n_obs, order, word_offsets, S, head, tail); break;
        default: rc = launch_vocab<64>(ctx, nw, a, nchunks, CH, n_obs, order, word_offsets, S, head, tail); break;
        }
        if (rc != VMP_OK) return rc;
    }
    const int64_t elems = per + (int64_t)M * K;
    hipLaunchKernelGGL(hmmv_combine_kernel, dim3((unsigned)((elems + HMMV_NT - 1) / HMMV_NT)),
                       dim3(HMMV_NT), 0, ctx->stream, nw, M, K, CH, n_obs, part, word_offsets, head,
                       tail, z0sum, xisum, S, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    int32_t rc = vmp_lda_dot(ctx, K, z0sum, elog_a0, dot_ws, scal + 2);
    if (rc != VMP_OK) return rc;
    return vmp_lda_dot(ctx, (int64_t)K * K, xisum, elog_A, dot_ws, scal + 3);
}

}  // extern "C"
