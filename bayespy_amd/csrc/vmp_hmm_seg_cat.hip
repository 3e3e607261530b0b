// vmp_hmm_seg_cat.hip -- the segmented (time-parallel) chain pass of the fused hidden-Markov-model
// block with categorical emissions: vmp_hmm_fused_pass_categorical (vmp_hmm_cat.hip) for few long
// chains.
//
// The sequential pass walks a chain with 2 (T - 1) dependent steps on one lane group.  Here the
// chain is cut into segments of L transitions as in vmp_hmm_seg.hip (vmp_hmm_seg_dev.h: the
// formulas, who owns what, the order of the additions; vmp_hmm_seg_cat_dev.h: the count).  By the
// rule recorded at the top of vmp_hmm_cat.hip the Gaussian kernels keep their text, so these are
// kernels of their own, and the discrete emission lets them differ where it pays:
//
//   hmmsc_transfer_kernel  log W_s[i, :] for every (chain, segment, start state i), the lane mapping
//                          of hmms_transfer_kernel.  No B T KP emission table exists: the word-major
//                          <log P> (M x KP, padded columns -inf) sits in LDS once per workgroup
//                          beside <log A>, a step costs one int32 word per lane group and one LDS
//                          read per lane.  b_t = max_j e_t[j] depends on the word alone: bmax[m]
//                          is formed once per workgroup and the butterfly maximum leaves the
//                          dependent chain of every step.  The word of step n + 1 is requested
//                          before the arithmetic of step n.
//   hmmsc_scan_kernel      la at the segment starts, lb at the segment ends, log Z and the weight of
//                          the chain; step 0 has la0[j] + <log P>[y_0][j], or la0[j] where masked
//   hmmsc_sweep_kernel     forward and backward inside every segment from the stored la and lb;
//                          four wavefronts share <log A>, its transpose and the table in LDS
//   hmmsc_count_kernel     S[m][k] from the in-place gamma and the words, each read once: private
//                          histograms per lane in LDS, sacc[m * 64 + lane] (the bank depends on the
//                          lane alone, two lane groups never share an address), one wavefront per
//                          workgroup, a fixed contiguous range of rows, no atomics
//   hmmsc_combine_kernel   one thread per output element, the partials in workgroup order
//
// A masked step has e = 0 and reads neither its word nor the table; so does a step whose word is
// outside [0, M) (vmp_hmmf_cat_observed): such a word never becomes an address.  With fixed labels
// the pass IS vmp_hmm_fused_pass_categorical.
#include <mutex>

#include "vmp_common.h"
#include "vmp_hmm_seg_cat_dev.h"

namespace {

struct HmmscArgs {
    int64_t B, S, ipw, rpw;   // chains, segments of a chain, items of a sweep workgroup, rows of a count one
    int T, M, K, L;
    const int32_t *y;         // B x T words
    const double *P;          // M x K <log P>, word-major, or null (no emission term)
    const double *la0, *lA;
    const uint8_t *mask;
    double *W;                // B S K x KP: log W less the segment's sum b
    double *laB, *lbB;        // B S x KP: la at the segment start, lb at the segment end
    double *seg;              // B S x 2: any step observed, sum b
    double *chain;            // B x 2: weight, weighted log Z
    double *aw;               // B x T x K: la on the way forward, gamma on the way back
    double *part;             // sweep workgroups x vmp_hmmw_chain_partial_doubles
    double *spart;            // count workgroups x M K
    double *gamma, *z0, *zz;
};

template <int KP>
__device__ __forceinline__ double hmmsc_grp_max(double v)
{
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

template <int KP>
__device__ __forceinline__ double hmmsc_grp_sum(double v)
{
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the value of lane (j, group g) added over the groups in group order; valid in lanes < KP
template <int KP>
__device__ __forceinline__ double hmmsc_across_groups(double v, int lane)
{
    double t = v;
#pragma unroll
    for (int g = 1; g < 64 / KP; ++g) t += __shfl(v, (lane & (KP - 1)) + g * KP, 64);
    return t;
}

// the word of step t of a chain, or -1 where the step is masked (the word is not read) or the
// word is out of range
__device__ __forceinline__ int hmmsc_word(const int32_t *yrow, const uint8_t *mrow, int64_t t, int M)
{
    if (mrow && mrow[t] == 0) return -1;
    const int32_t v = yrow[t];
    return vmp_hmmf_cat_observed(true, v, M) ? v : -1;
}

// the table in LDS: Ps[m * KP + c] = <log P>[m][c] (0 without an emission term), -inf at c >= K
template <int KP>
__device__ __forceinline__ void hmmsc_load_table(double *Ps, const double *P, int M, int K, int tid,
                                                 int nthreads)
{
    for (int e = tid; e < M * KP; e += nthreads) {
        const int m = e / KP, c = e % KP;
        Ps[e] = c < K ? (P ? P[m * K + c] : 0.0) : -INFINITY;
    }
}

// ---- stage 1: the transfer of every (chain, segment, start state) ---------------------------------
// LDS: <log A>, one vector per lane group, the table and its row maxima.  Item =
// (chain S + segment) K + i, 256 / KP consecutive items per round: the groups of a round sit in at
// most two segments next to each other and ask for the same words.  A group runs its own number
// of steps; nothing is exchanged between groups.
template <int KP>
__global__ __launch_bounds__(256) void hmmsc_transfer_kernel(HmmscArgs a)
{
    extern __shared__ double hmmsc_lds[];
    constexpr int GW = 256 / KP;
    const int T = a.T, M = a.M, K = a.K, L = a.L;
    double *As = hmmsc_lds;                // [i * KP + j]
    double *vec = As + KP * KP;            // [thread] = v of (group, i)
    double *Ps = vec + 256;                // [m * KP + j]
    double *bmax = Ps + M * KP;            // [m] = max_j <log P>[m][j], 0 where that is -inf
    const int tid = threadIdx.x, grp = tid / KP, j = tid % KP;
    const bool act = j < K;
    for (int e = tid; e < KP * KP; e += 256) {
        const int i = e / KP, c = e % KP;
        As[e] = (i < K && c < K) ? a.lA[i * K + c] : -INFINITY;
    }
    hmmsc_load_table<KP>(Ps, a.P, M, K, tid, 256);
    __syncthreads();
    for (int m = tid; m < M; m += 256) {
        double b = -INFINITY;
        for (int c = 0; c < K; ++c) b = fmax(b, Ps[m * KP + c]);
        bmax[m] = (b == -INFINITY) ? 0.0 : b;
    }
    __syncthreads();
    double *myv = vec + grp * KP;
    const double *Acol = As + j, *Pcol = Ps + j;
    const int64_t nitem = a.B * a.S * K;
    for (int64_t it0 = (int64_t)blockIdx.x * GW; it0 < nitem; it0 += (int64_t)gridDim.x * GW) {
        const int64_t it = it0 + grp;
        if (it >= nitem) continue;                     // the whole group leaves
        const int i = (int)(it % K);
        const int64_t bs = it / K, cc = bs / a.S;
        const int s = (int)(bs % a.S);
        const int n0 = s * L, n1 = (n0 + L < T - 1) ? n0 + L : T - 1;
        const int32_t *yrow = a.y + cc * (int64_t)T;
        const uint8_t *mrow = a.mask ? a.mask + cc * (int64_t)T : nullptr;
        int any = (mrow && s == 0) ? mrow[0] : 0;
        double v = (j == i) ? 0.0 : -INFINITY;
        double scale = 0.0, bsum = 0.0;
        int wd_next = hmmsc_word(yrow, mrow, n0 + 1, M);
        for (int n = n0 + 1; n <= n1; ++n) {
            const int wd = wd_next;
            if (n < n1) wd_next = hmmsc_word(yrow, mrow, n + 1, M);
            if (mrow) any |= mrow[n];
            myv[j] = v;
            lds_fence();
            // e - b of this lane and b of the step: two LDS reads off the dependent chain
            const double e = wd >= 0 ? Pcol[wd * KP] : 0.0;
            const double b = wd >= 0 ? bmax[wd] : 0.0;
            double m, sm;
            vmp_hmmf_column(myv, Acol, KP, K, &m, &sm);
            const double q = act ? m + log(sm) + (e - b) : -INFINITY;
            const double Mx = hmmsc_grp_max<KP>(q);
            const double Sm = hmmsc_grp_sum<KP>(vmp_hmmf_exp_shift(q, Mx));
            const double cn = Mx + log(Sm);
            // nothing reachable from i: the row of W stays -inf, no NaN from -inf - -inf
            if (Mx != -INFINITY) scale += cn;
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
__global__ __launch_bounds__(64) void hmmsc_scan_kernel(HmmscArgs a)
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
    const int wd0 = hmmsc_word(a.y + cc * (int64_t)T, a.mask ? a.mask + cc * (int64_t)T : nullptr,
                               0, a.M);
    double la = act ? a.la0[j] + ((wd0 >= 0 && a.P) ? a.P[(int64_t)wd0 * K + j] : 0.0) : -INFINITY;
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
        const double Mx = hmmsc_grp_max<KP>(q);
        const double Sm = hmmsc_grp_sum<KP>(vmp_hmmf_exp_shift(q, Mx));
        const double cn = Mx + log(Sm);
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
        lb = lbn - hmmsc_grp_max<KP>(lbn);
        lds_fence();
    }
    if (j == 0) {
        a.chain[cc * 2] = w;
        a.chain[cc * 2 + 1] = logZ;
    }
}

// ---- stage 3: the sweep inside every segment --------------------------------------------------------
// The recursion, the lane mapping and the order inside a step of hmmc_pass_kernel.  Registers: the
// column of sum xi and the exponentials of the step (KP doubles each); LDS: <log A>, its
// transpose, the la / u vectors of the four wavefronts and the table; the partial of the
// workgroup is added up in the place of <log A> once every wavefront is done with it.
template <int KP>
__global__ __launch_bounds__(64 * VMP_HMMS_WAVES) void hmmsc_sweep_kernel(HmmscArgs a)
{
    extern __shared__ double hmmsc_lds[];
    constexpr int G = 64 / KP, WV = VMP_HMMS_WAVES;
    const int T = a.T, M = a.M, K = a.K, L = a.L;
    const int64_t S = a.S;
    double *As = hmmsc_lds;                // [i * KP + j]
    double *ATs = As + KP * KP;            // [j * KP + i]
    double *vec = ATs + KP * KP;           // [thread] = la of (wavefront, group, i)
    double *uvec = vec + 64 * WV;          // [thread] = u of (wavefront, group, j)
    double *Ps = uvec + 64 * WV;           // [m * KP + j]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane / KP, j = lane % KP;
    const bool act = j < K;
    for (int e = tid; e < KP * KP; e += 64 * WV) {
        const int i = e / KP, c = e % KP;
        const double v = (i < K && c < K) ? a.lA[i * K + c] : -INFINITY;
        As[e] = v;
        ATs[c * KP + i] = v;
    }
    hmmsc_load_table<KP>(Ps, a.P, M, K, tid, 64 * WV);
    __syncthreads();
    double *myv = vec + wave * 64 + grp * KP, *myu = uvec + wave * 64 + grp * KP;
    const double *Acol = As + j, *ATcol = ATs + j, *Pcol = Ps + j;

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
        const int32_t *yrow = a.y + cc * (int64_t)T;
        const uint8_t *mrow = a.mask ? a.mask + cc * (int64_t)T : nullptr;
        auto word = [&](int t) -> int { return hmmsc_word(yrow, mrow, t, M); };
        // this lane's e_t[j]: 0 at a masked step, which counts for nothing in sum gamma . e
        auto emit = [&](int wd) -> double { return wd >= 0 ? Pcol[wd * KP] : 0.0; };
        // ---- forward from la at n0: the word of step n + 1 is requested before the arithmetic of
        // step n ---------------------------------------------------------------------------------
        const double la_start = a.laB[it * KP + j];
        double la = la_start;
        int wd_next = word(n0 + 1);
        for (int n = n0 + 1; n <= n1; ++n) {
            const int wd = wd_next;
            if (n < n1) wd_next = word(n + 1);
            myv[j] = la;
            lds_fence();
            const double e = emit(wd);
            double m, sm;
            vmp_hmmf_column(myv, Acol, KP, K, &m, &sm);
            const double q = act ? m + log(sm) + e : -INFINITY;
            const double Mx = hmmsc_grp_max<KP>(q);
            const double Sm = hmmsc_grp_sum<KP>(vmp_hmmf_exp_shift(q, Mx));
            la = q - (Mx + log(Sm));
            if (act) aw[(int64_t)n * K + j] = la;
            lds_fence();
        }
        // ---- backward from lb at n1: gamma_{n+1} goes where la_{n+1} stood; la_n and the word of
        // the step to come are requested first.  aw[n K + j], n0 < n <= n1, was written by this
        // lane; la at n0 is the stored boundary value. -------------------------------------------
        double lb = a.lbB[it * KP + j];
        double la_next = la;
        int wd = word(n1);
        double lan = (n1 - 1 > n0) ? (act ? aw[(int64_t)(n1 - 1) * K + j] : -INFINITY) : la_start;
        for (int n = n1 - 1; n >= n0; --n) {
            int wd_prev = -1;
            double lan_prev = -INFINITY;
            if (n > n0) {
                wd_prev = word(n);
                lan_prev = (n - 1 > n0) ? (act ? aw[(int64_t)(n - 1) * K + j] : -INFINITY) : la_start;
            }
            const double e = emit(wd);
            const double gl = act ? la_next + lb : -INFINITY;
            const double Mx = hmmsc_grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, Mx);
            const double gamma = ex / hmmsc_grp_sum<KP>(ex);
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
            lb = lbn - hmmsc_grp_max<KP>(lbn);
            la_next = lan;
            lan = lan_prev;
            wd = wd_prev;
            lds_fence();
        }
        if (s == 0) {
            // step 0 and log Z of the chain belong to its first segment
            const double e = emit(word(0));
            const double gl = act ? la_next + lb : -INFINITY;
            const double Mx = hmmsc_grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, Mx);
            const double gamma = ex / hmmsc_grp_sum<KP>(ex);
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
    double *red = hmmsc_lds;                // per <= 2 KP KP + 2: inside <log A> and the vectors
    __syncthreads();                        // every wavefront is done with <log A>
    for (int wv = 0; wv < WV; ++wv) {
        if (wave == wv) {
            const double z0s = hmmsc_across_groups<KP>(z0acc, lane);
            if (lane < K) red[lane] = wv ? red[lane] + z0s : z0s;
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                const double v = hmmsc_across_groups<KP>(xi[i], lane);
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

// ---- stage 4: the counts ------------------------------------------------------------------------------
// One wavefront owns rows [blockIdx rpw, + rpw) of the flattened (b, t) plate; lane group g takes
// the rows g, g + G, ... of the range, lane (g, k) reads gamma[row][k] (the K lanes of a group one
// contiguous row) and the group one word.  The row of the round to come is requested before the
// LDS update of the present one.  The kernel is bound by reading gamma: a one-hot product on the
// matrix cores would spend M multiply-adds per entry to save this one add.
template <int KP>
__global__ __launch_bounds__(64) void hmmsc_count_kernel(HmmscArgs a)
{
    extern __shared__ double hmmsc_lds[];
    constexpr int G = 64 / KP;
    const int M = a.M, K = a.K;
    double *sacc = hmmsc_lds;              // [m * 64 + lane]
    const int lane = threadIdx.x, grp = lane / KP, j = lane % KP;
    const bool act = j < K;
    for (int e = lane; e < M * 64; e += 64) sacc[e] = 0.0;     // the lane's own column
    const int64_t R = a.B * (int64_t)a.T;
    const int64_t r_begin = (int64_t)blockIdx.x * a.rpw;
    const int64_t r_end = (r_begin + a.rpw < R) ? r_begin + a.rpw : R;
    // a lane's own loads and its own histogram: no fence and no shuffle in the loop
    auto fetch = [&](int64_t r, int *wd, double *g) {
        *wd = -1;
        *g = 0.0;
        if (r < r_end) {
            *wd = hmmsc_word(a.y, a.mask, r, M);
            if (*wd >= 0 && act) *g = a.aw[r * K + j];
        }
    };
    int wd_next;
    double g_next;
    fetch(r_begin + grp, &wd_next, &g_next);
    for (int64_t r0 = r_begin; r0 < r_end; r0 += G) {
        const int wd = wd_next;
        const double g = g_next;
        fetch(r0 + G + grp, &wd_next, &g_next);
        if (wd >= 0 && act) sacc[wd * 64 + lane] += g;
    }
    lds_fence();
    if (lane < K) {
        double *ps = a.spart + (int64_t)blockIdx.x * M * K + lane;
        for (int m = 0; m < M; ++m) {
            double t = 0.0;
            for (int g = 0; g < G; ++g) t += sacc[m * 64 + g * KP + lane];
            ps[(int64_t)m * K] = t;
        }
    }
}

// one thread per output element: the partials of the sweep and of the count kernel, each in
// workgroup order; the counts stay word-major
__global__ void __launch_bounds__(256)
hmmsc_combine_kernel(int64_t nws, int64_t nwc, int M, int K, const double *__restrict__ cpart,
                     const double *__restrict__ spart, double *__restrict__ z0sum,
                     double *__restrict__ xisum, double *__restrict__ S, double *__restrict__ scal)
{
    const int64_t perc = vmp_hmmw_chain_partial_doubles(K), MK = (int64_t)M * K;
    const int64_t oS = perc - 2, nout = perc + MK;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= nout) return;
    double v = 0.0;
    if (e >= oS && e < oS + MK) {
        for (int64_t w = 0; w < nwc; ++w) v += spart[w * MK + (e - oS)];
        S[e - oS] = v;
        return;
    }
    const int64_t ec = e < oS ? e : e - MK;
    for (int64_t w = 0; w < nws; ++w) v += cpart[w * perc + ec];
    if (ec < K) {
        z0sum[ec] = v;
    } else if (ec < oS) {
        xisum[ec - K] = v;
    } else {
        scal[ec - oS] = v;
    }
}

template <int KP>
int32_t launch_seg_cat(vmp_ctx *ctx, int64_t nws, int64_t nwc, const HmmscArgs &a)
{
    const size_t lds1 = (size_t)vmp_hmmsc_transfer_lds_doubles(KP, a.M) * sizeof(double);
    const size_t lds3 = (size_t)vmp_hmmsc_sweep_lds_doubles(KP, a.M) * sizeof(double);
    const size_t lds4 = (size_t)a.M * 64 * sizeof(double);
    static std::once_flag raised[64];           // per instance and device; host threads may race
    if (lds1 > 48 * 1024 || lds3 > 48 * 1024 || lds4 > 48 * 1024) {
        hipError_t err = hipSuccess;
        std::call_once(raised[ctx->device & 63], [&] {
            const void *kernels[3] = {(const void *)hmmsc_transfer_kernel<KP>,
                                      (const void *)hmmsc_sweep_kernel<KP>,
                                      (const void *)hmmsc_count_kernel<KP>};
            for (int k = 0; k < 3 && err == hipSuccess; ++k)
                err = hipFuncSetAttribute(kernels[k], hipFuncAttributeMaxDynamicSharedMemorySize,
                                          160 * 1024);
        });
        VMP_HIP_CHECK(ctx, err);
    }
    const int64_t rounds = (a.B * a.S * a.K + 256 / KP - 1) / (256 / KP);
    const int64_t g1 = rounds < VMP_HMMS_MAX_TRANSFER_WGS ? rounds : VMP_HMMS_MAX_TRANSFER_WGS;
    hipLaunchKernelGGL((hmmsc_transfer_kernel<KP>), dim3((unsigned)g1), dim3(256), lds1, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    const int64_t g2 = (a.B + 64 / KP - 1) / (64 / KP);
    hipLaunchKernelGGL((hmmsc_scan_kernel<KP>), dim3((unsigned)g2), dim3(64), 0, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL((hmmsc_sweep_kernel<KP>), dim3((unsigned)nws), dim3(64 * VMP_HMMS_WAVES), lds3,
                       ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    hipLaunchKernelGGL((hmmsc_count_kernel<KP>), dim3((unsigned)nwc), dim3(64), lds4, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // namespace

extern "C" {

int32_t vmp_hmm_seg_cat_limits(int32_t *max_K, int32_t *max_M)
{
    if (!max_K || !max_M) return VMP_ERR_INVALID;
    *max_K = VMP_HMMSC_MAX_K;
    *max_M = VMP_HMMSC_MAX_M;
    return VMP_OK;
}

int32_t vmp_hmm_seg_cat_plan(int64_t B, int32_t T, int32_t M, int32_t K, int32_t seg_len,
                             int32_t *seg_len_used, int64_t *workspace_doubles)
{
    if (B < 0 || T < 2 || M < 1 || K < 1 || seg_len < 0 || !seg_len_used || !workspace_doubles)
        return VMP_ERR_INVALID;
    if (K > VMP_HMMSC_MAX_K || M > VMP_HMMSC_MAX_M) return VMP_ERR_UNSUPPORTED;
    if (seg_len == 0) {
        const int tuned = vmp_tune_get("hmm_seg_len", 0);
        if (tuned > 0) seg_len = tuned;
    }
    *seg_len_used = vmp_hmms_clamp_len(B, T, K, seg_len);
    *workspace_doubles = vmp_hmmsc_workspace_doubles(B, T, M, K, *seg_len_used);
    return VMP_OK;
}

int32_t vmp_hmm_seg_pass_categorical(vmp_ctx *ctx, int64_t B, int32_t T, int32_t M, int32_t K,
                                     const int32_t *y, const double *elogPt, const double *elog_a0,
                                     const double *elog_A, const int32_t *labels,
                                     const uint8_t *mask, double *ws, double *z0sum, double *xisum,
                                     double *S, double *scal, double *gamma, double *z0, double *zz,
                                     int32_t seg_len)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, B >= 0 && T >= 2 && M >= 1 && K >= 1 && seg_len >= 0, VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_HMMSC_MAX_K && M <= VMP_HMMSC_MAX_M, VMP_ERR_UNSUPPORTED,
                "M = %d, K = %d exceed the limits (%d, %d)", M, K, VMP_HMMSC_MAX_M, VMP_HMMSC_MAX_K);
    VMP_REQUIRE(ctx, ctx && elog_a0 && elog_A && ws && z0sum && xisum && S && scal
                     && (B == 0 || y), VMP_ERR_INVALID, "null argument");
    // fixed states: the one-hot path of the sequential pass, and its bits (the workspace covers it)
    if (labels)
        return vmp_hmm_fused_pass_categorical(ctx, B, T, M, K, y, elogPt, elog_a0, elog_A, labels,
                                              mask, ws, z0sum, xisum, S, scal, gamma, z0, zz);
    VMP_FLUSH_SMALL(ctx);
    int32_t L = 0;
    int64_t wsd = 0;
    int32_t rc = vmp_hmm_seg_cat_plan(B, T, M, K, seg_len, &L, &wsd);
    if (rc != VMP_OK) return rc;
    const int KP = vmp_hmmf_kpad(K);
    const int64_t R = B * (int64_t)T, Sg = vmp_hmms_segments(T, L), BS = B * Sg;
    const int64_t nws = vmp_hmms_sweep_wgs(B, T, K, L), nwc = vmp_hmmsc_count_wgs(B, T, M, K);
    const int64_t perc = vmp_hmmw_chain_partial_doubles(K);
    double *aw = ws, *cpart = aw + R * K, *spart = cpart + nws * perc;
    double *dot_ws = spart + nwc * (int64_t)M * K;
    double *W = dot_ws + 1024, *laB = W + BS * K * KP, *lbB = laB + BS * KP, *seg = lbB + BS * KP;
    double *chain = seg + 2 * BS;
    if (R > 0) {
        HmmscArgs sa = {B, Sg, vmp_hmms_items_per_wg(B, T, K, L), vmp_hmmsc_rows_per_wg(B, T, M, K),
                        T, M, K, L, y, elogPt, elog_a0, elog_A, mask, W, laB, lbB, seg, chain, aw,
                        cpart, spart, gamma, z0, zz};
        switch (KP) {
        case 2: rc = launch_seg_cat<2>(ctx, nws, nwc, sa); break;
        case 4: rc = launch_seg_cat<4>(ctx, nws, nwc, sa); break;
        case 8: rc = launch_seg_cat<8>(ctx, nws, nwc, sa); break;
        case 16: rc = launch_seg_cat<16>(ctx, nws, nwc, sa); break;
        case 32: rc = launch_seg_cat<32>(ctx, nws, nwc, sa); break;
        default: rc = launch_seg_cat<64>(ctx, nws, nwc, sa); break;
        }
        if (rc != VMP_OK) return rc;
    }
    const int64_t nout = perc + (int64_t)M * K;
    hipLaunchKernelGGL(hmmsc_combine_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0,
                       ctx->stream, nws, nwc, M, K, cpart, spart, z0sum, xisum, S, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    rc = vmp_lda_dot(ctx, K, z0sum, elog_a0, dot_ws, scal + 2);
    if (rc != VMP_OK) return rc;
    return vmp_lda_dot(ctx, (int64_t)K * K, xisum, elog_A, dot_ws, scal + 3);
}

}  // extern "C"
