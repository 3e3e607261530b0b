// vmp_hmm_states.hip -- the wide-state pass of the fused hidden-Markov-model block: multinomial
// emissions with 65 to 128 states
//
//     Z = CategoricalMarkovChain(a0, A, states=T);  Y = Mixture(Z, Multinomial, n, P);  Y.observe(x)
//
// The emission, statistics, combine and shift kernels are those of vmp_hmm_mult.hip with eight
// state tiles (vmp_hmmm_stages).  The chain stage is the kernel of this file: the recursion in the
// domain of scaled probabilities, its K x K products on the fp64 matrix cores.  The recursion, the
// split and the order of the additions: vmp_hmm_states_dev.h.
//
// RANGE (vmp_hmm_states_dev.h): an entry of <log A> below about -745 acts as -inf, and a step whose
// predicted mass underflows entirely cannot be told from an impossible observation (NaN from there
// on, as for one).  There is no log-domain fallback.
//
// hmms_chain_kernel, 256 lanes = four wavefronts, one workgroup per compute unit (149 KB of LDS):
//   * P = exp(<log A>) is resident in LDS, 128 rows of 130 doubles.  Forward it is the B operand
//     B[k = i][col = j]; the contraction index of instruction q and lane group l4 is the state
//     i = (q & 7) + 8 l4 + 32 (q >> 3), so that the four rows of one instruction lie 8 rows =
//     1040 doubles = 16 (mod 32) apart: the two rows of a half-wavefront cover all 64 banks once.
//     Backward the same array is read transposed, B[k = j][col = i] = P[i][j] with j = 4 q + l4:
//     lanes l15 are 130 doubles = 2 (mod 32) apart, l4 fills the odd double.  Both are free of bank
//     conflicts under the half-wavefront model of an 8-byte LDS read.
//   * the tile of the step goes through one 18 KB buffer: forward ah_{t-1} state-major with stride
//     18 (A operand X[i][chain], conflict-free with the i of above), backward v_{t+1} chain-major
//     with stride 130 (A operand X[chain][j], conflict-free).  The same v tile is the B operand of
//     the sum-xi product, read X[chain = 4 q + l4][j]: there 14 of the 16 doubles of the two rows
//     of a half-wavefront share banks -- the one read of the kernel that is not conflict-free (32
//     reads per step and wavefront against 96 + 96 of the other two products).
//   * the accumulator layout D[row l4 + 4 r][col l15] is the operand layout of a product
//     contracted over the rows with k = l4 + 4 q: the A operand of the sum-xi product,
//     o_b ah_t / s_t for the wavefront's own 32 states, comes straight from registers.  Its 16
//     accumulator tiles (rows: the own states, columns: all 128) live in 128 registers over all
//     steps and tiles of the workgroup.
//   * sums over the states: in the lane over its two tiles, a butterfly over l15, the four
//     wavefronts through LDS in wavefront order.
//   * e of the step to come (and ah of the step to come, backward) are requested before the matrix
//     work of the step.  Every (chain, state) of the workspace is written and read back by the
//     same lane.
#include <mutex>

#include "vmp_common.h"
#include "vmp_hmm_states_dev.h"

namespace {

constexpr int KP = VMP_HMMS_KP, PS = VMP_HMMS_P_STRIDE, XF = VMP_HMMS_XF_STRIDE;
constexpr int XB = VMP_HMMS_XB_STRIDE, TILE = VMP_HMMS_TILE;

struct HmmsChainArgs {
    int64_t B, cpw;
    int T, K;
    const double *E;          // B T x 128, or null (no emission term)
    const double *la0, *lA;
    const int32_t *labels;
    const uint8_t *mask;
    double *aw;               // B x T x K: ah on the way forward, gamma on the way back
    double *part;
    double *gamma, *z0, *zz;
};

__device__ __forceinline__ double hmms_exp(double e) { return e == -INFINITY ? 0.0 : exp(e); }

// v[r] (NV values per chain l4 + 4 r, this lane's share of the states) added over the 128 states;
// every lane ends with the sums of its four chains.  One barrier; the caller has another between
// this call's reads of red and the next call's writes.
template <int NV>
__device__ __forceinline__ void hmms_state_sums(double (&v)[NV][4], double *red, int w, int l15, int l4)
{
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) v[s][r] += __shfl_xor(v[s][r], m, 64);
            if (l15 == 0) red[(w * TILE + l4 + 4 * r) * 2 + s] = v[s][r];
        }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NV; ++s)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double *p = red + (l4 + 4 * r) * 2 + s;
            v[s][r] = ((p[0] + p[TILE * 2]) + p[2 * TILE * 2]) + p[3 * TILE * 2];
        }
}

// a chain's weight: 0 past the end of the range and without an observed step; 16 lanes per chain
__device__ __forceinline__ void hmms_weights(const HmmsChainArgs &a, int64_t c0, int64_t c_end, int tid,
                                             double *wts)
{
    const int ch = tid >> 4, sub = tid & 15;
    const bool lv = c0 + ch < c_end;
    int any = a.mask ? 0 : 1;
    if (a.mask && lv)
        for (int t = sub; t < a.T; t += 16) any |= a.mask[(c0 + ch) * (int64_t)a.T + t];
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) any |= __shfl_xor(any, m, 64);
    if (sub == 0) wts[ch] = (lv && any) ? 1.0 : 0.0;
}

template <bool ZZ>
__global__ __launch_bounds__(256) void hmms_chain_kernel(HmmsChainArgs a)
{
    extern __shared__ double hmms_lds[];
    double *Ps = hmms_lds;                       // [i * PS + j]
    double *X = Ps + KP * PS;                    // the tile of the step
    double *red = X + KP * XF;                   // [wavefront][chain][2]
    double *wts = red + 4 * TILE * 2;            // [chain]
    const int T = a.T, K = a.K;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int st[2] = {(2 * w) * 16 + l15, (2 * w + 1) * 16 + l15};     // this lane's states
    const bool act[2] = {st[0] < K, st[1] < K};

    for (int e = tid; e < KP * KP; e += 256) {
        const int i = e >> 7, j = e & (KP - 1);
        Ps[i * PS + j] = (i < K && j < K) ? hmms_exp(a.lA[i * K + j]) : 0.0;
    }
    double m0 = -INFINITY;
    for (int j = 0; j < K; ++j) m0 = fmax(m0, a.la0[j]);
    double pi[2];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) pi[t2] = act[t2] ? hmms_exp(a.la0[st[t2]] - m0) : 0.0;

    v4f64 xi[2][8];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int jt = 0; jt < 8; ++jt) xi[t2][jt] = v4f64{0.0, 0.0, 0.0, 0.0};
    double z0acc[2] = {0.0, 0.0}, logZ = 0.0, ge = 0.0;

    const int64_t c_begin = (int64_t)blockIdx.x * a.cpw;
    const int64_t c_end = (c_begin + a.cpw < a.B) ? c_begin + a.cpw : a.B;
    for (int64_t c0 = c_begin; c0 < c_end; c0 += TILE) {
        __syncthreads();            // P is written; the readers of the previous tile are done
        hmms_weights(a, c0, c_end, tid, wts);
        __syncthreads();
        bool live[4];
        int64_t cc[4];
        double wt[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t c = c0 + l4 + 4 * r;
            live[r] = c < c_end;
            cc[r] = live[r] ? c : c_begin;
            wt[r] = wts[l4 + 4 * r];
        }
        // the sum-xi product of a step: A from registers, B the chain-major tile in X
        auto add_xi = [&](const double (&as)[4][2]) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int jt = 0; jt < 8; ++jt) {
                    const double bv = X[(4 * q + l4) * XB + jt * 16 + l15];
#pragma unroll
                    for (int t2 = 0; t2 < 2; ++t2)
                        xi[t2][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[q][t2], bv, xi[t2][jt], 0, 0, 0);
                }
        };
        auto put = [&](int t, const double (&g)[4][2]) {    // gamma_t (or ah_t) of the own states
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
                    if (live[r] && act[t2]) a.aw[(cc[r] * T + t) * K + st[t2]] = g[r][t2];
        };
        auto put_out = [&](int t, const double (&g)[4][2]) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    if (!live[r] || !act[t2]) continue;
                    if (a.gamma) a.gamma[(cc[r] * T + t) * K + st[t2]] = g[r][t2];
                    if (a.z0 && t == 0) a.z0[cc[r] * K + st[t2]] = g[r][t2];
                }
        };

        auto load_e = [&](int t, double (&e)[4][2]) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
                    e[r][t2] = a.E ? a.E[(cc[r] * T + t) * KP + st[t2]] : (act[t2] ? 0.0 : -INFINITY);
        };
        // ---- forward ------------------------------------------------------------------------------
        double e[4][2], en[4][2], al[4][2];
        load_e(0, e);
        load_e(1, en);
        {
            double s[1][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) al[r][t2] = pi[t2] * hmms_exp(e[r][t2]);
                s[0][r] = al[r][0] + al[r][1];
            }
            hmms_state_sums<1>(s, red, w, l15, l4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) al[r][t2] /= s[0][r];
                logZ += (log(s[0][r]) + m0) * wt[r];
            }
            put(0, al);
        }
        for (int n = 1; n < T; ++n) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    e[r][t2] = en[r][t2];
                    X[st[t2] * XF + l4 + 4 * r] = al[r][t2];
                }
            __syncthreads();
            if (n + 1 < T) load_e(n + 1, en);
            v4f64 acc[2][2];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) acc[t2][0] = acc[t2][1] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
            for (int q = 0; q < KP / 4; q += 2)
#pragma unroll
                for (int h = 0; h < 2; ++h) {       // two accumulators per tile: even and odd q
                    const int i = ((q + h) & 7) + 8 * l4 + 32 * ((q + h) >> 3);
                    const double av = X[i * XF + l15];
#pragma unroll
                    for (int t2 = 0; t2 < 2; ++t2)
                        acc[t2][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Ps[i * PS + st[t2]],
                                                                          acc[t2][h], 0, 0, 0);
                }
            double s[1][4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
                    al[r][t2] = (acc[t2][0][r] + acc[t2][1][r]) * hmms_exp(e[r][t2]);
                s[0][r] = al[r][0] + al[r][1];
            }
            hmms_state_sums<1>(s, red, w, l15, l4);     // its barrier: every read of X is done
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) al[r][t2] /= s[0][r];
                logZ += log(s[0][r]) * wt[r];
            }
            put(n, al);
        }
        // ---- backward: e holds e_{T-1}, al holds ah_{T-1}.  A row past the end of the range reads
        // nothing back: ones keep it finite, so that its zero weight gives zeros in sum xi --------
        double be[4][2], an[4][2];
        {
            double s[1][4], g[4][2];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    be[r][t2] = act[t2] ? 1.0 : 0.0;
                    g[r][t2] = al[r][t2] * be[r][t2];
                    an[r][t2] = !act[t2] ? 0.0 : live[r] ? a.aw[(cc[r] * T + (T - 2)) * K + st[t2]] : 1.0;
                }
                s[0][r] = g[r][0] + g[r][1];
            }
            __syncthreads();            // the sums of the last forward step are read by every wavefront
            hmms_state_sums<1>(s, red, w, l15, l4);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    g[r][t2] /= s[0][r];
                    if (g[r][t2] * wt[r] != 0.0) ge += g[r][t2] * wt[r] * e[r][t2];
                }
            put(T - 1, g);
            put_out(T - 1, g);
        }
        for (int n = T - 2; n >= 0; --n) {
            // e = e_{n+1}, be = bh_{n+1}, an = ah_n
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
                    X[(l4 + 4 * r) * XB + st[t2]] = hmms_exp(e[r][t2]) * be[r][t2];
            __syncthreads();
            double ap[4][2];
            load_e(n, en);
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2)
                    ap[r][t2] = !act[t2] ? 0.0 : (n > 0 && live[r])
                                    ? a.aw[(cc[r] * T + (n - 1)) * K + st[t2]] : 1.0;
            v4f64 acc[2][2];
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2) acc[t2][0] = acc[t2][1] = v4f64{0.0, 0.0, 0.0, 0.0};
#pragma unroll 2
            for (int q = 0; q < KP / 4; q += 2)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int j = 4 * (q + h) + l4;
                    const double av = X[l15 * XB + j];
#pragma unroll
                    for (int t2 = 0; t2 < 2; ++t2)
                        acc[t2][h] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Ps[st[t2] * PS + j],
                                                                          acc[t2][h], 0, 0, 0);
                }
            double s[2][4], g[4][2], u[4][2];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    u[r][t2] = acc[t2][0][r] + acc[t2][1][r];
                    g[r][t2] = an[r][t2] * u[r][t2];
                }
                s[0][r] = g[r][0] + g[r][1];
                s[1][r] = u[r][0] + u[r][1];
            }
            hmms_state_sums<2>(s, red, w, l15, l4);
            double as[4][2];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    g[r][t2] /= s[0][r];
                    be[r][t2] = u[r][t2] / s[1][r];
                    as[r][t2] = wt[r] == 0.0 ? 0.0 : an[r][t2] / s[0][r];
                    if (g[r][t2] * wt[r] != 0.0) ge += g[r][t2] * wt[r] * en[r][t2];
                    if (n == 0) z0acc[t2] += g[r][t2] * wt[r];
                }
            put(n, g);
            put_out(n, g);
            add_xi(as);
            for (int r = 0; r < 4; ++r)
                    for (int t2 = 0; t2 < 2; ++t2) {
                        if (!ZZ || !live[r] || !act[t2]) continue;
                        const double f = an[r][t2] / s[0][r];
                        const double *prow = Ps + st[t2] * PS, *vrow = X + (l4 + 4 * r) * XB;
                        double *z = a.zz + ((cc[r] * (T - 1) + n) * K + st[t2]) * K;
                        for (int j = 0; j < K; ++j) z[j] = f * prow[j] * vrow[j];
                    }
            __syncthreads();            // the tile is free for the step to come
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    an[r][t2] = ap[r][t2];
                    e[r][t2] = en[r][t2];
                }
        }
    }

    // ---- the partial of this workgroup -------------------------------------------------------------
    __syncthreads();
    const int64_t per = vmp_hmmw_chain_partial_doubles(K);
    double *part = a.part + (int64_t)blockIdx.x * per;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
        double v = z0acc[t2];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (l4 == 0 && act[t2]) part[st[t2]] = v;
    }
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int jt = 0; jt < 8; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = (2 * w + t2) * 16 + l4 + 4 * r, j = jt * 16 + l15;
                if (i < K && j < K)
                    part[K + i * K + j] = xi[t2][jt][r] * Ps[i * PS + j];
            }
    // log Z of a chain is the same in every lane that holds the chain: those of lane l15 = 0 of
    // the first wavefront, chains in ascending l4; gamma . e is a lane's own share
    double zs = logZ;
    zs += __shfl_xor(zs, 16, 64);
    zs += __shfl_xor(zs, 32, 64);
    X[tid] = ge;
    __syncthreads();
    block_halve_sum<256>(X, tid);
    if (tid == 0) {
        part[per - 2] = zs;
        part[per - 1] = X[0];
    }
}

// Fixed states: gamma and xi are one-hot, sum log Z = sum gamma . e = 0.  The lane mapping and the
// sum-xi product of hmms_chain_kernel with one-hot operands, so the counts are exact; nothing is
// multiplied by P.
__global__ __launch_bounds__(256) void hmms_labels_kernel(HmmsChainArgs a)
{
    __shared__ double X[TILE * XB];
    __shared__ double wts[TILE];
    const int T = a.T, K = a.K;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int st[2] = {(2 * w) * 16 + l15, (2 * w + 1) * 16 + l15};
    v4f64 xi[2][8];
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int jt = 0; jt < 8; ++jt) xi[t2][jt] = v4f64{0.0, 0.0, 0.0, 0.0};
    double z0acc[2] = {0.0, 0.0};
    const int64_t c_begin = (int64_t)blockIdx.x * a.cpw;
    const int64_t c_end = (c_begin + a.cpw < a.B) ? c_begin + a.cpw : a.B;
    for (int64_t c0 = c_begin; c0 < c_end; c0 += TILE) {
        __syncthreads();
        hmms_weights(a, c0, c_end, tid, wts);
        __syncthreads();
        for (int r = 0; r < 4; ++r) {               // chain l4 + 4 r: one-hot rows of gamma, z0, zz
            const int64_t c = c0 + l4 + 4 * r;
            if (c >= c_end) continue;
            const int32_t *lab = a.labels + c * T;
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    if (st[t2] >= K) continue;
                    const double g = st[t2] == lab[t] ? 1.0 : 0.0;
                    a.aw[(c * T + t) * K + st[t2]] = g;
                    if (a.gamma) a.gamma[(c * T + t) * K + st[t2]] = g;
                    if (a.z0 && t == 0) a.z0[c * K + st[t2]] = g;
                    if (a.zz && t > 0) {
                        double *z = a.zz + ((c * (T - 1) + (t - 1)) * K + st[t2]) * K;
                        for (int j = 0; j < K; ++j)
                            z[j] = (st[t2] == lab[t - 1] && j == lab[t]) ? 1.0 : 0.0;
                    }
                }
        }
        int prev[4] = {-1, -1, -1, -1};
        for (int t = 0; t < T; ++t) {
            double as[4][2];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t c = c0 + l4 + 4 * r;
                const int cur = a.labels[(c < c_end ? c : c_begin) * T + t];
                const double wt = wts[l4 + 4 * r];
#pragma unroll
                for (int t2 = 0; t2 < 2; ++t2) {
                    const double g = st[t2] == cur ? 1.0 : 0.0;
                    as[r][t2] = st[t2] == prev[r] ? wt : 0.0;
                    if (t == 0) z0acc[t2] += g * wt;
                    X[(l4 + 4 * r) * XB + st[t2]] = g;
                }
                prev[r] = cur;
            }
            if (t == 0) continue;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int jt = 0; jt < 8; ++jt) {
                    const double bv = X[(4 * q + l4) * XB + jt * 16 + l15];
#pragma unroll
                    for (int t2 = 0; t2 < 2; ++t2)
                        xi[t2][jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[q][t2], bv, xi[t2][jt], 0, 0, 0);
                }
            __syncthreads();
        }
    }
    const int64_t per = vmp_hmmw_chain_partial_doubles(K);
    double *part = a.part + (int64_t)blockIdx.x * per;
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2) {
        double v = z0acc[t2];
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (l4 == 0 && st[t2] < K) part[st[t2]] = v;
    }
#pragma unroll
    for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
        for (int jt = 0; jt < 8; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = (2 * w + t2) * 16 + l4 + 4 * r, j = jt * 16 + l15;
                if (i < K && j < K) part[K + i * K + j] = xi[t2][jt][r];
            }
    if (tid == 0) part[per - 2] = part[per - 1] = 0.0;
}

}  // namespace

int32_t vmp_hmms_chain(vmp_ctx *ctx, int64_t B, int T, int K, const double *E, const double *la0,
                       const double *lA, const int32_t *labels, const uint8_t *mask, double *aw,
                       double *cpart, double *gamma, double *z0, double *zz)
{
    if (B <= 0) return VMP_OK;
    HmmsChainArgs ca = {B, vmp_hmms_chains_per_wg(B), T, K, E, la0, lA, labels, mask, aw, cpart,
                        gamma, z0, zz};
    const dim3 grid((unsigned)vmp_hmms_chain_wgs(B));
    if (labels) {
        hipLaunchKernelGGL(hmms_labels_kernel, grid, dim3(256), 0, ctx->stream, ca);
        VMP_HIP_CHECK(ctx, hipGetLastError());
        return VMP_OK;
    }
    // 149 KB of LDS: asked for once per device and kernel; host threads may race
    const size_t lds = (size_t)vmp_hmms_lds_doubles() * sizeof(double);
    static std::once_flag raised[64];
    hipError_t err = hipSuccess;
    std::call_once(raised[ctx->device & 63], [&] {
        err = hipFuncSetAttribute((const void *)hmms_chain_kernel<false>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (err == hipSuccess)
            err = hipFuncSetAttribute((const void *)hmms_chain_kernel<true>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    VMP_HIP_CHECK(ctx, err);
    if (zz) hipLaunchKernelGGL(hmms_chain_kernel<true>, grid, dim3(256), lds, ctx->stream, ca);
    else hipLaunchKernelGGL(hmms_chain_kernel<false>, grid, dim3(256), lds, ctx->stream, ca);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

extern "C" {

int32_t vmp_hmm_states_limits(int32_t *max_K, int32_t *min_K, int32_t *max_M, int32_t *max_count)
{
    if (!max_K || !min_K || !max_M || !max_count) return VMP_ERR_INVALID;
    *max_K = VMP_HMMS_MAX_K;
    *min_K = VMP_HMMS_MIN_K;
    *max_M = VMP_HMMM_MAX_M;
    *max_count = VMP_HMMM_MAX_COUNT;
    return VMP_OK;
}

int32_t vmp_hmm_states_plan(int64_t B, int32_t T, int32_t M, int32_t K, int64_t *chains_per_wg,
                            int64_t *workspace_doubles)
{
    if (B < 0 || T < 2 || M < 1 || K < 1) return VMP_ERR_INVALID;
    if (K < VMP_HMMS_MIN_K || K > VMP_HMMS_MAX_K || M > VMP_HMMM_MAX_M) return VMP_ERR_UNSUPPORTED;
    if (!chains_per_wg || !workspace_doubles) return VMP_ERR_INVALID;
    *chains_per_wg = vmp_hmms_chains_per_wg(B);
    *workspace_doubles = vmp_hmms_workspace_doubles(B, T, M, K);
    return VMP_OK;
}

int32_t vmp_hmm_states_pass(vmp_ctx *ctx, int64_t B, int32_t T, int32_t M, int32_t K,
                            const uint16_t *x_packed, const double *elogPt, const double *elog_a0,
                            const double *elog_A, const int32_t *labels, const uint8_t *mask,
                            double *ws, double *z0sum, double *xisum, double *S, double *scal,
                            double *gamma, double *z0, double *zz)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, B >= 0 && T >= 2 && M >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K >= VMP_HMMS_MIN_K && K <= VMP_HMMS_MAX_K && M <= VMP_HMMM_MAX_M,
                VMP_ERR_UNSUPPORTED, "M = %d, K = %d outside the limits (M <= %d, %d <= K <= %d)", M,
                K, VMP_HMMM_MAX_M, VMP_HMMS_MIN_K, VMP_HMMS_MAX_K);
    VMP_REQUIRE(ctx, ctx && elog_a0 && elog_A && ws && z0sum && xisum && S && scal
                     && (B == 0 || x_packed), VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    return vmp_hmmm_stages(ctx, B, T, M, K, vmp_hmms_chain_wgs(B), vmp_hmms_chain, x_packed, elogPt,
                           elog_a0, elog_A, labels, mask, ws, z0sum, xisum, S, scal, gamma, z0, zz);
}

}  // extern "C"
