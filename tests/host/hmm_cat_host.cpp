// TEST DOUBLE: the chain pass of csrc/vmp_hmm_cat.hip on the host, built with g++ from the very
// header the kernels include (csrc/vmp_hmm_fused_dev.h).  Workgroups are walked one after the
// other, a workgroup's chains by lane group, the lanes of a chain as an array reduced by the
// header's butterflies -- the order of every addition is the one the header states.  y (B x T
// int32 words), Pt (M x K, word-major) or null, mask (B x T bytes, 1 = observed) or null.  A step
// that is masked or whose word is outside [0, M) (vmp_hmmf_cat_observed) has e = 0, adds nothing
// to S or to sum gamma . e, and its word indexes nothing; a chain whose mask row is all zero has
// weight 0 in every sum.
#include <math.h>
#include <stdint.h>
#include <vector>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_hmm_fused_dev.h"

namespace {

double group_lse_parts(const double *q, int KP, double *M)
{
    double v[VMP_HMMF_MAX_K];
    for (int j = 0; j < KP; ++j) v[j] = q[j];
    vmp_hmmf_group_max_host(v, KP);
    *M = v[0];
    for (int j = 0; j < KP; ++j) v[j] = vmp_hmmf_exp_shift(q[j], *M);
    vmp_hmmf_group_sum_host(v, KP);
    return v[0];
}

void softmax(const double *g, int KP, double *out)
{
    double M;
    const double S = group_lse_parts(g, KP, &M);
    for (int j = 0; j < KP; ++j) out[j] = vmp_hmmf_exp_shift(g[j], M) / S;
}

}  // namespace

extern "C" {

int hmmc_max_k() { return VMP_HMMF_MAX_K; }
int hmmc_max_m() { return VMP_HMMF_MAX_M; }
int64_t hmmc_partial_doubles(int M, int K) { return vmp_hmmf_cat_partial_doubles(M, K); }
int64_t hmmc_chains_per_wg(int64_t B, int M, int K) { return vmp_hmmf_cat_chains_per_wg(B, M, K); }
int64_t hmmc_wgs(int64_t B, int M, int K) { return vmp_hmmf_cat_wgs(B, M, K); }
int64_t hmmc_workspace_doubles(int64_t B, int T, int M, int K)
{
    return vmp_hmmf_cat_workspace_doubles(B, T, M, K);
}

// z0sum (K), xisum (K x K), S (M x K), scal[0] = sum log Z, scal[1] = sum gamma . e;
// gamma (B T K), z0 (B K), zz (B (T-1) K K) or null
void hmmc_pass(int64_t B, int T, int M, int K, const int32_t *y, const double *Pt,
               const double *la0, const double *lA, const int32_t *labels, const uint8_t *mask,
               double *z0sum, double *xisum, double *S, double *scal, double *gamma_out,
               double *z0_out, double *zz_out)
{
    const int KP = vmp_hmmf_kpad(K), G = 64 / KP;
    const int64_t cpw = vmp_hmmf_cat_chains_per_wg(B, M, K), nw = vmp_hmmf_cat_wgs(B, M, K);
    const int64_t per = vmp_hmmf_cat_partial_doubles(M, K);
    std::vector<double> part((size_t)(nw * per), 0.0);
    std::vector<double> As(KP * KP, -INFINITY), ATs(KP * KP, -INFINITY);
    for (int i = 0; i < K; ++i)
        for (int j = 0; j < K; ++j) As[i * KP + j] = ATs[j * KP + i] = lA[i * K + j];
    std::vector<double> la((size_t)T * KP);
    double e[VMP_HMMF_MAX_K], q[VMP_HMMF_MAX_K];
    double lb[VMP_HMMF_MAX_K], gl[VMP_HMMF_MAX_K], gam[VMP_HMMF_MAX_K], u[VMP_HMMF_MAX_K];
    double p[VMP_HMMF_MAX_K], gw[VMP_HMMF_MAX_K];

    for (int64_t wg = 0; wg < nw; ++wg) {
        const int64_t cb = wg * cpw, ce = cb + cpw < B ? cb + cpw : B;
        std::vector<double> xi((size_t)G * KP * KP, 0.0), sacc((size_t)M * G * KP, 0.0);
        std::vector<double> z0a(G * KP, 0.0), ge(G * KP, 0.0), lz(G, 0.0);
        for (int64_t c = cb; c < ce; ++c) {
            const int g = (int)((c - cb) % G);
            double *xg = xi.data() + (size_t)g * KP * KP;          // [i * KP + j]
            const int32_t *yrow = y + c * (int64_t)T;
            const uint8_t *mrow = mask ? mask + c * (int64_t)T : nullptr;
            const double w = (!mask || vmp_hmmf_chain_observed(mrow, T)) ? 1.0 : 0.0;
            int wd = -1;                                    // of the step of the last emit()
            auto emit = [&](int t) {
                wd = -1;
                if (!mrow || mrow[t] != 0) {
                    const int32_t v = yrow[t];
                    if (vmp_hmmf_cat_observed(true, v, M)) wd = v;
                }
                for (int j = 0; j < KP; ++j)
                    e[j] = (wd >= 0 && Pt && j < K) ? Pt[(int64_t)wd * K + j] : 0.0;
            };
            // gm holds gamma * w, as in the kernel
            auto accumulate = [&](const double *gm, bool with_e) {
                if (wd < 0) return;
                for (int j = 0; j < KP; ++j) {
                    if (with_e && gm[j] != 0.0) ge[g * KP + j] += gm[j] * e[j];
                    sacc[(size_t)wd * G * KP + g * KP + j] += gm[j];
                }
            };
            if (labels) {
                int prev = -1;
                for (int t = 0; t < T; ++t) {
                    const int cur = labels[c * T + t];
                    emit(t);
                    for (int j = 0; j < KP; ++j) gam[j] = j == cur ? 1.0 : 0.0;
                    for (int j = 0; j < KP; ++j) gw[j] = gam[j] * w;
                    accumulate(gw, false);
                    for (int j = 0; j < K; ++j) {
                        if (t == 0) {
                            z0a[g * KP + j] += gam[j] * w;
                            if (z0_out) z0_out[c * K + j] = gam[j];
                        } else {
                            for (int i = 0; i < K; ++i) {
                                const double x = i == prev ? gam[j] : 0.0;
                                xg[i * KP + j] += x * w;
                                if (zz_out)
                                    zz_out[((c * (int64_t)(T - 1) + t - 1) * K + i) * K + j] = x;
                            }
                        }
                        if (gamma_out) gamma_out[(c * (int64_t)T + t) * K + j] = gam[j];
                    }
                    prev = cur;
                }
                continue;
            }
            // forward
            emit(0);
            for (int j = 0; j < KP; ++j) la[j] = j < K ? la0[j] + e[j] : -INFINITY;
            for (int n = 1; n < T; ++n) {
                emit(n);
                const double *v = la.data() + (size_t)(n - 1) * KP;
                for (int j = 0; j < KP; ++j) {
                    double m, s;
                    vmp_hmmf_column(v, As.data() + j, KP, K, &m, &s);
                    q[j] = j < K ? m + log(s) + e[j] : -INFINITY;
                }
                double Mx;
                const double Sx = group_lse_parts(q, KP, &Mx);
                const double cn = Mx + log(Sx);
                lz[g] += cn * w;
                for (int j = 0; j < KP; ++j) la[(size_t)n * KP + j] = q[j] - cn;
            }
            // backward
            for (int j = 0; j < KP; ++j) lb[j] = 0.0;
            for (int n = T - 2; n >= 0; --n) {
                emit(n + 1);
                const double *lnext = la.data() + (size_t)(n + 1) * KP;
                const double *v = la.data() + (size_t)n * KP;
                for (int j = 0; j < KP; ++j) {
                    gl[j] = j < K ? lnext[j] + lb[j] : -INFINITY;
                    u[j] = j < K ? e[j] + lb[j] : -INFINITY;
                }
                softmax(gl, KP, gam);
                for (int j = 0; j < KP; ++j) {
                    double m = -INFINITY, s = 0.0;
                    for (int i = 0; i < KP; ++i) m = fmax(m, v[i] + As[i * KP + j]);
                    for (int i = 0; i < KP; ++i) {
                        p[i] = vmp_hmmf_exp_shift(v[i] + As[i * KP + j], m);
                        s += p[i];
                    }
                    const double r = vmp_hmmf_ratio(gam[j], s);
                    for (int i = 0; i < KP; ++i) {
                        const double x = p[i] * r;
                        xg[i * KP + j] += x * w;
                        if (zz_out && i < K && j < K)
                            zz_out[((c * (int64_t)(T - 1) + n) * K + i) * K + j] = x;
                    }
                    if (gamma_out && j < K) gamma_out[(c * (int64_t)T + n + 1) * K + j] = gam[j];
                }
                for (int j = 0; j < KP; ++j) gw[j] = gam[j] * w;
                accumulate(gw, true);
                double lbn[VMP_HMMF_MAX_K], mx[VMP_HMMF_MAX_K];
                for (int i = 0; i < KP; ++i) {
                    double mr, sr;
                    vmp_hmmf_column(u, ATs.data() + i, KP, K, &mr, &sr);
                    lbn[i] = i < K ? mr + log(sr) : -INFINITY;
                    mx[i] = lbn[i];
                }
                vmp_hmmf_group_max_host(mx, KP);
                for (int i = 0; i < KP; ++i) lb[i] = lbn[i] - mx[0];
            }
            emit(0);
            for (int j = 0; j < KP; ++j) gl[j] = j < K ? la[j] + lb[j] : -INFINITY;
            softmax(gl, KP, gam);
            for (int j = 0; j < KP; ++j) gw[j] = gam[j] * w;
            accumulate(gw, true);
            for (int j = 0; j < K; ++j) {
                z0a[g * KP + j] += gam[j] * w;
                if (gamma_out) gamma_out[c * (int64_t)T * K + j] = gam[j];
                if (z0_out) z0_out[c * K + j] = gam[j];
            }
        }
        double *pt = part.data() + wg * per;
        for (int j = 0; j < K; ++j) {
            double t = z0a[j];
            for (int g = 1; g < G; ++g) t += z0a[g * KP + j];
            pt[j] = t;
            for (int i = 0; i < K; ++i) {
                double x = xi[i * KP + j];
                for (int g = 1; g < G; ++g) x += xi[(size_t)g * KP * KP + i * KP + j];
                pt[K + i * K + j] = x;
            }
            for (int m = 0; m < M; ++m) {
                double x = 0.0;
                for (int g = 0; g < G; ++g) x += sacc[(size_t)m * G * KP + g * KP + j];
                pt[K + K * K + (int64_t)m * K + j] = x;
            }
        }
        double zs = 0.0, gs = 0.0;
        for (int g = 0; g < G; ++g) zs += lz[g];
        for (int l = 0; l < G * KP; ++l) gs += ge[l];
        pt[per - 2] = zs;
        pt[per - 1] = gs;
    }
    const int64_t oS = K + (int64_t)K * K;
    for (int64_t el = 0; el < per; ++el) {
        double v = 0.0;
        for (int64_t w = 0; w < nw; ++w) v += part[w * per + el];
        if (el < K) z0sum[el] = v;
        else if (el < oS) xisum[el - K] = v;
        else if (el < per - 2) S[el - oS] = v;
        else scal[el - (per - 2)] = v;
    }
}

}  // extern "C"
