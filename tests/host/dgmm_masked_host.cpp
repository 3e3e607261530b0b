// TEST DOUBLE: the pack, the tables, the plate pass and the updates of csrc/vmp_dgmm_masked.hip on
// the host, built with g++ from the very header the kernels include
// (csrc/vmp_dgmm_masked_dev.h); the special functions of vmp_common.h come in ahead of this file
// (host_build.special_functions_text).  Chunks are walked one after the other, a chunk's rows in
// tiles of 64, the logit in steps of 4 columns (m g, then yt h, then yt^2 q), the softmax, the
// slots and the two levels of the statistics as in tests/host/dgmm_host.cpp -- the order of every
// addition is the one the header states.
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_dgmm_masked_dev.h"

extern "C" {

int dgmmm_max_k() { return VMP_DGMM_MASKED_MAX_K; }
int dgmmm_max_d() { return VMP_DGMM_MASKED_MAX_D; }
int dgmmm_dblock() { return VMP_DGMM_MASKED_DBLOCK; }
int64_t dgmmm_chunk_rows(int64_t N, int D, int K) { return vmp_dgmm_masked_chunk_rows(N, D, K); }
int64_t dgmmm_chunks(int64_t N, int D, int K) { return vmp_dgmm_masked_chunks(N, D, K); }
int64_t dgmmm_partial_doubles(int D, int K) { return vmp_dgmm_masked_partial_doubles(D, K); }

// out (N x D) and the number of observed entries
int64_t dgmmm_pack(int64_t N, int D, const double *y, const uint8_t *mask, double *out)
{
    int64_t count = 0;
    for (int64_t i = 0; i < N * D; ++i) {
        const int ob = mask[i] != 0;
        out[i] = vmp_dgmm_pack_value(y[i], ob);
        count += ob;
    }
    return count;
}

void dgmmm_tables(int D, int K, const double *mu_mom, const double *tau_mom, const double *elog_pi,
                  double *h, double *q, double *g, double *c)
{
    const bool have = mu_mom && tau_mom;
    for (int i = 0; i < D * K; ++i) {
        h[i] = have ? vmp_dgmm_h(tau_mom[2 * i], mu_mom[2 * i]) : 0.0;
        q[i] = have ? vmp_dgmm_q(tau_mom[2 * i]) : 0.0;
        g[i] = have ? vmp_dgmm_g(tau_mom[2 * i], tau_mom[2 * i + 1], mu_mom[2 * i + 1]) : 0.0;
    }
    double m = elog_pi[0];
    for (int k = 1; k < K; ++k) m = fmax(m, elog_pi[k]);
    for (int k = 0; k < K; ++k) c[k] = elog_pi[k] - m;
}

// S1, S2, M (D x K), Nk (K), scal[0] = sum lse; r_out (N x K) or null; y is the packed array
void dgmmm_pass(int64_t N, int D, int K, const double *y, const int32_t *labels, const double *h,
                const double *q, const double *g, const double *c, double *S1, double *S2,
                double *M, double *Nk, double *scal, double *r_out)
{
    const int KP = vmp_dgmm_kpad(K);
    const int64_t chunk = vmp_dgmm_masked_chunk_rows(N, D, K), nc = vmp_dgmm_masked_chunks(N, D, K);
    const int64_t per = vmp_dgmm_masked_partial_doubles(D, K), DK = (int64_t)D * K;
    std::vector<double> part((size_t)(nc * per), 0.0);
    double logit[VMP_DGMM_MASKED_MAX_K], r[VMP_DGMM_MASKED_MAX_K], v[16];
    for (int64_t ch = 0; ch < nc; ++ch) {
        const int64_t r0 = ch * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
        double *p1 = part.data() + ch * per, *p2 = p1 + DK, *p3 = p2 + DK;   // [k][d]
        std::vector<double> nk(16 * K, 0.0), t1((size_t)DK), t2((size_t)DK), t3((size_t)DK);
        double ls[16] = {0};
        for (int64_t row = r0; row < r1; ++row) {
            if ((row - r0) % VMP_DGMM_TILE == 0) {            // a new tile: its sums start at zero
                std::fill(t1.begin(), t1.end(), 0.0);
                std::fill(t2.begin(), t2.end(), 0.0);
                std::fill(t3.begin(), t3.end(), 0.0);
            }
            const double *yr = y + row * D;
            const int slot = vmp_dgmm_slot((int)((row - r0) % VMP_DGMM_TILE));
            bool obs = false;
            for (int d = 0; d < D; ++d) obs = obs || vmp_dgmm_observed(yr[d]);
            double lse = 0.0;
            if (labels) {
                for (int k = 0; k < K; ++k) r[k] = k == labels[row] ? 1.0 : 0.0;
            } else {
                for (int k = 0; k < KP; ++k) {
                    double l = 0.0;
                    if (k < K)
                        for (int d0 = 0; d0 < D; d0 += 4) {   // a step: m g, then yt h, then yt^2 q
                            const int d1 = d0 + 4 < D ? d0 + 4 : D;
                            for (int d = d0; d < d1; ++d)
                                l = vmp_dgmm_mac(l, vmp_dgmm_mask_value(yr[d]), g[d * K + k]);
                            for (int d = d0; d < d1; ++d)
                                l = vmp_dgmm_mac(l, vmp_dgmm_masked_value(yr[d]), h[d * K + k]);
                            for (int d = d0; d < d1; ++d)
                                l = vmp_dgmm_mac(l, vmp_dgmm_square(vmp_dgmm_masked_value(yr[d])),
                                                 q[d * K + k]);
                        }
                    logit[k] = vmp_dgmm_logit_finish(l, k < K ? c[k] : -INFINITY);
                }
                double m = logit[0];
                for (int k = 1; k < KP; ++k) m = fmax(m, logit[k]);
                for (int j = 0; j < 16; ++j) {
                    double s = 0.0;
                    for (int k = j; k < KP; k += 16) s += vmp_dgmm_shifted_exp(logit[k], m);
                    v[j] = s;
                }
                vmp_dgmm_group_sum_host(v);
                lse = vmp_dgmm_lse(m, v[0]);
                for (int k = 0; k < K; ++k) r[k] = vmp_dgmm_resp(logit[k], lse);
            }
            if (r_out)
                for (int k = 0; k < K; ++k) r_out[row * K + k] = r[k];
            if (obs) ls[slot] += lse;
            for (int k = 0; k < K; ++k) {
                if (obs) nk[slot * K + k] += r[k];
                for (int d = 0; d < D; ++d) {
                    const double yt = vmp_dgmm_masked_value(yr[d]);
                    t1[k * D + d] = vmp_dgmm_mac(t1[k * D + d], r[k], yt);
                    t2[k * D + d] = vmp_dgmm_mac(t2[k * D + d], r[k], vmp_dgmm_square(yt));
                    t3[k * D + d] = vmp_dgmm_mac(t3[k * D + d], r[k], vmp_dgmm_mask_value(yr[d]));
                }
            }
            if ((row - r0) % VMP_DGMM_TILE == VMP_DGMM_TILE - 1 || row == r1 - 1)
                for (int64_t i = 0; i < DK; ++i) {            // the tile's sums, in tile order
                    p1[i] += t1[i];
                    p2[i] += t2[i];
                    p3[i] += t3[i];
                }
        }
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int s = 0; s < 16; ++s) t += nk[s * K + k];
            p1[3 * DK + k] = t;
        }
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += ls[s];
        p1[3 * DK + K] = t;
    }
    for (int k = 0; k < K; ++k) {
        double n = 0.0;
        for (int64_t ch = 0; ch < nc; ++ch) n += part[ch * per + 3 * DK + k];
        Nk[k] = n;
        for (int d = 0; d < D; ++d) {
            double s1 = 0.0, s2 = 0.0, m = 0.0;
            for (int64_t ch = 0; ch < nc; ++ch) {
                s1 += part[ch * per + k * D + d];
                s2 += part[ch * per + DK + k * D + d];
                m += part[ch * per + 2 * DK + k * D + d];
            }
            S1[d * K + k] = s1;
            S2[d * K + k] = s2;
            M[d * K + k] = m;
        }
    }
    double t = 0.0;
    for (int64_t ch = 0; ch < nc; ++ch) t += part[ch * per + 3 * DK + K];
    scal[0] = t;
}

double dgmmm_dots(double s1h, double s2q, double mg) { return vmp_dgmm_masked_dots(s1h, s2q, mg); }

// par, mom: (D K, 2); bound: the 256 threads' sums halved eight times; null statistics: the prior
void dgmmm_update(int D, int K, int which, const double *prior_a, const double *prior_b,
                  const double *S1, const double *S2, const double *M, const double *other,
                  double *par, double *mom, double *bound)
{
    const bool stats = S1 && S2 && M && other;
    double v[VMP_DGMM_NT];
    for (int tid = 0; tid < VMP_DGMM_NT; ++tid) {
        double t = 0.0;
        for (int e = tid; e < D * K; e += VMP_DGMM_NT) {
            const double cnt = stats ? M[e] : 0.0, s1 = stats ? S1[e] : 0.0, s2 = stats ? S2[e] : 0.0;
            const double o0 = stats ? other[2 * e] : 0.0, o1 = stats ? other[2 * e + 1] : 0.0;
            if (which == 0)
                t += vmp_dgmm_update_mu(prior_a[e], prior_b[e], o0, cnt, s1, par + 2 * e, mom + 2 * e);
            else
                t += vmp_dgmm_masked_update_tau(prior_a[e], prior_b[e], o0, o1, cnt, s1, s2,
                                                par + 2 * e, mom + 2 * e);
        }
        v[tid] = t;
    }
    for (int off = VMP_DGMM_NT / 2; off > 0; off >>= 1)
        for (int i = 0; i < off; ++i) v[i] += v[i + off];
    bound[0] = v[0];
}

}  // extern "C"
