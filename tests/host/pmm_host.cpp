// TEST DOUBLE: the pack, the tables, the plate pass and the update of csrc/vmp_pmm.hip on the host,
// built with g++ from the very header the kernels include (csrc/vmp_pmm_dev.h); the special
// functions of vmp_common.h come in ahead of this file (host_build.special_functions_text).  Chunks
// are walked one after the other, a chunk's rows in tiles of 64, the logit in steps of 4 columns
// (xt l, then m (-lb)), the softmax, the slots and the two levels of the statistics as in
// tests/host/dgmm_masked_host.cpp -- the order of every addition is the one the header states.
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_pmm_dev.h"

extern "C" {

int pmm_max_k() { return VMP_PMM_MAX_K; }
int pmm_max_d() { return VMP_PMM_MAX_D; }
int pmm_max_count() { return VMP_PMM_MAX_COUNT; }
int pmm_dblock(int hidden) { return vmp_pmm_dblock(hidden); }
int64_t pmm_chunk_rows(int64_t N, int D, int K) { return vmp_pmm_chunk_rows(N, D, K); }
int64_t pmm_chunks(int64_t N, int D, int K) { return vmp_pmm_chunks(N, D, K); }
int64_t pmm_workspace_doubles(int64_t N, int D, int K) { return vmp_pmm_workspace_doubles(N, D, K); }
int64_t pmm_pack_span(int64_t n) { return vmp_pmm_pack_span(n); }
int64_t pmm_pack_blocks(int64_t n) { return vmp_pmm_pack_blocks(n); }

// xp (N x D), flags (3), counts (2), lgam (1)
void pmm_pack(int64_t N, int D, int dtype, const void *x, const uint8_t *mask, uint16_t *xp,
              int32_t *flags, int64_t *counts, double *lgam)
{
    const int64_t n = N * D, span = vmp_pmm_pack_span(n), nb = n > 0 ? vmp_pmm_pack_blocks(n) : 0;
    double total = 0.0, total_e = 0.0;
    int64_t hidden = 0;
    int bad = 0;
    for (int64_t b = 0; b < nb; ++b) {
        double v[VMP_PMM_NT];
        for (int t = 0; t < VMP_PMM_NT; ++t) {
            double lg = 0.0, lge = 0.0;
            for (int64_t i = t; i < span; i += VMP_PMM_NT) {
                const int64_t e = b * span + i;
                if (e >= n) break;
                const uint16_t p = vmp_pmm_pack_at(dtype, x, e, mask ? mask[e] != 0 : true, &bad);
                xp[e] = p;
                vmp_pmm_sum_add(&lg, &lge, vmp_pmm_lgamma1(p));
                hidden += vmp_pmm_observed(p) ? 0 : 1;
            }
            v[t] = lg + lge;
        }
        for (int off = VMP_PMM_NT / 2; off > 0; off >>= 1)
            for (int i = 0; i < off; ++i) v[i] += v[i + off];
        vmp_pmm_sum_add(&total, &total_e, v[0]);
    }
    if (bad & VMP_PMM_BAD_INVALID) flags[0] = 1;
    if (bad & VMP_PMM_BAD_ABOVE) flags[1] = 1;
    if (bad & VMP_PMM_BAD_FRACTION) flags[2] = 1;
    counts[0] = n - hidden;
    counts[1] = hidden;
    lgam[0] = total + total_e;
}

void pmm_tables(int D, int K, int form, const double *lam_mom, const double *elog_pi, double *l,
                double *lb, double *c, double *lsum)
{
    for (int i = 0; i < D * K; ++i) {
        const int e0 = i / K * K;
        l[i] = lam_mom ? vmp_pmm_table(lam_mom[2 * i + 1], lam_mom[2 * e0 + 1], form) : 0.0;
        lb[i] = lam_mom ? vmp_pmm_table(lam_mom[2 * i], lam_mom[2 * e0], form) : 0.0;
    }
    double cs[VMP_PMM_MAX_K];
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
        if (lam_mom)
            for (int d = 0; d < D; ++d)
                t += vmp_pmm_table(lam_mom[2 * (d * K + k)], lam_mom[2 * (d * K)], form);
        if (lsum) lsum[k] = t;
        cs[k] = vmp_pmm_c_raw(elog_pi[k], t, form);
    }
    double m = cs[0];
    for (int k = 1; k < K; ++k) m = fmax(m, cs[k]);
    for (int k = 0; k < K; ++k) c[k] = cs[k] - m;
}

// what pmm_pass_kernel leaves: a partial per chunk, vmp_pmm_partial_doubles(D, K, hidden) apart --
// S (K x D), with hidden entries M (K x D), N_k (K), sum lse; r_out (N x K) or null.  The pass of
// tests/host/mmm_host.cpp starts here as well, as vmp_mmm_pass starts with that kernel.
static std::vector<double> pmm_pass_partials(int64_t N, int D, int K, int hidden, const uint16_t *x,
                                             const int32_t *labels, const double *l,
                                             const double *lb, const double *c, double *r_out)
{
    const int KP = vmp_pmm_kpad(K), ns = hidden ? 2 : 1;
    const int64_t chunk = vmp_pmm_chunk_rows(N, D, K), nc = vmp_pmm_chunks(N, D, K);
    const int64_t per = vmp_pmm_partial_doubles(D, K, hidden), DK = (int64_t)D * K;
    std::vector<double> part((size_t)(nc * per), 0.0);
    double logit[VMP_PMM_MAX_K], ex[VMP_PMM_MAX_K], r[VMP_PMM_MAX_K], v[16];
    for (int64_t ch = 0; ch < nc; ++ch) {
        const int64_t r0 = ch * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
        double *p1 = part.data() + ch * per, *p2 = p1 + DK;             // [k][d]; p2 with hidden
        std::vector<double> nk(16 * K, 0.0), t1((size_t)DK), t2((size_t)DK);
        double ls[16] = {0};
        for (int64_t row = r0; row < r1; ++row) {
            if ((row - r0) % VMP_PMM_TILE == 0) {             // a new tile: its sums start at zero
                std::fill(t1.begin(), t1.end(), 0.0);
                std::fill(t2.begin(), t2.end(), 0.0);
            }
            const uint16_t *xr = x + row * D;
            const int slot = vmp_pmm_slot((int)((row - r0) % VMP_PMM_TILE));
            bool obs = !hidden;
            for (int d = 0; d < D; ++d) obs = obs || vmp_pmm_observed(xr[d]);
            double lse = 0.0;
            if (labels) {
                for (int k = 0; k < K; ++k) r[k] = k == labels[row] ? 1.0 : 0.0;
            } else {
                for (int k = 0; k < KP; ++k) {
                    double lg = 0.0;
                    if (k < K)
                        for (int d0 = 0; d0 < D; d0 += 4) {   // a step: xt l, then m (-lb)
                            const int d1 = d0 + 4 < D ? d0 + 4 : D;
                            for (int d = d0; d < d1; ++d)
                                lg = vmp_pmm_mac(lg, hidden ? vmp_pmm_masked_count(xr[d])
                                                            : vmp_pmm_count(xr[d]), l[d * K + k]);
                            if (hidden)
                                for (int d = d0; d < d1; ++d)
                                    lg = vmp_pmm_mac(lg, vmp_pmm_mask_value(xr[d]),
                                                     vmp_pmm_neg(lb[d * K + k]));
                        }
                    logit[k] = vmp_dgmm_logit_finish(lg, k < K ? c[k] : -INFINITY);
                }
                double m = logit[0];
                for (int k = 1; k < KP; ++k) m = fmax(m, logit[k]);
                for (int j = 0; j < 16; ++j) {
                    double s = 0.0;
                    for (int k = j; k < KP; k += 16) {
                        ex[k] = vmp_dgmm_shifted_exp(logit[k], m);
                        s += ex[k];
                    }
                    v[j] = s;
                }
                vmp_dgmm_group_sum_host(v);
                lse = vmp_dgmm_lse(m, v[0]);
                for (int k = 0; k < K; ++k) r[k] = vmp_pmm_resp(ex[k], v[0]);
            }
            if (r_out)
                for (int k = 0; k < K; ++k) r_out[row * K + k] = r[k];
            if (obs) ls[slot] += lse;
            for (int k = 0; k < K; ++k) {
                if (obs) nk[slot * K + k] += r[k];
                for (int d = 0; d < D; ++d) {
                    t1[k * D + d] = vmp_pmm_mac(t1[k * D + d], r[k],
                                                hidden ? vmp_pmm_masked_count(xr[d])
                                                       : vmp_pmm_count(xr[d]));
                    if (hidden)
                        t2[k * D + d] = vmp_pmm_mac(t2[k * D + d], r[k], vmp_pmm_mask_value(xr[d]));
                }
            }
            if ((row - r0) % VMP_PMM_TILE == VMP_PMM_TILE - 1 || row == r1 - 1)
                for (int64_t i = 0; i < DK; ++i) {            // the tile's sums, in tile order
                    p1[i] += t1[i];
                    if (hidden) p2[i] += t2[i];
                }
        }
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int s = 0; s < 16; ++s) t += nk[s * K + k];
            p1[ns * DK + k] = t;
        }
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += ls[s];
        p1[ns * DK + K] = t;
    }
    return part;
}

// S, M (D x K; M only with hidden), Nk (K), scal[0] = sum lse; r_out (N x K) or null
void pmm_pass(int64_t N, int D, int K, int hidden, const uint16_t *x, const int32_t *labels,
              const double *l, const double *lb, const double *c, double *S, double *M, double *Nk,
              double *scal, double *r_out)
{
    const std::vector<double> part = pmm_pass_partials(N, D, K, hidden, x, labels, l, lb, c, r_out);
    const int ns = hidden ? 2 : 1;
    const int64_t nc = vmp_pmm_chunks(N, D, K);
    const int64_t per = vmp_pmm_partial_doubles(D, K, hidden), DK = (int64_t)D * K;
    for (int k = 0; k < K; ++k) {
        double n = 0.0;
        for (int64_t ch = 0; ch < nc; ++ch) n += part[ch * per + ns * DK + k];
        Nk[k] = n;
        for (int d = 0; d < D; ++d) {
            double s = 0.0, m = 0.0;
            for (int64_t ch = 0; ch < nc; ++ch) {
                s += part[ch * per + k * D + d];
                if (hidden) m += part[ch * per + DK + k * D + d];
            }
            S[d * K + k] = s;
            if (hidden) M[d * K + k] = m;
        }
    }
    double t = 0.0;
    for (int64_t ch = 0; ch < nc; ++ch) t += part[ch * per + ns * DK + K];
    scal[0] = t;
}

double pmm_dots(double s_l, double m_lb) { return vmp_pmm_dots(s_l, m_lb); }

// par, mom: (D K, 2); bound: the 256 threads' sums halved eight times; null statistics: the prior
void pmm_update(int D, int K, int per_element, const double *prior_a, const double *prior_b,
                const double *S, const double *cnt, double *par, double *mom, double *bound)
{
    const bool stats = S && cnt;
    double v[VMP_PMM_NT];
    for (int tid = 0; tid < VMP_PMM_NT; ++tid) {
        double t = 0.0;
        for (int e = tid; e < D * K; e += VMP_PMM_NT) {
            const double s = stats ? S[e] : 0.0;
            const double n = stats ? (per_element ? cnt[e] : cnt[e % K]) : 0.0;
            t += vmp_pmm_update_lam(prior_a[e], prior_b[e], s, n, par + 2 * e, mom + 2 * e);
        }
        v[tid] = t;
    }
    for (int off = VMP_PMM_NT / 2; off > 0; off >>= 1)
        for (int i = 0; i < off; ++i) v[i] += v[i + off];
    bound[0] = v[0];
}

}  // extern "C"
