// TEST DOUBLE: the pack, the tables and the two-plane plate pass of csrc/vmp_binm.hip on the host,
// built with g++ from the very header the kernels include (csrc/vmp_binm_dev.h); the special
// functions of vmp_common.h come in ahead of this file (host_build.special_functions_text).  Chunks
// are walked one after the other, a chunk's rows in tiles of 64, the logit in steps of 4 columns
// (xt l1, then nt l0), the softmax, the slots and the two levels of the statistics as in
// tests/host/pmm_host.cpp -- the order of every addition is the one the header states.  The
// one-plane form is the Poisson pass: tests/binm_host.py runs it on tests/host/pmm_host.cpp and
// finishes it with binm_const below.
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_binm_dev.h"

extern "C" {

int binm_max_k() { return VMP_BINM_MAX_K; }
int binm_max_d() { return VMP_BINM_MAX_D; }
int binm_max_trials() { return VMP_BINM_MAX_TRIALS; }
int binm_dblock() { return VMP_BINM_DBLOCK; }
int64_t binm_chunk_rows(int64_t N, int D, int K) { return vmp_pmm_chunk_rows(N, D, K); }
int64_t binm_workspace_doubles(int64_t N, int D, int K) { return vmp_binm_workspace_doubles(N, D, K); }

static void binm_pack_one(int dtype, const void *x, int64_t e, int64_t tn, bool seen, uint16_t *xo,
                     uint16_t *no, int *bad)
{
    switch (dtype) {
    case 0: vmp_binm_pack_f64(((const double *)x)[e], tn, seen, xo, no, bad); break;
    case 1: vmp_binm_pack_i64(((const int64_t *)x)[e], tn, seen, xo, no, bad); break;
    case 2: vmp_binm_pack_i64((int64_t)((const uint8_t *)x)[e], tn, seen, xo, no, bad); break;
    default: vmp_binm_pack_i64((int64_t)((const int32_t *)x)[e], tn, seen, xo, no, bad); break;
    }
}

// xp, np (N x D), flags (4), counts (3), lcoef (1)
void binm_pack(int64_t N, int D, int dtype, const void *x, const int64_t *trials, int64_t ts_n,
               int64_t ts_d, const uint8_t *mask, uint16_t *xp, uint16_t *np, int32_t *flags,
               int64_t *counts, double *lcoef)
{
    const int64_t n = N * D, span = vmp_pmm_pack_span(n), nb = n > 0 ? vmp_pmm_pack_blocks(n) : 0;
    double total = 0.0, total_e = 0.0;
    int64_t hidden = 0;
    int bad = 0, var = 0;
    for (int64_t b = 0; b < nb; ++b) {
        double v[VMP_PMM_NT];
        for (int t = 0; t < VMP_PMM_NT; ++t) {
            double lc = 0.0, lce = 0.0;
            for (int64_t i = t; i < span; i += VMP_PMM_NT) {
                const int64_t e = b * span + i;
                if (e >= n) break;
                const int64_t row = e / D, d = e - row * D;
                const int64_t tn = trials[row * ts_n + d * ts_d];
                var |= tn != trials[d * ts_d] ? 1 : 0;
                uint16_t xo, no;
                binm_pack_one(dtype, x, e, tn, mask ? mask[e] != 0 : true, &xo, &no, &bad);
                xp[e] = xo;
                np[e] = no;
                vmp_pmm_sum_add(&lc, &lce, vmp_binm_lchoose(xo, no));
                hidden += vmp_binm_observed(no) ? 0 : 1;
            }
            v[t] = lc + lce;
        }
        for (int off = VMP_PMM_NT / 2; off > 0; off >>= 1)
            for (int i = 0; i < off; ++i) v[i] += v[i + off];
        vmp_pmm_sum_add(&total, &total_e, v[0]);
    }
    if (bad & VMP_BINM_BAD_NEGATIVE) flags[0] = 1;
    if (bad & VMP_BINM_BAD_FRACTION) flags[1] = 1;
    if (bad & VMP_BINM_BAD_ABOVE) flags[2] = 1;
    if (bad & VMP_BINM_BAD_TRIALS) flags[3] = 1;
    counts[0] = n - hidden;
    counts[1] = hidden;
    counts[2] = var ? 0 : 1;
    lcoef[0] = total + total_e;
}

// ncol and cfold may be null
void binm_tables(int D, int K, int form, const double *elog_p, const double *elog_pi,
                 const double *ncol, double *l1, double *l0, double *c, double *cfold)
{
    for (int i = 0; i < D * K; ++i) {
        const int e0 = i / K * K;
        l1[i] = elog_p ? vmp_binm_table(vmp_binm_l1(elog_p[2 * i], elog_p[2 * i + 1]),
                                        vmp_binm_l1(elog_p[2 * e0], elog_p[2 * e0 + 1]), form)
                       : 0.0;
        l0[i] = elog_p ? vmp_binm_table(elog_p[2 * i + 1], elog_p[2 * e0 + 1], form) : 0.0;
    }
    const bool fold = cfold && ncol;
    double cs[VMP_BINM_MAX_K], fs[VMP_BINM_MAX_K];
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
        if (elog_p && fold)
            for (int d = 0; d < D; ++d)
                t = vmp_pmm_mac(t, ncol[d], vmp_binm_table(elog_p[2 * (d * K + k) + 1],
                                                           elog_p[2 * (d * K) + 1], form));
        cs[k] = elog_pi[k];
        fs[k] = elog_pi[k] + t;
    }
    double m = cs[0], mf = fs[0];
    for (int k = 1; k < K; ++k) {
        m = fmax(m, cs[k]);
        mf = fmax(mf, fs[k]);
    }
    for (int k = 0; k < K; ++k) {
        c[k] = cs[k] - m;
        if (fold) cfold[k] = fs[k] - mf;
    }
}

// two planes: S, T (D x K), Nk (K), counts (D K x 2), scal[0] = sum lse, scal[1] = the rows' parts of
// scal[2] (zero with labels: binm_dots below); r_out (N x K) or null
void binm_pass(int64_t N, int D, int K, const uint16_t *x, const uint16_t *n, const int32_t *labels,
               const double *l1, const double *l0, const double *c, double *S, double *T,
               double *Nk, double *counts, double *scal, double *r_out)
{
    const int KP = vmp_pmm_kpad(K);
    const int64_t chunk = vmp_pmm_chunk_rows(N, D, K), nc = vmp_pmm_chunks(N, D, K);
    const int64_t per = vmp_pmm_partial_doubles(D, K, 1), DK = (int64_t)D * K;
    std::vector<double> part((size_t)(nc * per), 0.0), dots((size_t)nc, 0.0);
    double logit[VMP_BINM_MAX_K], raw[VMP_BINM_MAX_K], ex[VMP_BINM_MAX_K], r[VMP_BINM_MAX_K], v[16];
    for (int64_t ch = 0; ch < nc; ++ch) {
        const int64_t r0 = ch * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
        double *p1 = part.data() + ch * per, *p2 = p1 + DK;             // [k][d]
        std::vector<double> nk(16 * K, 0.0), t1((size_t)DK), t2((size_t)DK);
        double ls[16] = {0}, ds[16] = {0};
        for (int64_t row = r0; row < r1; ++row) {
            if ((row - r0) % VMP_PMM_TILE == 0) {             // a new tile: its sums start at zero
                std::fill(t1.begin(), t1.end(), 0.0);
                std::fill(t2.begin(), t2.end(), 0.0);
            }
            const uint16_t *xr = x + row * D, *nr = n + row * D;
            const int slot = vmp_pmm_slot((int)((row - r0) % VMP_PMM_TILE));
            bool obs = false;
            for (int d = 0; d < D; ++d) obs = obs || vmp_binm_observed(nr[d]);
            double lse = 0.0, rd = 0.0;
            if (labels) {
                for (int k = 0; k < K; ++k) r[k] = k == labels[row] ? 1.0 : 0.0;
            } else {
                for (int k = 0; k < KP; ++k) {
                    double lg = 0.0;
                    if (k < K)
                        for (int d0 = 0; d0 < D; d0 += 4) {   // a step: xt l1, then nt l0
                            const int d1 = d0 + 4 < D ? d0 + 4 : D;
                            for (int d = d0; d < d1; ++d)
                                lg = vmp_pmm_mac(lg, vmp_binm_count(xr[d], nr[d]), l1[d * K + k]);
                            for (int d = d0; d < d1; ++d)
                                lg = vmp_pmm_mac(lg, vmp_binm_trials(nr[d]), l0[d * K + k]);
                        }
                    raw[k] = lg;
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
                for (int j = 0; j < 16; ++j) {                // r . (logit - c), lane by lane
                    double s = 0.0;
                    for (int k = j; k < KP; k += 16)
                        s = vmp_pmm_mac(s, k < K ? r[k] : 0.0, raw[k]);
                    v[j] = s;
                }
                vmp_dgmm_group_sum_host(v);
                rd = v[0];
            }
            if (r_out)
                for (int k = 0; k < K; ++k) r_out[row * K + k] = r[k];
            if (obs) {
                ls[slot] += lse;
                ds[slot] += rd;
            }
            for (int k = 0; k < K; ++k) {
                if (obs) nk[slot * K + k] += r[k];
                for (int d = 0; d < D; ++d) {
                    t1[k * D + d] = vmp_pmm_mac(t1[k * D + d], r[k], vmp_binm_count(xr[d], nr[d]));
                    t2[k * D + d] = vmp_pmm_mac(t2[k * D + d], r[k], vmp_binm_trials(nr[d]));
                }
            }
            if ((row - r0) % VMP_PMM_TILE == VMP_PMM_TILE - 1 || row == r1 - 1)
                for (int64_t i = 0; i < DK; ++i) {            // the tile's sums, in tile order
                    p1[i] += t1[i];
                    p2[i] += t2[i];
                }
        }
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int s = 0; s < 16; ++s) t += nk[s * K + k];
            p1[2 * DK + k] = t;
        }
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += ls[s];
        p1[2 * DK + K] = t;
        double u = 0.0;
        for (int s = 0; s < 16; ++s) u += ds[s];
        dots[(size_t)ch] = u;
    }
    for (int k = 0; k < K; ++k) {
        double nn = 0.0;
        for (int64_t ch = 0; ch < nc; ++ch) nn += part[ch * per + 2 * DK + k];
        Nk[k] = nn;
        for (int d = 0; d < D; ++d) {
            double s = 0.0, t = 0.0;
            for (int64_t ch = 0; ch < nc; ++ch) {
                s += part[ch * per + k * D + d];
                t += part[ch * per + DK + k * D + d];
            }
            S[d * K + k] = s;
            T[d * K + k] = t;
            counts[2 * (d * K + k)] = s;
            counts[2 * (d * K + k) + 1] = vmp_binm_failures(t, s);
        }
    }
    double t = 0.0;
    for (int64_t ch = 0; ch < nc; ++ch) t += part[ch * per + 2 * DK + K];
    scal[0] = t;
    double u = 0.0;
    for (int64_t ch = 0; ch < nc; ++ch) u += dots[(size_t)ch];
    scal[1] = u;
}

// one plane: T and counts from the S and N_k of the Poisson pass
void binm_const(int D, int K, const double *ncol, const double *S, const double *Nk, double *T,
                double *counts)
{
    for (int e = 0; e < D * K; ++e) {
        const double t = vmp_binm_t_const(ncol[e / K], Nk[e % K]);
        T[e] = t;
        counts[2 * e] = S[e];
        counts[2 * e + 1] = vmp_binm_failures(t, S[e]);
    }
}

// scal[2] of the two-plane form under fixed labels: the 256 threads' sums halved eight times
double binm_dots(int n, const double *S, const double *l1, const double *T, const double *l0)
{
    double v[VMP_PMM_NT];
    for (int tid = 0; tid < VMP_PMM_NT; ++tid) {
        double t = 0.0, te = 0.0;
        for (int e = tid; e < n; e += VMP_PMM_NT) {
            double err;
            const double x = vmp_binm_dot_term(S[e], l1[e], T[e], l0[e], &err);
            vmp_pmm_sum_add(&t, &te, x);
            te += err;
        }
        v[tid] = t + te;
    }
    for (int off = VMP_PMM_NT / 2; off > 0; off >>= 1)
        for (int i = 0; i < off; ++i) v[i] += v[i + off];
    return v[0];
}

}  // extern "C"
