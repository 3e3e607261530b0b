// TEST DOUBLE: the pack, the tables and the plate pass of csrc/vmp_mmm.hip on the host, built with
// g++ from the very header the kernels include (csrc/vmp_mmm_dev.h); the special functions of
// vmp_common.h come in ahead of this file (host_build.special_functions_text).  Chunks are walked
// one after the other, a chunk's rows in tiles of 64, the logit in steps of 4 words, the softmax,
// the slots and the two levels of the statistics as in tests/host/pmm_host.cpp -- the order of
// every addition is the one the header states.
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_mmm_dev.h"

extern "C" {

int mmm_max_k() { return VMP_MMM_MAX_K; }
int mmm_max_m() { return VMP_MMM_MAX_M; }
int mmm_max_count() { return VMP_MMM_MAX_COUNT; }
int mmm_mblock() { return VMP_MMM_MBLOCK; }
int64_t mmm_chunk_rows(int64_t N, int M, int K) { return vmp_mmm_chunk_rows(N, M, K); }
int64_t mmm_chunks(int64_t N, int M, int K) { return vmp_mmm_chunks(N, M, K); }
int64_t mmm_workspace_doubles(int64_t N, int M, int K) { return vmp_mmm_workspace_doubles(N, M, K); }

static uint16_t pack_one(int dtype, const void *x, int64_t e, int *bad)
{
    switch (dtype) {
    case 0: return vmp_mmm_entry(vmp_pmm_pack_f64(((const double *)x)[e], true, bad));
    case 1: return vmp_mmm_entry(vmp_pmm_pack_i64(((const int64_t *)x)[e], true, bad));
    case 2: return vmp_mmm_entry(vmp_pmm_pack_i64((int64_t)((const uint8_t *)x)[e], true, bad));
    default: return vmp_mmm_entry(vmp_pmm_pack_i64((int64_t)((const int32_t *)x)[e], true, bad));
    }
}

// xp (N x M), flags (4), lcoef (1)
void mmm_pack(int64_t N, int M, int dtype, const void *x, const int64_t *trials, uint16_t *xp,
              int32_t *flags, double *lcoef)
{
    const int64_t span = vmp_pmm_pack_span(N), nb = N > 0 ? vmp_pmm_pack_blocks(N) : 0;
    double total = 0.0, total_e = 0.0;
    int bad = 0;
    for (int64_t b = 0; b < nb; ++b) {
        double v[VMP_MMM_NT];
        for (int t = 0; t < VMP_MMM_NT; ++t) {
            double lg = 0.0, lge = 0.0;
            for (int64_t i = t; i < span; i += VMP_MMM_NT) {
                const int64_t row = b * span + i;
                if (row >= N) break;
                int bad_row = 0;
                int64_t sum = 0;
                vmp_pmm_sum_add(&lg, &lge, vmp_mmm_lgamma1_trials(trials[row]));
                for (int m = 0; m < M; ++m) {
                    const uint16_t p = pack_one(dtype, x, row * M + m, &bad_row);
                    xp[row * M + m] = p;
                    sum += p;
                    vmp_pmm_sum_add(&lg, &lge, -vmp_pmm_lgamma1(p));
                }
                if (vmp_mmm_sum_mismatch(sum, trials[row], bad_row)) bad_row |= VMP_MMM_BAD_SUM;
                bad |= bad_row;
            }
            v[t] = lg + lge;
        }
        for (int off = VMP_MMM_NT / 2; off > 0; off >>= 1)
            for (int i = 0; i < off; ++i) v[i] += v[i + off];
        vmp_pmm_sum_add(&total, &total_e, v[0]);
    }
    if (bad & VMP_PMM_BAD_INVALID) flags[0] = 1;
    if (bad & VMP_PMM_BAD_ABOVE) flags[1] = 1;
    if (bad & VMP_PMM_BAD_FRACTION) flags[2] = 1;
    if (bad & VMP_MMM_BAD_SUM) flags[3] = 1;
    lcoef[0] = total + total_e;
}

// L (M x K) from elog_p (K x M) or null, c (K)
void mmm_tables(int M, int K, const double *elog_p, const double *elog_pi, double *L, double *c)
{
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < K; ++k)
            L[m * K + k] = elog_p ? vmp_mmm_table(elog_p[k * M + m], elog_p[m]) : 0.0;
    double mx = elog_pi[0];
    for (int k = 1; k < K; ++k) mx = fmax(mx, elog_pi[k]);
    for (int k = 0; k < K; ++k) c[k] = elog_pi[k] - mx;
}

// S (K x M), Nk (K), scal[0] = sum lse, scal[1] = Nk . c, scal[2] = S . L; r_out (N x K) or null
void mmm_pass(int64_t N, int M, int K, const uint16_t *x, const int32_t *labels, const double *L,
              const double *c, double *S, double *Nk, double *scal, double *r_out)
{
    const int KP = vmp_pmm_kpad(K);
    const int64_t chunk = vmp_mmm_chunk_rows(N, M, K), nc = vmp_mmm_chunks(N, M, K);
    const int64_t per = vmp_mmm_partial_doubles(M, K), MK = (int64_t)M * K;
    std::vector<double> part((size_t)(nc * per), 0.0);
    double logit[VMP_MMM_MAX_K], ex[VMP_MMM_MAX_K], r[VMP_MMM_MAX_K], v[16];
    for (int64_t ch = 0; ch < nc; ++ch) {
        const int64_t r0 = ch * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
        double *p1 = part.data() + ch * per;                            // [k][m]
        std::vector<double> nk(16 * K, 0.0), t1((size_t)MK);
        double ls[16] = {0};
        for (int64_t row = r0; row < r1; ++row) {
            if ((row - r0) % VMP_MMM_TILE == 0) std::fill(t1.begin(), t1.end(), 0.0);
            const uint16_t *xr = x + row * M;
            const int slot = vmp_pmm_slot((int)((row - r0) % VMP_MMM_TILE));
            double lse = 0.0;
            if (labels) {
                for (int k = 0; k < K; ++k) r[k] = k == labels[row] ? 1.0 : 0.0;
            } else {
                for (int k = 0; k < KP; ++k) {
                    double lg = 0.0;
                    if (k < K)
                        for (int m = 0; m < M; ++m)
                            lg = vmp_pmm_mac(lg, vmp_pmm_count(xr[m]), L[m * K + k]);
                    logit[k] = vmp_dgmm_logit_finish(lg, k < K ? c[k] : -INFINITY);
                }
                double mx = logit[0];
                for (int k = 1; k < KP; ++k) mx = fmax(mx, logit[k]);
                for (int j = 0; j < 16; ++j) {
                    double s = 0.0;
                    for (int k = j; k < KP; k += 16) {
                        ex[k] = vmp_dgmm_shifted_exp(logit[k], mx);
                        s += ex[k];
                    }
                    v[j] = s;
                }
                vmp_dgmm_group_sum_host(v);
                lse = vmp_dgmm_lse(mx, v[0]);
                for (int k = 0; k < K; ++k) r[k] = vmp_pmm_resp(ex[k], v[0]);
            }
            if (r_out)
                for (int k = 0; k < K; ++k) r_out[row * K + k] = r[k];
            ls[slot] += lse;
            for (int k = 0; k < K; ++k) {
                nk[slot * K + k] += r[k];
                for (int m = 0; m < M; ++m)
                    t1[k * M + m] = vmp_pmm_mac(t1[k * M + m], r[k], vmp_pmm_count(xr[m]));
            }
            if ((row - r0) % VMP_MMM_TILE == VMP_MMM_TILE - 1 || row == r1 - 1)
                for (int64_t i = 0; i < MK; ++i) p1[i] += t1[i];    // the tile's sums, in tile order
        }
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int s = 0; s < 16; ++s) t += nk[s * K + k];
            p1[MK + k] = t;
        }
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += ls[s];
        p1[MK + K] = t;
    }
    for (int64_t i = 0; i < MK; ++i) {
        double s = 0.0;
        for (int64_t ch = 0; ch < nc; ++ch) s += part[ch * per + i];
        S[i] = s;
    }
    for (int k = 0; k < K; ++k) {
        double n = 0.0;
        for (int64_t ch = 0; ch < nc; ++ch) n += part[ch * per + MK + k];
        Nk[k] = n;
    }
    double t = 0.0;
    for (int64_t ch = 0; ch < nc; ++ch) t += part[ch * per + MK + K];
    scal[0] = t;
    double n = 0.0;
    for (int k = 0; k < K; ++k) n = vmp_pmm_mac(n, Nk[k], c[k]);
    scal[1] = n;
    double d[VMP_MMM_NT];
    for (int tid = 0; tid < VMP_MMM_NT; ++tid) {
        double a = 0.0;
        for (int64_t e = tid; e < MK; e += VMP_MMM_NT)
            a = vmp_pmm_mac(a, S[e], L[(e % M) * K + e / M]);
        d[tid] = a;
    }
    for (int off = VMP_MMM_NT / 2; off > 0; off >>= 1)
        for (int i = 0; i < off; ++i) d[i] += d[i + off];
    scal[2] = d[0];
}

}  // extern "C"
