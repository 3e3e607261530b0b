// TEST DOUBLE: the plate pass of csrc/vmp_cmm.hip on the host, built with g++ from the very header
// the kernels include (csrc/vmp_cmm_dev.h).  Chunks are walked one after the other, a chunk's rows
// in tiles of 64, the KP logits of a row as the lanes of a lane group reduced by the header's
// butterfly, N_k and sum lse per group (row t of a tile: group t % NG) in row order, every cell of
// the count table -- kept in the kernel's LDS layout (vmp_cmm_cell) -- in ascending row order
// through the chunk, and the chunks' partials in chunk order: the order of every addition is the
// one the header states.
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_cmm_dev.h"

extern "C" {

int cmm_kpad(int K) { return vmp_cmm_kpad(K); }
int cmm_max_k() { return VMP_CMM_MAX_K; }
int cmm_min_m() { return VMP_CMM_MIN_M; }
int cmm_max_m() { return VMP_CMM_MAX_M; }
int cmm_max_cells() { return VMP_CMM_MAX_CELLS; }
int cmm_supported(int D, int K, int M) { return vmp_cmm_supported(D, K, M) ? 1 : 0; }
int64_t cmm_cells(int D, int K, int M) { return vmp_cmm_cells(D, K, M); }
int64_t cmm_lds_bytes(int D, int K, int M) { return vmp_cmm_lds_bytes(D, K, M); }
int64_t cmm_chunk_rows(int64_t N, int D, int K, int M) { return vmp_cmm_chunk_rows(N, D, K, M); }
int64_t cmm_chunks(int64_t N, int D, int K, int M) { return vmp_cmm_chunks(N, D, K, M); }
int64_t cmm_partial_doubles(int D, int K, int M) { return vmp_cmm_partial_doubles(D, K, M); }

// dtype 0 = float64, 1 = int64, 2 = uint8, 3 = int32; mask: N x D uint8 or null; xb: N x D bytes;
// returns the flag
int cmm_pack(int64_t N, int D, int M, int dtype, const void *x, const uint8_t *mask, uint8_t *xb)
{
    bool bad = false;
    for (int64_t e = 0; e < N * D; ++e) {
        const bool seen = mask ? mask[e] != 0 : true;
        if (dtype == 0) xb[e] = vmp_cmm_byte_f64(((const double *)x)[e], seen, M, &bad);
        else if (dtype == 1) xb[e] = vmp_cmm_byte_i64(((const int64_t *)x)[e], seen, M, &bad);
        else if (dtype == 2) xb[e] = vmp_cmm_byte_i64(((const uint8_t *)x)[e], seen, M, &bad);
        else xb[e] = vmp_cmm_byte_i64(((const int32_t *)x)[e], seen, M, &bad);
    }
    return bad ? 1 : 0;
}

void cmm_tables(int D, int K, int M, const double *elog_p, const double *elog_pi, double *L,
                double *c)
{
    for (int64_t i = 0; i < (int64_t)M * D * K; ++i) L[i] = elog_p ? elog_p[i] : 0.0;
    double m = elog_pi[0];
    for (int k = 1; k < K; ++k) m = fmax(m, elog_pi[k]);
    for (int k = 0; k < K; ++k) c[k] = elog_pi[k] - m;
}

// S (M x D x K), Nk (K), scal[0] = sum lse; r_out (N x K) or null
void cmm_pass(int64_t N, int D, int K, int M, const uint8_t *xb, const int32_t *labels,
              const double *L, const double *c, double *S, double *Nk, double *scal, double *r_out)
{
    const int KP = vmp_cmm_kpad(K), NG = vmp_cmm_groups(K);
    const int64_t chunk = vmp_cmm_chunk_rows(N, D, K, M), nc = vmp_cmm_chunks(N, D, K, M);
    const int64_t per = vmp_cmm_partial_doubles(D, K, M), MDK = (int64_t)M * D * K;
    std::vector<double> part((size_t)(nc * per), 0.0);
    double logit[64], r[64], v[64];
    for (int64_t ch = 0; ch < nc; ++ch) {
        const int64_t r0 = ch * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
        std::vector<double> cnt((size_t)vmp_cmm_cells(D, K, M), 0.0), nk((size_t)NG * KP, 0.0);
        double ls[16] = {0};
        for (int64_t row = r0; row < r1; ++row) {
            const uint8_t *xr = xb + row * D;
            const int gid = (int)((row - r0) % VMP_CMM_TILE) % NG;
            bool any = false;
            for (int d = 0; d < D; ++d) any = any || vmp_cmm_observed(xr[d], M);
            double lse = 0.0;
            if (labels) {
                for (int k = 0; k < KP; ++k) r[k] = k == labels[row] ? 1.0 : 0.0;
            } else {
                for (int k = 0; k < KP; ++k) {
                    double l = 0.0;
                    if (k < K)
                        for (int d = 0; d < D; ++d)
                            if (vmp_cmm_observed(xr[d], M))
                                l = vmp_cmm_logit_step(l, L[((int64_t)xr[d] * D + d) * K + k]);
                    logit[k] = vmp_cmm_logit_finish(l, k < K ? c[k] : -INFINITY);
                }
                double m = logit[0];
                for (int k = 1; k < KP; ++k) m = fmax(m, logit[k]);
                for (int k = 0; k < KP; ++k) v[k] = vmp_cmm_shifted_exp(logit[k], m);
                vmp_cmm_group_sum_host(v, KP);
                lse = vmp_cmm_lse(m, v[0]);
                for (int k = 0; k < KP; ++k) r[k] = vmp_cmm_resp(logit[k], lse);
            }
            if (r_out)
                for (int k = 0; k < K; ++k) r_out[row * K + k] = r[k];
            if (!any) continue;                               // adds exactly nothing
            ls[gid] += lse;
            for (int k = 0; k < KP; ++k) nk[(size_t)gid * KP + k] += r[k];
            for (int d = 0; d < D; ++d)
                if (vmp_cmm_observed(xr[d], M))
                    for (int k = 0; k < KP; ++k) cnt[vmp_cmm_cell(d, xr[d], k, M, KP)] += r[k];
        }
        double *p = part.data() + ch * per;
        for (int64_t e = 0; e < MDK; ++e) {
            const int kk = (int)(e % K), md = (int)(e / K), d = md % D, m = md / D;
            p[e] = cnt[vmp_cmm_cell(d, m, kk, M, KP)];
        }
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int s = 0; s < NG; ++s) t += nk[(size_t)s * KP + k];
            p[MDK + k] = t;
        }
        double t = 0.0;
        for (int s = 0; s < NG; ++s) t += ls[s];
        p[MDK + K] = t;
    }
    for (int64_t e = 0; e < per; ++e) {
        double t = 0.0;
        for (int64_t ch = 0; ch < nc; ++ch) t += part[ch * per + e];
        if (e < MDK) S[e] = t;
        else if (e < MDK + K) Nk[e - MDK] = t;
        else scal[0] = t;
    }
}

}  // extern "C"
