// TEST DOUBLE: the plate pass of csrc/vmp_bmm.hip on the host, built with g++ from the very header
// the kernels include (csrc/vmp_bmm_dev.h).  Chunks are walked one after the other, a chunk's rows
// in tiles of 64, the KP logits of a row as the columns of a 16-lane group reduced by the header's
// butterfly, N_k and sum lse per slot -- the order of every addition is the one the header states.
#include <math.h>
#include <stdint.h>
#include <vector>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_bmm_dev.h"

extern "C" {

int bmm_kpad(int K) { return vmp_bmm_kpad(K); }
int bmm_words(int D) { return vmp_bmm_words(D); }
int64_t bmm_chunk_rows(int64_t N, int D, int K) { return vmp_bmm_chunk_rows(N, D, K); }
int64_t bmm_chunks(int64_t N, int D, int K) { return vmp_bmm_chunks(N, D, K); }
int64_t bmm_partial_doubles(int D, int K) { return vmp_bmm_partial_doubles(D, K); }

// dtype 0 = float64, 1 = int64, 2 = bool / uint8; returns the flag
int bmm_pack(int64_t N, int D, int dtype, const void *x, uint64_t *xw)
{
    const int W = vmp_bmm_words(D);
    int flag = 0;
    for (int64_t n = 0; n < N; ++n)
        for (int wd = 0; wd < W; ++wd) {
            uint64_t bits = 0;
            for (int d = wd * 64; d < D && d < wd * 64 + 64; ++d) {
                const int64_t e = n * D + d;
                double v = dtype == 0 ? ((const double *)x)[e]
                         : dtype == 1 ? (double)((const int64_t *)x)[e]
                                      : (double)((const uint8_t *)x)[e];
                if (v == 1.0) bits |= (uint64_t)1 << (d - wd * 64);
                else if (!(v == 0.0)) flag = 1;
            }
            xw[n * W + wd] = bits;
        }
    return flag;
}

void bmm_unpack(int64_t N, int D, const uint64_t *xw, double *x)
{
    const int W = vmp_bmm_words(D);
    for (int64_t n = 0; n < N; ++n)
        for (int d = 0; d < D; ++d) x[n * D + d] = vmp_bmm_bit(xw + n * W, d);
}

void bmm_tables(int D, int K, const double *elog_p, const double *elog_pi, double *w, double *c)
{
    for (int i = 0; i < D * K; ++i) w[i] = elog_p ? elog_p[2 * i] - elog_p[2 * i + 1] : 0.0;
    double m = -INFINITY;
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
        if (elog_p)
            for (int d = 0; d < D; ++d) t += elog_p[2 * (d * K + k) + 1];
        c[k] = t + elog_pi[k];
        m = fmax(m, c[k]);
    }
    for (int k = 0; k < K; ++k) c[k] -= m;
}

// S (D x K), Nk (K), counts (D K x 2), scal[0] = sum lse; r_out (N x K) or null
void bmm_pass(int64_t N, int D, int K, const uint64_t *xw, const int32_t *labels, const double *w,
              const double *c, double *S, double *Nk, double *counts, double *scal, double *r_out)
{
    const int KP = vmp_bmm_kpad(K), W = vmp_bmm_words(D);
    const int64_t chunk = vmp_bmm_chunk_rows(N, D, K), nc = vmp_bmm_chunks(N, D, K);
    const int64_t per = vmp_bmm_partial_doubles(D, K);
    std::vector<double> part((size_t)(nc * per), 0.0);
    double logit[VMP_BMM_MAX_K], r[VMP_BMM_MAX_K], v[16];
    for (int64_t ch = 0; ch < nc; ++ch) {
        const int64_t r0 = ch * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
        double *pS = part.data() + ch * per;              // [k][d]
        std::vector<double> nk(16 * K, 0.0);
        double ls[16] = {0};
        for (int64_t row = r0; row < r1; ++row) {
            const uint64_t *xr = xw + row * W;
            const int slot = vmp_bmm_slot((int)((row - r0) % VMP_BMM_TILE));
            double lse = 0.0;
            if (labels) {
                for (int k = 0; k < K; ++k) r[k] = k == labels[row] ? 1.0 : 0.0;
            } else {
                for (int k = 0; k < KP; ++k) {
                    double l = 0.0;
                    if (k < K)
                        for (int d = 0; d < D; ++d)
                            l = vmp_bmm_logit_step(l, vmp_bmm_bit(xr, d), w[d * K + k]);
                    logit[k] = vmp_bmm_logit_finish(l, k < K ? c[k] : -INFINITY);
                }
                double m = logit[0];
                for (int k = 1; k < KP; ++k) m = fmax(m, logit[k]);
                for (int j = 0; j < 16; ++j) {
                    double s = 0.0;
                    for (int k = j; k < KP; k += 16) s += vmp_bmm_shifted_exp(logit[k], m);
                    v[j] = s;
                }
                vmp_bmm_group_sum_host(v);
                lse = vmp_bmm_lse(m, v[0]);
                for (int k = 0; k < K; ++k) r[k] = vmp_bmm_resp(logit[k], lse);
            }
            ls[slot] += lse;
            for (int k = 0; k < K; ++k) {
                nk[slot * K + k] += r[k];
                if (r_out) r_out[row * K + k] = r[k];
                for (int d = 0; d < D; ++d) pS[k * D + d] += r[k] * vmp_bmm_bit(xr, d);
            }
        }
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int s = 0; s < 16; ++s) t += nk[s * K + k];
            pS[D * K + k] = t;
        }
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += ls[s];
        pS[D * K + K] = t;
    }
    for (int k = 0; k < K; ++k)
        for (int d = 0; d < D; ++d) {
            double s = 0.0, n = 0.0;
            for (int64_t ch = 0; ch < nc; ++ch) {
                s += part[ch * per + k * D + d];
                n += part[ch * per + D * K + k];
            }
            const int e = d * K + k;
            S[e] = s;
            counts[2 * e] = s;
            counts[2 * e + 1] = n - s;
            if (d == 0) Nk[k] = n;
        }
    double t = 0.0;
    for (int64_t ch = 0; ch < nc; ++ch) t += part[ch * per + D * K + K];
    scal[0] = t;
}

}  // extern "C"
