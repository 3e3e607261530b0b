// TEST DOUBLE: the masked plate pass of csrc/vmp_bmm.hip on the host, built with g++ from the very
// header the kernels include (csrc/vmp_bmm_dev.h).  A row is two bit planes (x & m, then m).
// Chunks are walked one after the other, a chunk's rows in tiles of 64, the logit over plane 0 and
// then over plane 1, the KP logits of a row as the columns of a 16-lane group reduced by the
// header's butterfly, N_k and sum lse per slot over the observed rows, S and M per tile from zero
// and the tiles' sums in tile order -- the order of every addition is the one the header states.
#include <math.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_bmm_dev.h"

extern "C" {

int bmmm_words(int D) { return vmp_bmm_words(D); }
int bmmm_max_k() { return VMP_BMM_MASKED_MAX_K; }
int bmmm_max_d() { return VMP_BMM_MASKED_MAX_D; }
int64_t bmmm_chunk_rows(int64_t N, int D, int K) { return vmp_bmm_chunk_rows_masked(N, D, K); }
int64_t bmmm_chunks(int64_t N, int D, int K) { return vmp_bmm_chunks_masked(N, D, K); }
int64_t bmmm_partial_doubles(int D, int K) { return vmp_bmm_partial_doubles_masked(D, K); }

// dtype 0 = float64, 1 = int64, 2 = bool / uint8; mask: N x D uint8; xw: N x 2 W; returns the flag.
// A hidden value is never read.
int bmmm_pack(int64_t N, int D, int dtype, const void *x, const uint8_t *mask, uint64_t *xw)
{
    const int W = vmp_bmm_words(D);
    int flag = 0;
    for (int64_t n = 0; n < N; ++n)
        for (int wd = 0; wd < W; ++wd) {
            uint64_t bits = 0, mbits = 0;
            for (int d = wd * 64; d < D && d < wd * 64 + 64; ++d) {
                const int64_t e = n * D + d;
                if (!mask[e]) continue;
                mbits |= (uint64_t)1 << (d - wd * 64);
                double v = dtype == 0 ? ((const double *)x)[e]
                         : dtype == 1 ? (double)((const int64_t *)x)[e]
                                      : (double)((const uint8_t *)x)[e];
                if (v == 1.0) bits |= (uint64_t)1 << (d - wd * 64);
                else if (!(v == 0.0)) flag = 1;
            }
            xw[n * 2 * W + wd] = bits;
            xw[n * 2 * W + W + wd] = mbits;
        }
    return flag;
}

void bmmm_tables(int D, int K, const double *elog_p, const double *elog_pi, double *w, double *l0,
                 double *c)
{
    for (int i = 0; i < D * K; ++i) {
        w[i] = elog_p ? elog_p[2 * i] - elog_p[2 * i + 1] : 0.0;
        l0[i] = elog_p ? elog_p[2 * i + 1] : 0.0;
    }
    double m = elog_pi[0];
    for (int k = 1; k < K; ++k) m = fmax(m, elog_pi[k]);
    for (int k = 0; k < K; ++k) c[k] = elog_pi[k] - m;
}

// S, M (D x K), Nk (K), counts (D K x 2), scal[0] = sum lse; r_out (N x K) or null
void bmmm_pass(int64_t N, int D, int K, const uint64_t *xw, const int32_t *labels, const double *w,
               const double *l0, const double *c, double *S, double *M, double *Nk, double *counts,
               double *scal, double *r_out)
{
    const int KP = vmp_bmm_kpad(K), W = vmp_bmm_words(D);
    const int64_t chunk = vmp_bmm_chunk_rows_masked(N, D, K), nc = vmp_bmm_chunks_masked(N, D, K);
    const int64_t per = vmp_bmm_partial_doubles_masked(D, K), DK = (int64_t)D * K;
    std::vector<double> part((size_t)(nc * per), 0.0);
    double logit[VMP_BMM_MASKED_MAX_K], r[VMP_BMM_MASKED_MAX_K], v[16];
    for (int64_t ch = 0; ch < nc; ++ch) {
        const int64_t r0 = ch * chunk, r1 = r0 + chunk < N ? r0 + chunk : N;
        double *pS = part.data() + ch * per, *pM = pS + DK;   // [k][d]
        std::vector<double> nk(16 * K, 0.0), tS((size_t)DK), tM((size_t)DK);
        double ls[16] = {0};
        for (int64_t row = r0; row < r1; ++row) {
            if ((row - r0) % VMP_BMM_TILE == 0) {             // a new tile: its sums start at zero
                std::fill(tS.begin(), tS.end(), 0.0);
                std::fill(tM.begin(), tM.end(), 0.0);
            }
            const uint64_t *xr = xw + row * 2 * W, *mr = xr + W;
            const int slot = vmp_bmm_slot((int)((row - r0) % VMP_BMM_TILE));
            double lse = 0.0;
            if (labels) {
                for (int k = 0; k < K; ++k) r[k] = k == labels[row] ? 1.0 : 0.0;
            } else {
                for (int k = 0; k < KP; ++k) {
                    double l = 0.0;
                    if (k < K) {
                        for (int d = 0; d < D; ++d)
                            l = vmp_bmm_logit_step(l, vmp_bmm_bit(xr, d), w[d * K + k]);
                        for (int d = 0; d < D; ++d)
                            l = vmp_bmm_logit_step(l, vmp_bmm_bit(mr, d), l0[d * K + k]);
                    }
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
            if (r_out)
                for (int k = 0; k < K; ++k) r_out[row * K + k] = r[k];
            if (vmp_bmm_row_observed(mr, W)) {                // else: adds exactly nothing
                ls[slot] += lse;
                for (int k = 0; k < K; ++k) {
                    nk[slot * K + k] += r[k];
                    for (int d = 0; d < D; ++d) {
                        tS[k * D + d] += r[k] * vmp_bmm_bit(xr, d);
                        tM[k * D + d] += r[k] * vmp_bmm_bit(mr, d);
                    }
                }
            }
            if ((row - r0) % VMP_BMM_TILE == VMP_BMM_TILE - 1 || row == r1 - 1)
                for (int64_t i = 0; i < DK; ++i) {            // the tile's sums, in tile order
                    pS[i] += tS[i];
                    pM[i] += tM[i];
                }
        }
        for (int k = 0; k < K; ++k) {
            double t = 0.0;
            for (int s = 0; s < 16; ++s) t += nk[s * K + k];
            pS[2 * DK + k] = t;
        }
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += ls[s];
        pS[2 * DK + K] = t;
    }
    for (int k = 0; k < K; ++k) {
        double n = 0.0;
        for (int64_t ch = 0; ch < nc; ++ch) n += part[ch * per + 2 * DK + k];
        Nk[k] = n;
        for (int d = 0; d < D; ++d) {
            double s = 0.0, m = 0.0;
            for (int64_t ch = 0; ch < nc; ++ch) {
                s += part[ch * per + k * D + d];
                m += part[ch * per + DK + k * D + d];
            }
            const int e = d * K + k;
            S[e] = s;
            M[e] = m;
            counts[2 * e] = s;
            counts[2 * e + 1] = m - s;
        }
    }
    double t = 0.0;
    for (int64_t ch = 0; ch < nc; ++ch) t += part[ch * per + 2 * DK + K];
    scal[0] = t;
}

}  // extern "C"
