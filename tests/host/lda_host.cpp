// TEST DOUBLE: the token pass of csrc/vmp_lda.hip on the host, built with g++ from the very header
// the kernels include (csrc/vmp_lda_dev.h).  One call is one pass (document order or word order)
// plus its combine step: chunks are walked one after the other, a chunk's tokens in order, the K
// logits of a token as an array of G values reduced by the header's butterflies -- the order of
// every addition is the kernel's.
#include <math.h>
#include <stdint.h>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_lda_dev.h"

extern "C" {

int lda_group(int K) { return vmp_lda_group(K); }
int lda_chunk_tokens(int64_t n, int K) { return vmp_lda_chunk_tokens(n, K); }

// pos == NULL: pass A (lse written, chunk_lse summed); else pass B (lse read through pos)
void lda_pass(int64_t n, int64_t nseg, int K, const int32_t *seg, const int32_t *oth,
              const int64_t *seg_off, const int32_t *pos, const int32_t *labels, const double *Tseg,
              const double *Toth, double *lse, double *N, double *head, double *tail,
              double *chunk_lse, const int32_t *orig, double *phi)
{
    const int G = vmp_lda_group(K);
    const int T = vmp_lda_chunk_tokens(n, K);
    const int64_t nc = n > 0 ? (n + T - 1) / T : 0;
    double acc[64], logit[64], v[64];
    for (int64_t c = 0; c < nc; ++c) {
        const int64_t cs = c * T, ce = cs + T < n ? cs + T : n;
        int cur = seg[cs];
        bool inside = seg_off[cur] >= cs;
        double lsum = 0.0;
        for (int k = 0; k < K; ++k) acc[k] = 0.0;
        for (int64_t i = cs; i < ce; ++i) {
            const int s = seg[i], o = oth[i];
            if (s != cur) {
                double *dst = inside ? N + (int64_t)cur * K : head + c * K;
                for (int k = 0; k < K; ++k) { dst[k] = acc[k]; acc[k] = 0.0; }
                cur = s;
                inside = true;
            }
            const int64_t li = pos ? pos[i] : i;
            for (int k = 0; k < K; ++k) {
                double p;
                if (labels) {
                    p = (k == labels[li]) ? 1.0 : 0.0;
                } else {
                    if (k == 0) {
                        for (int j = 0; j < G; ++j)
                            logit[j] = j < K ? vmp_lda_logit(Tseg ? Tseg[(int64_t)s * K + j] : 0.0,
                                                             Toth ? Toth[(int64_t)o * K + j] : 0.0)
                                             : -INFINITY;
                        if (!pos) {
                            for (int j = 0; j < G; ++j) v[j] = logit[j];
                            vmp_lda_group_max_host(v, G);
                            const double m = v[0];
                            for (int j = 0; j < G; ++j)
                                v[j] = j < K ? vmp_lda_shifted_exp(logit[j], m) : 0.0;
                            vmp_lda_group_sum_host(v, G);
                            lse[i] = vmp_lda_lse(m, v[0]);
                            lsum += lse[i];
                        }
                    }
                    p = vmp_lda_phi(logit[k], lse[li]);
                }
                acc[k] += p;
                if (phi) phi[(int64_t)orig[i] * K + k] = p;
            }
            if (labels && !pos) lse[i] = 0.0;
        }
        const bool ends = seg_off[cur + 1] <= ce;
        double *dst = (inside && ends) ? N + (int64_t)cur * K : (!inside ? head + c * K : tail + c * K);
        for (int k = 0; k < K; ++k) dst[k] = acc[k];
        if (!pos) chunk_lse[c] = lsum;
    }
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t b = seg_off[s], e = seg_off[s + 1];
        if (b == e) {
            for (int k = 0; k < K; ++k) N[s * K + k] = 0.0;
            continue;
        }
        const int64_t c0 = b / T, c1 = (e - 1) / T;
        if (c0 == c1) continue;
        for (int k = 0; k < K; ++k) {
            double sum = tail[c0 * K + k];
            for (int64_t c = c0 + 1; c < c1; ++c) sum += head[c * K + k];
            N[s * K + k] = sum + head[c1 * K + k];
        }
    }
}

}  // extern "C"
