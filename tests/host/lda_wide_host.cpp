// TEST DOUBLE: the wide-topic token pass of csrc/vmp_lda_wide.hip on the host, built with g++ from
// the very headers the kernels include (csrc/vmp_lda_wide_dev.h, which includes vmp_lda_dev.h).  One
// call is one pass (document order or word order) plus its combine step: chunks are walked one after
// the other, a chunk's tokens in order; the 64 R logits of a token are reduced in the header's order
// (in lane over r ascending, then the 64-lane butterfly) -- the order of every addition is the
// kernel's.  The kernel keeps the segment's row in registers and asks for the next token's gathered
// row early; neither changes a bit, so neither is restated here.
#include <math.h>
#include <stdint.h>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_lda_wide_dev.h"

extern "C" {

int lda_wide_regs(int K) { return vmp_lda_wide_regs(K); }
int lda_wide_chunk_tokens(int64_t n) { return vmp_lda_wide_chunk_tokens(n); }

// pos == NULL: pass A (lse written, chunk_lse summed); else pass B (lse read through pos)
void lda_wide_pass(int64_t n, int64_t nseg, int K, const int32_t *seg, const int32_t *oth,
                   const int64_t *seg_off, const int32_t *pos, const int32_t *labels,
                   const double *Tseg, const double *Toth, double *lse, double *N, double *head,
                   double *tail, double *chunk_lse, const int32_t *orig, double *phi)
{
    const int R = vmp_lda_wide_regs(K);
    const int W = VMP_LDA_WIDE_LANES * R;
    const int T = vmp_lda_wide_chunk_tokens(n);
    const int64_t nc = n > 0 ? (n + T - 1) / T : 0;
    double acc[VMP_LDA_WIDE_MAX_K], logit[VMP_LDA_WIDE_MAX_K], e[VMP_LDA_WIDE_MAX_K];
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
            if (labels) {
                for (int k = 0; k < K; ++k) {
                    const double p = (k == labels[li]) ? 1.0 : 0.0;
                    acc[k] += p;
                    if (phi) phi[(int64_t)orig[i] * K + k] = p;
                }
                if (!pos) lse[i] = 0.0;
                continue;
            }
            for (int k = 0; k < W; ++k)
                logit[k] = k < K ? vmp_lda_logit(Tseg ? Tseg[(int64_t)s * K + k] : 0.0,
                                                 Toth ? Toth[(int64_t)o * K + k] : 0.0)
                                 : -INFINITY;
            if (!pos) {
                const double m = vmp_lda_wide_max_host(logit, R);
                for (int k = 0; k < W; ++k) e[k] = k < K ? vmp_lda_shifted_exp(logit[k], m) : 0.0;
                lse[i] = vmp_lda_lse(m, vmp_lda_wide_sum_host(e, R));
                lsum += lse[i];
            }
            for (int k = 0; k < K; ++k) {
                const double p = vmp_lda_phi(logit[k], lse[li]);
                acc[k] += p;
                if (phi) phi[(int64_t)orig[i] * K + k] = p;
            }
        }
        const bool ends = seg_off[cur + 1] <= ce;
        double *dst = (inside && ends) ? N + (int64_t)cur * K : (!inside ? head + c * K : tail + c * K);
        for (int k = 0; k < K; ++k) dst[k] = acc[k];
        if (!pos) chunk_lse[c] = lsum;
    }
    for (int64_t s = 0; s < nseg; ++s) {
        const int64_t b = seg_off[s], e2 = seg_off[s + 1];
        if (b == e2) {
            for (int k = 0; k < K; ++k) N[s * K + k] = 0.0;
            continue;
        }
        const int64_t c0 = b / T, c1 = (e2 - 1) / T;
        if (c0 == c1) continue;
        for (int k = 0; k < K; ++k) {
            double sum = tail[c0 * K + k];
            for (int64_t c = c0 + 1; c < c1; ++c) sum += head[c * K + k];
            N[s * K + k] = sum + head[c1 * K + k];
        }
    }
}

}  // extern "C"
