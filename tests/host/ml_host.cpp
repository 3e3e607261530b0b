// TEST DOUBLE: the maximum-likelihood updates of csrc/vmp_ml.hip on the host, built with g++ from the
// very header the kernels include (csrc/vmp_ml_dev.h) plus the special functions sliced out of
// vmp_common.h (-include, see tests/ml_host.py).  The concentration loop is the kernel's loop run by
// one thread: every element steps every iteration (old values in one buffer, new ones in the other),
// the loop ends at the first iteration in which no element moved, capped at max_iter.
#include <math.h>
#include <stdint.h>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_ml_dev.h"

extern "C" {

void ml_invpsi(int64_t n, const double *x, double *y)
{
    for (int64_t i = 0; i < n; ++i) y[i] = vmp_invpsi(x[i]);
}

void ml_gamma_shape(int64_t n, const double *m0, const double *m1, const double *r0,
                    const double *r1, double *a, double *lga)
{
    for (int64_t i = 0; i < n; ++i) {
        a[i] = vmp_ml_gamma_shape_value(m0[i], m1[i], r0[i], r1[i]);
        lga[i] = vmp_lgamma(a[i]);
    }
}

void ml_concentration(int64_t rows, int K, const double *m0, const double *m1, const double *r0,
                      const double *r1, int max_iter, double *alpha, double *work, double *z,
                      int32_t *status)
{
    const int64_t ne = rows * K;
    bool inf = false;
    for (int64_t e = 0; e < ne; ++e) {
        const int64_t r = e / K;
        if (vmp_ml_isinf(vmp_ml_mean_logp(m0[e], r0[e], m1[r] + r1[r]))) inf = true;
        alpha[e] = 1.0;
    }
    int it = 0;
    bool capped = false;
    if (!inf) {
        for (;;) {
            if (it == max_iter) {
                capped = true;
                break;
            }
            const double *cur = (it & 1) ? work : alpha;
            double *nxt = (it & 1) ? alpha : work;
            bool moved = false;
            for (int64_t e = 0; e < ne; ++e) {
                const int64_t r = e / K;
                const double an = vmp_ml_concentration_element(cur + r * K, K, m0[e], m1[r], r0[e],
                                                                r1[r]);
                if (vmp_ml_moved(an, cur[e])) moved = true;
                nxt[e] = an;
            }
            ++it;
            if (!moved) break;
        }
    }
    if (it & 1)
        for (int64_t e = 0; e < ne; ++e) alpha[e] = work[e];
    for (int64_t r = 0; r < rows; ++r) z[r] = vmp_ml_concentration_z(alpha + r * K, K);
    status[0] = inf ? 1 : 0;
    status[1] = capped ? 1 : 0;
    status[2] = it;
}

}  // extern "C"
