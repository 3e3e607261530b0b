// TEST DOUBLE: the table half of csrc/vmp_dgmm_svi.hip on the host, built with g++ from the very
// header the kernel includes (csrc/vmp_dgmm_svi_dev.h); the special functions of vmp_common.h come
// in ahead of this file (host_build.special_functions_text).  The elements are walked one after the
// other -- each reads what it needs of both tables before it stores -- and the bound terms are added
// in the order the kernel states: element e to thread e % 256 in ascending order, the 256 sums
// halved eight times.
#include <math.h>
#include <stdint.h>
#include <vector>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_dgmm_svi_dev.h"

static double dgmm_svi_sum(const std::vector<double> &t)
{
    double v[VMP_DGMM_NT];
    for (int tid = 0; tid < VMP_DGMM_NT; ++tid) {
        double s = 0.0;
        for (size_t e = tid; e < t.size(); e += VMP_DGMM_NT) s += t[e];
        v[tid] = s;
    }
    for (int off = VMP_DGMM_NT / 2; off > 0; off >>= 1)
        for (int i = 0; i < off; ++i) v[i] += v[i + off];
    return v[0];
}

extern "C" {

// bound[0] of mu, bound[1] of tau, each written only when its node is named; null statistics: the
// prior
void dgmm_svi_step(int D, int K, int nodes, int per_element, const double *m0, const double *beta0,
                   const double *a0, const double *b0, const double *S1, const double *S2,
                   const double *cnt, double *mu_par, double *mu_mom, double *tau_par,
                   double *tau_mom, double mult, double scale, double *bound)
{
    const int stats = S1 && S2 && cnt;
    const int64_t DK = (int64_t)D * K;
    std::vector<double> tm((size_t)DK, 0.0), tt((size_t)DK, 0.0);
    for (int64_t e = 0; e < DK; ++e) {
        const double c = stats ? (per_element ? cnt[e] : cnt[e % K]) : 0.0;
        vmp_dgmm_svi_element(nodes, per_element, stats, m0 ? m0[e] : 0.0, beta0 ? beta0[e] : 0.0,
                             a0 ? a0[e] : 0.0, b0 ? b0[e] : 0.0, stats ? S1[e] : 0.0,
                             stats ? S2[e] : 0.0, c, mult, scale, mu_par + 2 * e, mu_mom + 2 * e,
                             tau_par + 2 * e, tau_mom + 2 * e, &tm[e], &tt[e]);
    }
    if (nodes & VMP_DGMM_SVI_MU) bound[0] = dgmm_svi_sum(tm);
    if (nodes & VMP_DGMM_SVI_TAU) bound[1] = dgmm_svi_sum(tt);
}

}  // extern "C"
