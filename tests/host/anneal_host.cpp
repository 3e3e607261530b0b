// TEST DOUBLE: the annealed tables and updates of csrc/vmp_dgmm.hip on the host, built with g++ from
// the very header the kernels include (csrc/vmp_dgmm_dev.h); the special functions of vmp_common.h
// come in ahead of this file (host_build.special_functions_text).  The parts A and B of a bound
// term are added as the kernel adds them: element e to thread e % 256, the 256 sums halved eight
// times.
#include <math.h>
#include <stdint.h>
#include <vector>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_dgmm_dev.h"

static double halve_sum(std::vector<double> &v)
{
    for (int off = VMP_DGMM_NT / 2; off > 0; off >>= 1)
        for (int i = 0; i < off; ++i) v[i] += v[i + off];
    return v[0];
}

extern "C" {

void anneal_tables(int D, int K, double ab, const double *mu_mom, const double *tau_mom,
                   const double *elog_pi, double *h, double *q, double *c, double *gsum)
{
    for (int i = 0; i < D * K; ++i) {
        h[i] = vmp_dgmm_anneal(ab, vmp_dgmm_h(tau_mom[2 * i], mu_mom[2 * i]));
        q[i] = vmp_dgmm_anneal(ab, vmp_dgmm_q(tau_mom[2 * i]));
    }
    std::vector<double> cs(K);
    for (int k = 0; k < K; ++k) {
        double t = 0.0;
        for (int d = 0; d < D; ++d) {
            const int e = d * K + k;
            t += vmp_dgmm_g(tau_mom[2 * e], tau_mom[2 * e + 1], mu_mom[2 * e + 1]);
        }
        if (gsum) gsum[k] = t;
        cs[k] = vmp_dgmm_anneal(ab, t + elog_pi[k]);
    }
    double m = cs[0];
    for (int k = 1; k < K; ++k) m = fmax(m, cs[k]);
    for (int k = 0; k < K; ++k) c[k] = cs[k] - m;
}

// which 0 / 1: the annealed update of mu / tau; 2 / 3: the parts alone of the q in par and mom
void anneal_update(int D, int K, int which, double beta, const double *prior_a,
                   const double *prior_b, const double *S1, const double *S2, const double *Nk,
                   const double *other, double *par, double *mom, double *ab)
{
    std::vector<double> as(VMP_DGMM_NT, 0.0), bs(VMP_DGMM_NT, 0.0);
    for (int e = 0; e < D * K; ++e) {
        const int k = e % K;
        double A, B;
        if (which == 2) vmp_dgmm_parts_mu(prior_a[e], prior_b[e], par + 2 * e, &A, &B);
        else if (which == 3) vmp_dgmm_parts_tau(prior_a[e], prior_b[e], par + 2 * e, mom + 2 * e, &A, &B);
        else if (which == 0)
            vmp_dgmm_update_mu_annealed(beta, prior_a[e], prior_b[e], other[2 * e], Nk[k], S1[e],
                                        par + 2 * e, mom + 2 * e, &A, &B);
        else
            vmp_dgmm_update_tau_annealed(beta, prior_a[e], prior_b[e], other[2 * e],
                                         other[2 * e + 1], Nk[k], S1[e], S2[e], par + 2 * e,
                                         mom + 2 * e, &A, &B);
        as[e % VMP_DGMM_NT] += A;
        bs[e % VMP_DGMM_NT] += B;
    }
    ab[0] = halve_sum(as);
    ab[1] = halve_sum(bs);
}

}  // extern "C"
