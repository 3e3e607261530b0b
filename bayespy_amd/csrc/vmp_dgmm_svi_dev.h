// vmp_dgmm_svi_dev.h -- arithmetic of a stochastic-VI step of the two diagonal-Gaussian-mixture
// blocks (csrc/vmp_dgmm_svi.hip), shared with the host build of the CPU tests
// (tests/host/dgmm_svi_host.cpp).  vmp_digamma and vmp_lgamma (vmp_common.h) are declared before
// this header is included.
//
// A mini-batch stands for mult times its rows.  Element e = d K + k of mu and of tau moves along its
// natural gradient (vmp.py:432-440), both from the state at entry:
//
//     mu    phi = (lambda m, -lambda / 2):   lambda* = beta0 + mult <tau> cnt
//                                            (lambda m)* = beta0 m0 + mult <tau> S1
//     tau   phi = (a, b):                    a* = a0 + mult cnt / 2
//                                            b* = b0 + mult (S2 - 2 <mu> S1 + <mu^2> cnt) / 2
//     phi <- phi + scale (phi* - phi)
//
// Element e of mu reads <tau> of element e, element e of tau reads <mu> and <mu^2> of element e and
// nothing else couples the two tables, so one call reads both old moments, forms both optima and
// only then stores: the order of the two nodes does not enter.
//
// scale == 1 does not read the old parameters (the NaN of a point mass may stand there) and runs
// vmp_dgmm_update_mu / vmp_dgmm_update_tau (vmp_dgmm_masked_update_tau where the count is per
// element) on the scaled statistics: mult == 1 leaves the bits of vmp_dgmm_update /
// vmp_dgmm_update_masked in par, mom and the element's bound term.  Otherwise the bound term of the
// stepped q is A - B of vmp_dgmm_parts_mu / vmp_dgmm_parts_tau.
#pragma once

#include "vmp_dgmm_masked_dev.h"

#define VMP_DGMM_SVI_MU 1
#define VMP_DGMM_SVI_TAU 2
#define VMP_DGMM_SVI_WEIGHTS 4

// one step of a natural parameter
__host__ __device__ inline double vmp_dgmm_svi_move(double old, double opt, double scale)
{
    return old + scale * (opt - old);
}

// q(mu_e) one step on: par = (m, lambda), mom = (<mu>, <mu^2>); returns its bound term.  `tau` is
// <tau_e> at entry, `mc` = mult cnt and `ms1` = mult S1 (zero without statistics).
__host__ __device__ inline double vmp_dgmm_svi_mu(double m0, double beta0, double tau, double mc,
                                                  double ms1, double scale, double *par,
                                                  double *mom)
{
    if (scale == 1.0) return vmp_dgmm_update_mu(m0, beta0, tau, mc, ms1, par, mom);
    const double lam_o = par[1], lm_o = par[1] * par[0];
    const double lam = vmp_dgmm_svi_move(lam_o, beta0 + tau * mc, scale);
    const double lm = vmp_dgmm_svi_move(lm_o, beta0 * m0 + tau * ms1, scale);
    const double m = lm / lam;
    par[0] = m;
    par[1] = lam;
    mom[0] = m;
    mom[1] = m * m + 1.0 / lam;
    double A, B;
    vmp_dgmm_parts_mu(m0, beta0, par, &A, &B);
    return A - B;
}

// q(tau_e) one step on: par = (a, b), mom = (<tau>, <log tau>); returns its bound term.  `mu1` and
// `mu2` are <mu_e> and <mu_e^2> at entry, `mc`, `ms1`, `ms2` = mult (cnt, S1, S2).
__host__ __device__ inline double vmp_dgmm_svi_tau(double a0, double b0, double mu1, double mu2,
                                                   double mc, double ms1, double ms2, double scale,
                                                   int per_element, double *par, double *mom)
{
    if (scale == 1.0)
        return per_element ? vmp_dgmm_masked_update_tau(a0, b0, mu1, mu2, mc, ms1, ms2, par, mom)
                           : vmp_dgmm_update_tau(a0, b0, mu1, mu2, mc, ms1, ms2, par, mom);
    const double a_s = a0 + 0.5 * mc;
    const double b_s = b0 + 0.5 * (ms2 - 2.0 * mu1 * ms1 + mu2 * mc);
    const double a = vmp_dgmm_svi_move(par[0], a_s, scale);
    const double b = vmp_dgmm_svi_move(par[1], b_s, scale);
    par[0] = a;
    par[1] = b;
    mom[0] = a / b;
    mom[1] = vmp_digamma(a) - log(b);
    double A, B;
    vmp_dgmm_parts_tau(a0, b0, par, mom, &A, &B);
    return A - B;
}

// Element e of both tables (pointers at the element's pair).  Everything the two steps read is read
// before anything is stored.  `nodes`: VMP_DGMM_SVI_MU | VMP_DGMM_SVI_TAU; the tables of a node that
// is not named are read at most (its moments, where the named one needs them), and its term is left
// alone.  `stats` == 0: phi* is the prior, and as in vmp_dgmm_update the moments of the other node
// are not looked at.
__host__ __device__ inline void vmp_dgmm_svi_element(int nodes, int per_element, int stats,
                                                     double m0, double beta0, double a0, double b0,
                                                     double s1, double s2, double cnt, double mult,
                                                     double scale, double *mu_par, double *mu_mom,
                                                     double *tau_par, double *tau_mom, double *L_mu,
                                                     double *L_tau)
{
    const bool mu = (nodes & VMP_DGMM_SVI_MU) != 0, ta = (nodes & VMP_DGMM_SVI_TAU) != 0;
    const double tau = stats && mu ? tau_mom[0] : 0.0;
    const double mu1 = stats && ta ? mu_mom[0] : 0.0, mu2 = stats && ta ? mu_mom[1] : 0.0;
    const double mc = stats ? mult * cnt : 0.0, ms1 = stats ? mult * s1 : 0.0;
    const double ms2 = stats ? mult * s2 : 0.0;
    if (mu)
        *L_mu = vmp_dgmm_svi_mu(m0, beta0, tau, mc, ms1, scale, mu_par, mu_mom);
    if (ta)
        *L_tau = vmp_dgmm_svi_tau(a0, b0, mu1, mu2, mc, ms1, ms2, scale, per_element, tau_par,
                                  tau_mom);
}
