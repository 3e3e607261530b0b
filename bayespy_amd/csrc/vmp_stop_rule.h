// vmp_stop_rule.h -- the convergence test of the VB loop (vmp.py:693-764) as plain host + device
// code: the tail kernel of a batched PCA sweep (vmp_pca_sweeps) evaluates it on the bound terms it
// has just produced, the host replays it on the same numbers, and a CPU test compiles this file
// with g++ against the Python expression.  fp64 throughout, IEEE operations only, no contraction:
// the two sides must agree bit for bit.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define VMP_STOP_HD __host__ __device__
#else
#define VMP_STOP_HD
#endif

#if defined(__clang__)
#define VMP_STOP_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VMP_STOP_NO_CONTRACT
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif

#define VMP_BOUND_TERMS 5        /* Y, X, W, tau, alpha: the order the PCA block keeps them in */
#define VMP_BOUND_MAX_ORDER 8

// L = 0.0 + t[order[0]] + t[order[1]] + ...: the sum VB.loglikelihood_lowerbound forms in MODEL
// order.  order[i] < 0 stands for a node that contributes the constant 0.0 (a deterministic node).
VMP_STOP_HD static inline double vmp_bound_sum(const double *terms, const int *order, int norder)
{
    VMP_STOP_NO_CONTRACT
    double L = 0.0;
    for (int i = 0; i < norder; ++i) L += order[i] < 0 ? 0.0 : terms[order[i]];
    return L;
}

// (L - L0) / (0.5 (|L0| + |L|)) < tol.  A NaN anywhere compares false (no stop), as on the host.
VMP_STOP_HD static inline int vmp_stop_rule(double L, double L0, double tol)
{
    VMP_STOP_NO_CONTRACT
    const double div = 0.5 * (fabs(L0) + fabs(L));
    return ((L - L0) / div < tol) ? 1 : 0;
}

#if !defined(__clang__)
#pragma GCC pop_options
#endif
