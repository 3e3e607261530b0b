// vmp_ml_dev.h -- per-element / per-row arithmetic of the maximum-likelihood hyperparameter nodes
// (GammaShape gamma.py:273-334, Concentration dirichlet.py:234-330), shared by the kernels of
// vmp_ml.hip and the host build of the CPU tests.  Include after vmp_common.h (vmp_digamma,
// vmp_lgamma, vmp_invpsi).
#pragma once

// relative change above which an element of a concentration row has not converged yet
#define VMP_ML_CONC_TOL 1e-5

// ML shape of a gamma node: psi(a) = -m0 / m1 with the messages of the children plus the node's own
// "prior" terms (gamma.py:316-318)
__host__ __device__ inline double vmp_ml_gamma_shape_value(double m0, double m1, double r0, double r1)
{
    return vmp_invpsi(-(m0 + r0) / (m1 + r1));
}

__host__ __device__ inline bool vmp_ml_isinf(double x) { return x == INFINITY || x == -INFINITY; }

// mean_logp of a row: (m0 + reg0) / (m1 + reg1) elementwise (dirichlet.py:288-293)
__host__ __device__ inline double vmp_ml_mean_logp(double m0, double r0, double n)
{
    return (m0 + r0) / n;
}

// One element of a step of the fixed point of dirichlet.py:305-311: the new value of element k of a
// row from the row's OLD values, invpsi(psi(sum a) + mean_logp_k).  The row sum runs in index order
// whoever evaluates it, so every element of a row sees the same psi(sum a).
__host__ __device__ inline double vmp_ml_concentration_element(const double *a_row, int K, double m0k,
                                                              double m1, double r0k, double r1)
{
    double s = 0.0;
    for (int j = 0; j < K; ++j) s += a_row[j];
    return vmp_invpsi(vmp_digamma(s) + vmp_ml_mean_logp(m0k, r0k, m1 + r1));
}

// Has an element not converged yet?  |da / a| with the NEW value (the reference tests it after
// `a = a_new`); a NaN compares false.
__host__ __device__ inline bool vmp_ml_moved(double a_new, double a_old)
{
    return fabs((a_new - a_old) / a_new) > VMP_ML_CONC_TOL;
}

// second moment of a concentration row: lgamma(sum a) - sum lgamma(a) (dirichlet.py:37-51)
__host__ __device__ inline double vmp_ml_concentration_z(const double *a, int K)
{
    double s = 0.0, lg = 0.0;
    for (int k = 0; k < K; ++k) {
        s += a[k];
        lg += vmp_lgamma(a[k]);
    }
    return vmp_lgamma(s) - lg;
}
