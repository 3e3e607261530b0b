// vmp_table_dev.h -- one row of a Dirichlet table, for the kernels that set it (vmp_lda_dirichlet),
// step it (vmp_lda_dirichlet_step) or step it beside another table in one launch
// (vmp_mix_natural_step, csrc/vmp_mix_svi.hip).  Included after vmp_common.h (vmp_digamma,
// vmp_lgamma, block_sum).
//
// Element (r, c) of every array stands at r * rs + c * cs.  A row leaves alpha, <log> and its term
// of the lower bound, <log p> - <log q> = sum_c (p_c - a_c) <log>_c + lnB(a) - lnB(p).  The order of
// the additions depends on the number of columns and, for the workgroup form, on NT alone.
#pragma once

constexpr int VMP_TABLE_NT = 256;           // threads of the kernels that walk Dirichlet rows
constexpr int VMP_TABLE_THREAD_COLS = 64;   // up to here a thread owns a row, above a workgroup

// The parameter a Dirichlet step leaves at element e: q = prior + mult * counts, and from the
// present alpha a step of length `scale` towards q.  scale == 1 does not read alpha (it may hold the
// NaN of a point mass).
__device__ __forceinline__ double vmp_table_step_value(double p, const double *__restrict__ counts,
                                                       int64_t e, double mult, double scale,
                                                       const double *alpha)
{
    const double q = counts ? p + mult * counts[e] : p;
    if (scale == 1.0) return q;
    const double a = alpha[e];
    return a + scale * (q - a);
}

// Row r by one thread.  STEP: alpha moves by vmp_table_step_value instead of being set to
// prior + counts.
template <bool STEP>
__device__ __forceinline__ double vmp_dirichlet_row_thread(int64_t r, int cols, int64_t rs,
                                                           int64_t cs,
                                                           const double *__restrict__ prior,
                                                           const double *__restrict__ counts,
                                                           double mult, double scale, double *alpha,
                                                           double *__restrict__ elog)
{
    double s = 0.0, s0 = 0.0;
    for (int c = 0; c < cols; ++c) {
        const int64_t e = r * rs + c * cs;
        const double p = prior[e];
        const double v = STEP ? vmp_table_step_value(p, counts, e, mult, scale, alpha)
                              : (counts ? p + counts[e] : p);
        alpha[e] = v;
        s += v;
        s0 += p;
    }
    const double psis = vmp_digamma(s);
    double g = vmp_lgamma(s), g0 = vmp_lgamma(s0), L = 0.0;
    for (int c = 0; c < cols; ++c) {
        const int64_t e = r * rs + c * cs;
        const double p = prior[e], v = alpha[e];
        const double el = vmp_digamma(v) - psis;
        elog[e] = el;
        g -= vmp_lgamma(v);
        g0 -= vmp_lgamma(p);
        L += (p - v) * el;
    }
    return L + g0 - g;
}

// Row r by a workgroup of NT threads; every thread returns the row's term.  `red`: NT / 64 doubles
// of LDS.
template <bool STEP, int NT>
__device__ __forceinline__ double vmp_dirichlet_row_block(int64_t r, int64_t cols, int64_t rs,
                                                          int64_t cs,
                                                          const double *__restrict__ prior,
                                                          const double *__restrict__ counts,
                                                          double mult, double scale, double *alpha,
                                                          double *__restrict__ elog, double *red)
{
    double s = 0.0, s0 = 0.0;
    for (int64_t c = threadIdx.x; c < cols; c += NT) {
        const int64_t e = r * rs + c * cs;
        const double p = prior[e];
        const double v = STEP ? vmp_table_step_value(p, counts, e, mult, scale, alpha)
                              : (counts ? p + counts[e] : p);
        alpha[e] = v;
        s += v;
        s0 += p;
    }
    s = block_sum<NT>(s, red);
    s0 = block_sum<NT>(s0, red);
    const double psis = vmp_digamma(s);
    double g = 0.0, g0 = 0.0, L = 0.0;
    for (int64_t c = threadIdx.x; c < cols; c += NT) {
        const int64_t e = r * rs + c * cs;
        const double p = prior[e], v = alpha[e];       // this thread's own stores
        const double el = vmp_digamma(v) - psis;
        elog[e] = el;
        g += vmp_lgamma(v);
        g0 += vmp_lgamma(p);
        L += (p - v) * el;
    }
    g = block_sum<NT>(g, red);
    g0 = block_sum<NT>(g0, red);
    L = block_sum<NT>(L, red);
    return L + (vmp_lgamma(s0) - g0) - (vmp_lgamma(s) - g);
}
