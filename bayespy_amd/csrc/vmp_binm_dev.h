// vmp_binm_dev.h -- arithmetic of the binomial-mixture block (csrc/vmp_binm.hip), shared with the
// host build of the CPU tests (tests/host/binm_host.cpp).  vmp_digamma, vmp_lgamma and vmp_lgamma_dd
// (vmp_common.h) are declared before this header is included.
//
//     R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
//     P = Beta(a0, plates=(D, K));  X = Mixture(Z, Binomial, n, P);  X.observe(x[, mask=m])
//
// n is a constant that broadcasts to (N, D) beside the cluster axis.  With l1 = <log p> - <log(1-p)>,
// l0 = <log(1-p)> (both D x K), m the mask, xt = m o x and nt = m o n a row has the logits
//     l_k = c[k] + sum_d xt_nd l1[d, k] + nt_nd l0[d, k],        c = <log pi>
// c less its largest element (vmp_bmm_dev.h gives the reason).  The binomial coefficient is the same
// for every k and never enters the logits (mixture.py, binomial.py).  The statistics are
// S[d, k] = sum_n r_nk xt_nd, T[d, k] = sum_n r_nk nt_nd and N_k; the message to P is
// counts = (S, T - S): alpha = alpha0 + S, beta = beta0 + T - S, the Dirichlet rows of two columns
// that the Bernoulli block updates (vmp_lda_dirichlet).  N_k and sum lse run over the rows with an
// observed entry.
//
// TWO PLANES OF 16 BITS PER ENTRY: vmp_binm_pack writes the count and the trials of every entry as
// one uint16 each; a hidden position gets trials VMP_BINM_HIDDEN (0xFFFF) and count 0 by a select,
// whatever stands there; the most trials are VMP_BINM_MAX_TRIALS.  The pass converts the staged 16
// bits to doubles and selects against VMP_BINM_HIDDEN when it forms an operand.
//
// TWO FORMS of the pass, chosen by the caller (the plan):
//   * two planes: two products per logit step and two statistics; COLUMN BLOCKS of
//     VMP_BINM_DBLOCK = 64, the 128 accumulator registers of the Poisson block's hidden form;
//   * one plane, when the trials are constant along the rows (n_nd = n_d) and nothing is hidden:
//     sum_d n_d l0[d, k] does not depend on the row and stands inside c (vmp_binm_tables' cfold),
//     only the plane of counts is read, and T[d, k] = n_d N_k.  That is the arithmetic of the
//     Poisson pass without hidden entries and runs on that very kernel (vmp_pmm_pass with l = l1,
//     c = cfold): column blocks of VMP_PMM_DBLOCK = 128, order of additions in vmp_pmm_dev.h.
//
// THE TABLES OF THE PASS ARE CENTRED (bit VMP_BINM_FORM_CENTRE): column 0 is taken out of every row
// of l1 and l0; vmp_pmm_dev.h gives the reason.  The bound terms use the tables as they are.
//
// ORDER OF THE ADDITIONS (what the host build restates):
//   * tables: l1 = <log p> - <log(1-p)> first, then less its column 0; c[k] = <log pi_k> less the
//     maximum; cfold[k] = <log pi_k> + sum_d n_d l0[d, k] (of the table as written), the sum from
//     zero in ascending d, then less the maximum;
//   * logit (two planes): starts at zero; the columns are walked in steps of 4: the four xt l1 of a
//     step in ascending d, then its four nt l0 in ascending d, one matrix instruction each; c[k]
//     last;
//   * softmax, slots, tiles of 64 rows, chunks, the two levels of S and T, N_k and sum lse, the
//     combine in chunk order: as in vmp_pmm_dev.h (hidden form), whose chunk and partial layout
//     this block shares; a row with nothing observed has r = softmax(c) and adds nothing to N_k and
//     sum lse and zeros to S and T;
//   * counts[d, k] = (S, T - S), one subtraction;
//   * scal[2] = S . l1 + T . l0 (two planes) is formed ROW BY ROW inside the pass, as
//     sum_n r_n . (logit_n - c) over the rows with an observed entry, which is the same number: the
//     logit of a row before c is added is sum_d xt l1 + nt l0 already, a sum of D terms of order
//     one, whereas S . l1 and T . l0 are D K products of the size of S that cancel, each with the
//     rounding of the N additions behind S (measured at (300, 70, 64): 5e-14 against 3e-13 from
//     long double).  Lane j of a 16-lane group adds r_k logit_k of its columns j, j + 16, ... in
//     ascending order and the butterfly follows, as for the softmax; per slot in row order, the 16
//     slots in slot order, the chunks in chunk order.  Under fixed labels no logits exist: one sum
//     over the elements, element e = d K + k belongs to thread e % 256 and adds S l1 + T l0 of the
//     element with the rounding errors of the products and of every addition kept
//     (vmp_binm_dot_term, vmp_pmm_sum_add), in ascending e; the 256 sums are halved eight times.
//     One plane: S . l1 (vmp_pmm_pass);
//   * pack: block b of vmp_pmm_pack_blocks(n) owns the elements [b span, (b + 1) span); thread t adds
//     the coefficients of its elements b span + t + 256 i in ascending i, keeping the rounding errors
//     (vmp_pmm_sum_add); the 256 sums are halved eight times; the blocks' partials are added in block
//     order, again with their rounding errors kept.  Entries are counted in integers.
// The bits of every output therefore depend on the packed planes, the tables and (N, D, K) only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vmp_pmm_dev.h"

#define VMP_BINM_MAX_K VMP_PMM_MAX_K
#define VMP_BINM_MAX_D VMP_PMM_MAX_D
#define VMP_BINM_MAX_TRIALS 65534
#define VMP_BINM_HIDDEN 0xFFFF
#define VMP_BINM_DBLOCK VMP_PMM_DBLOCK_HIDDEN      // columns a workgroup holds at a time, two planes

// bit of the form of vmp_binm_tables
#define VMP_BINM_FORM_CENTRE 1

// flags of the pack (four int32), for an OBSERVED entry: a negative count; a count that is no
// integer (NaN included); a count above its trials (or trials below zero); trials above
// VMP_BINM_MAX_TRIALS
#define VMP_BINM_BAD_NEGATIVE 1
#define VMP_BINM_BAD_FRACTION 2
#define VMP_BINM_BAD_ABOVE 4
#define VMP_BINM_BAD_TRIALS 8

// doubles of workspace: what the Poisson pass of the shape needs (the one-plane form runs it, the
// two-plane form has its partials), never less than the three arrays of the pack
__host__ __device__ inline int64_t vmp_binm_workspace_doubles(int64_t N, int D, int K)
{
    const int64_t w = vmp_pmm_workspace_doubles(N, D, K);
    return w > 3 * VMP_PMM_PACK_BLOCKS ? w : 3 * VMP_PMM_PACK_BLOCKS;
}

// -- the pack -----------------------------------------------------------------------------------------
// The two 16-bit values of one entry.  `seen`: the mask says observed.  A hidden entry gets
// (0, VMP_BINM_HIDDEN) by a select, whatever its value; an observed entry that fails a check gets
// them as well and sets one bit of *bad.  All checks come before the conversion to an integer, so
// NaN, -1 and 1e300 are never converted.
__host__ __device__ inline void vmp_binm_pack_f64(double v, int64_t tn, bool seen, uint16_t *xo,
                                                  uint16_t *no, int *bad)
{
    const bool whole = v == floor(v);                           // false for NaN, true for +-inf
    const bool nonneg = v >= 0.0;                               // false for NaN
    const bool tfit = tn <= (int64_t)VMP_BINM_MAX_TRIALS;
    const bool within = tn >= 0 && v <= (double)tn;             // tn < 2^53 wherever it matters
    const bool ok = whole && nonneg && tfit && within;
    const uint32_t iv = ok ? (uint32_t)v : 0u;
    if (seen && !ok)
        *bad |= !whole ? VMP_BINM_BAD_FRACTION
                       : (!nonneg ? VMP_BINM_BAD_NEGATIVE
                                  : (!tfit ? VMP_BINM_BAD_TRIALS : VMP_BINM_BAD_ABOVE));
    *xo = (seen && ok) ? (uint16_t)iv : (uint16_t)0;
    *no = (seen && ok) ? (uint16_t)tn : (uint16_t)VMP_BINM_HIDDEN;
}

__host__ __device__ inline void vmp_binm_pack_i64(int64_t v, int64_t tn, bool seen, uint16_t *xo,
                                                  uint16_t *no, int *bad)
{
    const bool nonneg = v >= 0;
    const bool tfit = tn <= (int64_t)VMP_BINM_MAX_TRIALS;
    const bool within = tn >= 0 && v <= tn;
    const bool ok = nonneg && tfit && within;
    if (seen && !ok)
        *bad |= !nonneg ? VMP_BINM_BAD_NEGATIVE : (!tfit ? VMP_BINM_BAD_TRIALS : VMP_BINM_BAD_ABOVE);
    *xo = (seen && ok) ? (uint16_t)v : (uint16_t)0;
    *no = (seen && ok) ? (uint16_t)tn : (uint16_t)VMP_BINM_HIDDEN;
}

// an entry of any dtype the pack takes: a double by vmp_binm_pack_f64, every integer by
// vmp_binm_pack_i64
__host__ __device__ inline void vmp_binm_pack(double v, int64_t tn, bool seen, uint16_t *xo,
                                              uint16_t *no, int *bad)
{
    vmp_binm_pack_f64(v, tn, seen, xo, no, bad);
}

template <typename T>
__host__ __device__ inline void vmp_binm_pack(T v, int64_t tn, bool seen, uint16_t *xo,
                                              uint16_t *no, int *bad)
{
    vmp_binm_pack_i64((int64_t)v, tn, seen, xo, no, bad);
}

__host__ __device__ inline bool vmp_binm_observed(uint16_t np) { return np != VMP_BINM_HIDDEN; }

// lgamma(p + 1) as a sum hi + lo; exactly zero for 0 and 1.  Up to 20 the factorial is an exact
// integer and its logarithm is rounded once; above, vmp_lgamma_dd.
__host__ __device__ inline double vmp_binm_lfact(uint32_t p, double *lo)
{
    *lo = 0.0;
    if (p < 2) return 0.0;
    if (p <= 20) {
        uint64_t f = 2;
        for (uint64_t i = 3; i <= p; ++i) f *= i;
        return log((double)f);
    }
    return vmp_lgamma_dd((double)p + 1.0, 0.0, lo);
}

// log of the binomial coefficient of a packed entry: lgamma(n + 1) - lgamma(x + 1) - lgamma(n - x + 1),
// the high parts first, then the low parts; exactly zero for a hidden entry, x = 0 and x = n
__host__ __device__ inline double vmp_binm_lchoose(uint16_t xp, uint16_t np)
{
    if (!vmp_binm_observed(np) || xp == 0 || xp >= np) return 0.0;
    double ln, lx, ld;
    const double hn = vmp_binm_lfact(np, &ln), hx = vmp_binm_lfact(xp, &lx);
    const double hd = vmp_binm_lfact((uint32_t)np - xp, &ld);
    return ((hn - hx) - hd) + ((ln - lx) - ld);
}

// -- the operands, from the staged 16 bits of the two planes ------------------------------------------
__host__ __device__ inline double vmp_binm_count(uint16_t xp, uint16_t np)
{
    return vmp_binm_observed(np) ? (double)xp : 0.0;
}

__host__ __device__ inline double vmp_binm_trials(uint16_t np)
{
    return vmp_binm_observed(np) ? (double)np : 0.0;
}

// -- the tables ---------------------------------------------------------------------------------------
__host__ __device__ inline double vmp_binm_l1(double elog_p, double elog_q) { return elog_p - elog_q; }

// an entry of a table of the pass: column 0 of its row taken out where the form says so
__host__ __device__ inline double vmp_binm_table(double v, double v0, int form)
{
    return (form & VMP_BINM_FORM_CENTRE) ? v - v0 : v;
}

// -- the tail -------------------------------------------------------------------------------------------
// the second column of the message to P
__host__ __device__ inline double vmp_binm_failures(double t, double s) { return t - s; }

// T of the one-plane form
__host__ __device__ inline double vmp_binm_t_const(double n_d, double nk) { return n_d * nk; }

// one term of scal[2] of the two-plane form under fixed labels: s a + t b, the rounding errors of the two products and
// of their sum to *err
__host__ __device__ inline double vmp_binm_dot_term(double s, double a, double t, double b,
                                                    double *err)
{
    const double p = s * a, pe = fma(s, a, -p), q = t * b, qe = fma(t, b, -q);
    double se;
    const double v = vmp_two_sum(p, q, &se);
    *err = se + (pe + qe);
    return v;
}
