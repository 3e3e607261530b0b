// vmp_pmm_dev.h -- arithmetic of the Poisson-mixture block (csrc/vmp_pmm.hip), shared with the host
// build of the CPU tests (tests/host/pmm_host.cpp).  vmp_digamma, vmp_lgamma and vmp_lgamma_dd
// (vmp_common.h) are declared before this header is included.
//
//     R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
//     lam = Gamma(a0, b0, plates=(D, K));  X = Mixture(Z, Poisson, lam);  X.observe(x[, mask=m])
//
// With l = <log lam>, lb = <lam> (both D x K), m the mask and xt = m o x a row of counts has the logits
//     nothing hidden:  l_k = c[k] + sum_d x_nd l[d, k],              c = <log pi> - sum_d lb[d, .]
//     hidden entries:  l_k = c[k] + sum_d xt_nd l[d, k] - m_nd lb[d, k],   c = <log pi>
// each c less its largest element (vmp_bmm_dev.h gives the reason).  sum_d lgamma(x + 1) is the same
// for every k and never enters the logits (mixture.py: the (N, D, K) broadcast of the Poisson
// log-density summed over D plus the message of the Categorical parent; poisson.py).  The statistics
// are S[d, k] = sum_n r_nk xt_nd, N_k and, with hidden entries, M[d, k] = sum_n r_nk m_nd, which
// takes the place of N_k in the update of lam: a = a0 + S, b = b0 + N_k (or M).  N_k and sum lse
// run over the rows with an observed entry.
//
// x IS KEPT AS 16 BITS PER ENTRY: vmp_pmm_pack writes one uint16 per count, VMP_PMM_HIDDEN (0xFFFF)
// at a hidden position by a select, whatever stands there; the largest count is VMP_PMM_MAX_COUNT.
// The pass converts the staged 16 bits to a double and selects against VMP_PMM_HIDDEN when it forms
// an operand; it reads no other array of size N D.
//
// TWO FORMS of the pass, chosen by the caller (the plan: hidden = n_hidden > 0; a mask of ones runs
// the form without hidden entries and gives its bits):
//   * nothing hidden: one product per logit step and one statistic; the columns are held in COLUMN
//     BLOCKS of VMP_PMM_DBLOCK = 128;
//   * hidden: two products per step and two statistics; COLUMN BLOCKS of VMP_PMM_DBLOCK_HIDDEN = 64.
// Either way a block is 32 accumulator tiles of 16 x 16 at K = 64, eight per wavefront, held twice
// (the tile of rows and the chunk): 128 registers, the budget of the Gaussian passes.  An element's
// sum does not depend on the block width.
//
// THE TABLES OF THE PASS ARE CENTRED (bit VMP_PMM_FORM_CENTRE of the form): column 0 is taken out
// of every row, l[d, k] - l[d, 0] and lb[d, k] - lb[d, 0].  That moves every logit of a row by one
// amount, so r does not change, and sum lse and scal[2] move by the same sum, so the entropy
// sum lse - N_k . c - scal[2] does not change either; but the logits are sums of D differences
// between clusters instead of D log-rates (2400 at D = 257 and rates near 5, where one ulp of the
// logit is 5e-13 of r).  The bound term of X needs the tables as they are: the plan asks for them
// without the bit.
//
// ORDER OF THE ADDITIONS (what the host build restates):
//   * tables: lsum[k] = sum_d lb[d, k] (of the table as written, centred or not) from zero in
//     ascending d; c[k] = <log pi_k> - lsum[k] (nothing hidden) or <log pi_k> (bit
//     VMP_PMM_FORM_HIDDEN), then less the maximum;
//   * logit: starts at zero; the columns are walked in steps of 4: the four xt l of a step in
//     ascending d, then (hidden form) its four m (-lb) in ascending d, one matrix instruction each;
//     c[k] last;
//   * softmax, slots, tiles of 64 rows and chunks as in vmp_dgmm_dev.h / vmp_dgmm_masked_dev.h: K
//     is padded to a multiple of 16 with -inf logits, lane j of a 16-lane group adds its columns
//     j, j + 16, ... in ascending order and the butterfly follows; N_k and sum lse per slot in row
//     order, the 16 slots in slot order at the end of a chunk.  r_k = exp(l_k - m) / s with the
//     very exponentials of the sum s under the logarithm: a row of r adds up to one within an ulp,
//     where exp(l_k - lse) inherits the rounding of lse = m + log s at the size of m (1e-13 at the
//     logits of a few hundred columns), which N_k . c and S . l multiply by that size.  A row with
//     nothing observed has r = softmax(c) and adds nothing to N_k and sum lse and zeros to S and M;
//   * S and M in two levels: within a tile of 64 rows from zero in ascending row order, the tiles'
//     sums in tile order to the running sum of the chunk;
//   * a workgroup owns one chunk of vmp_pmm_chunk_rows(N, D, K) consecutive rows; the partials are
//     added in chunk order by a second kernel;
//   * scal[2] = S . l (nothing hidden: the lb part is inside c) or S . l - M . lb (two dot products);
//   * pack: sum lgamma(x + 1) over the observed entries.  Block b of vmp_pmm_pack_blocks(n) owns the
//     elements [b span, (b + 1) span), span = vmp_pmm_pack_span(n); thread t adds its elements
//     b span + t + 256 i in ascending i, keeping the rounding errors of the additions
//     (vmp_pmm_sum_add); the 256 sums are halved eight times; the blocks' partials are added in
//     block order, again with their rounding errors kept.  The hidden entries are counted in
//     integers;
//   * update: element e = d K + k belongs to thread e % 256, which adds its bound terms in ascending
//     order; the 256 sums are halved eight times.
// The bits of every output therefore depend on the packed x, the tables and (N, D, K) only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vmp_dgmm_masked_dev.h"

#define VMP_PMM_MAX_K 64
#define VMP_PMM_MAX_D 1024
#define VMP_PMM_MAX_COUNT 65534
#define VMP_PMM_HIDDEN 0xFFFF
#define VMP_PMM_TILE 64            // rows per tile: 16 per wavefront of a four-wavefront workgroup
#define VMP_PMM_NT 256             // threads of every kernel of the block
#define VMP_PMM_DBLOCK 128         // columns a workgroup holds at a time, nothing hidden
#define VMP_PMM_DBLOCK_HIDDEN 64   // with hidden entries (two statistics)
#define VMP_PMM_MIN_CHUNK 256
#define VMP_PMM_MAX_CHUNKS 1024
#define VMP_PMM_PACK_BLOCKS 1024   // most blocks of the pack; its workspace is twice as many doubles

// bits of the form of vmp_pmm_tables
#define VMP_PMM_FORM_HIDDEN 1
#define VMP_PMM_FORM_CENTRE 2

// flags of the pack (three int32): an observed value that is negative or no integer; one above
// VMP_PMM_MAX_COUNT; one that is no integer (which of poisson.py's two messages applies)
#define VMP_PMM_BAD_INVALID 1
#define VMP_PMM_BAD_ABOVE 2
#define VMP_PMM_BAD_FRACTION 4

__host__ __device__ inline int vmp_pmm_kpad(int K) { return (K + 15) & ~15; }

__host__ __device__ inline int vmp_pmm_dblock(int hidden)
{
    return hidden ? VMP_PMM_DBLOCK_HIDDEN : VMP_PMM_DBLOCK;
}

// doubles one chunk leaves behind: S (K x D), with hidden entries M (K x D), N_k (K), sum lse (1)
__host__ __device__ inline int64_t vmp_pmm_partial_doubles(int D, int K, int hidden)
{
    return (hidden ? 2 : 1) * (int64_t)D * K + K + 1;
}

// rows of a chunk: a function of (N, D, K) alone, the same for both forms (the larger partial
// counts).  At most VMP_PMM_MAX_CHUNKS chunks and at most 2^25 doubles (256 MB) of partials; a
// multiple of the tile, at least VMP_PMM_MIN_CHUNK.
__host__ __device__ inline int64_t vmp_pmm_chunk_rows(int64_t N, int D, int K)
{
    int64_t maxc = ((int64_t)1 << 25) / vmp_pmm_partial_doubles(D, K, 1);
    if (maxc > VMP_PMM_MAX_CHUNKS) maxc = VMP_PMM_MAX_CHUNKS;
    if (maxc < 1) maxc = 1;
    int64_t rows = (N + maxc - 1) / maxc;
    rows = (rows + VMP_PMM_TILE - 1) / VMP_PMM_TILE * VMP_PMM_TILE;
    if (rows < VMP_PMM_MIN_CHUNK) rows = VMP_PMM_MIN_CHUNK;
    return rows;
}

__host__ __device__ inline int64_t vmp_pmm_chunks(int64_t N, int D, int K)
{
    const int64_t rows = vmp_pmm_chunk_rows(N, D, K);
    return N > 0 ? (N + rows - 1) / rows : 0;
}

// doubles of workspace: the partials, the partial sums of a dot product, the two dot products of
// scal[2]; never less than the pack needs
__host__ __device__ inline int64_t vmp_pmm_workspace_doubles(int64_t N, int D, int K)
{
    const int64_t w = vmp_pmm_chunks(N, D, K) * vmp_pmm_partial_doubles(D, K, 1) + 1024 + 2;
    return w > 2 * VMP_PMM_PACK_BLOCKS ? w : 2 * VMP_PMM_PACK_BLOCKS;
}

// elements of one block of the pack, and the number of blocks: functions of n = N D alone
__host__ __device__ inline int64_t vmp_pmm_pack_span(int64_t n)
{
    int64_t span = (n + VMP_PMM_PACK_BLOCKS - 1) / VMP_PMM_PACK_BLOCKS;
    span = (span + VMP_PMM_NT - 1) / VMP_PMM_NT * VMP_PMM_NT;
    return span < VMP_PMM_NT ? VMP_PMM_NT : span;
}

__host__ __device__ inline int64_t vmp_pmm_pack_blocks(int64_t n)
{
    const int64_t span = vmp_pmm_pack_span(n);
    return (n + span - 1) / span;
}

// slot of row t (0 .. 63) of a tile
__host__ __device__ inline int vmp_pmm_slot(int t) { return (t >> 4) * 4 + (t & 3); }

// -- the pack -----------------------------------------------------------------------------------------
// The 16 bits of one entry.  `seen`: the mask says observed.  A hidden entry gets VMP_PMM_HIDDEN by a
// select, whatever its value; an observed value that fails a check gets it as well and sets bits of
// *bad.  The range checks come before the conversion to an integer, so NaN, -1 and 1e300 are never
// converted.
__host__ __device__ inline uint16_t vmp_pmm_pack_f64(double v, bool seen, int *bad)
{
    const bool nonneg = v >= 0.0;                               // false for NaN
    const bool whole = v == floor(v);                           // false for NaN, true for +-inf
    const bool fits = nonneg && v <= (double)VMP_PMM_MAX_COUNT;
    const uint32_t iv = fits ? (uint32_t)v : 0u;
    const bool ok = fits && whole;
    if (seen && !ok)
        *bad |= !whole ? (VMP_PMM_BAD_INVALID | VMP_PMM_BAD_FRACTION)
                       : (!nonneg ? VMP_PMM_BAD_INVALID : VMP_PMM_BAD_ABOVE);
    return (seen && ok) ? (uint16_t)iv : (uint16_t)VMP_PMM_HIDDEN;
}

__host__ __device__ inline uint16_t vmp_pmm_pack_i64(int64_t v, bool seen, int *bad)
{
    const bool ok = (uint64_t)v <= (uint64_t)VMP_PMM_MAX_COUNT;
    if (seen && !ok) *bad |= v < 0 ? VMP_PMM_BAD_INVALID : VMP_PMM_BAD_ABOVE;
    return (seen && ok) ? (uint16_t)v : (uint16_t)VMP_PMM_HIDDEN;
}

// an entry of any dtype the pack takes: a double by vmp_pmm_pack_f64, every integer by
// vmp_pmm_pack_i64
__host__ __device__ inline uint16_t vmp_pmm_pack(double v, bool seen, int *bad)
{
    return vmp_pmm_pack_f64(v, seen, bad);
}

template <typename T>
__host__ __device__ inline uint16_t vmp_pmm_pack(T v, bool seen, int *bad)
{
    return vmp_pmm_pack_i64((int64_t)v, seen, bad);
}

// entry e of an array by the dtype code of the pack entry points (0 double, 1 int64, 2 uint8,
// otherwise int32)
__host__ __device__ inline uint16_t vmp_pmm_pack_at(int dtype, const void *x, int64_t e, bool seen,
                                                    int *bad)
{
    switch (dtype) {
    case 0: return vmp_pmm_pack(((const double *)x)[e], seen, bad);
    case 1: return vmp_pmm_pack(((const int64_t *)x)[e], seen, bad);
    case 2: return vmp_pmm_pack(((const uint8_t *)x)[e], seen, bad);
    default: return vmp_pmm_pack(((const int32_t *)x)[e], seen, bad);
    }
}

// lgamma(x + 1) of a packed count; exactly zero for 0, 1 and a hidden entry.  Up to 20 the
// factorial is an exact integer and its logarithm is rounded once; above, vmp_lgamma_dd.
__host__ __device__ inline double vmp_pmm_lgamma1(uint16_t p)
{
    if (p == VMP_PMM_HIDDEN || p < 2) return 0.0;
    if (p <= 20) {
        uint64_t f = 2;
        for (uint64_t i = 3; i <= p; ++i) f *= i;
        return log((double)f);                      // 20! < 2^62; exact in a double up to 18!
    }
    double lo;
    return vmp_lgamma_dd((double)p + 1.0, 0.0, &lo);
}

// one addition of a long sum: *s += v with the rounding error of the addition added to *e
__host__ __device__ inline void vmp_pmm_sum_add(double *s, double *e, double v)
{
    double err;
    *s = vmp_two_sum(*s, v, &err);
    *e += err;
}

// -- the operands, from the 16 staged bits ------------------------------------------------------------
__host__ __device__ inline bool vmp_pmm_observed(uint16_t p) { return p != VMP_PMM_HIDDEN; }

// the form without hidden entries converts and nothing else
__host__ __device__ inline double vmp_pmm_count(uint16_t p) { return (double)p; }

__host__ __device__ inline double vmp_pmm_masked_count(uint16_t p)
{
    return vmp_pmm_observed(p) ? (double)p : 0.0;
}

__host__ __device__ inline double vmp_pmm_mask_value(uint16_t p)
{
    return vmp_pmm_observed(p) ? 1.0 : 0.0;
}

// -- the tables ---------------------------------------------------------------------------------------
// the B operand of the second product of the hidden form
__host__ __device__ inline double vmp_pmm_neg(double lb) { return -lb; }

__host__ __device__ inline double vmp_pmm_c_raw(double elog_pi, double lsum, int form)
{
    return (form & VMP_PMM_FORM_HIDDEN) ? elog_pi : elog_pi - lsum;
}

// an entry of a table of the pass: column 0 of its row taken out where the form says so
__host__ __device__ inline double vmp_pmm_table(double v, double v0, int form)
{
    return (form & VMP_PMM_FORM_CENTRE) ? v - v0 : v;
}

// -- the pass: one step of a product, the softmax (the functions of vmp_dgmm_dev.h but for r) ----------
__host__ __device__ inline double vmp_pmm_mac(double acc, double a, double b) { return acc + a * b; }

// r_k from e = exp(l_k - m) and the sum s of the row's e
__host__ __device__ inline double vmp_pmm_resp(double e, double s) { return e / s; }

// scal[2] of the hidden form from its two dot products
__host__ __device__ inline double vmp_pmm_dots(double s_l, double m_lb) { return s_l - m_lb; }

// -- the update (gamma.py, expfamily.py:400-480 for the bound term) -----------------------------------
// q(lam_dk) = Gamma(a, b) with a = a0 + s, b = b0 + cnt: par = (a, b), mom = (<lam>, <log lam>).
// Returns <log p(lam)> - <log q(lam)> = a0 (log b0 - log b) - lgamma(a0) + lgamma(a) + (a0 - a) psi(a)
// + a - b0 a / b in the form of vmp_dgmm_masked_update_tau: a - a0 = s and b - b0 = cnt are kept as
// they are.  lgamma(a) - lgamma(a0) - s psi(a) is vmp_dgmm_lgamma_diff with s psi(a) taken into it
// term by term (vmp_pmm_lgamma_psi_diff): s runs to 1e8 here, and s log(a + 16) and s psi(a), each
// with the error of its function times s, differ by s / (2 a) only.  Exactly zero at s = cnt = 0,
// where q is the prior.
//
// lgamma(a0 + s) - lgamma(a0) - s psi(a0 + s), s >= 0: with y0 = a0 + 16, y1 = y0 + s and
// psi(a) = psi(y1) - sum_{i < 16} 1 / (a + i), log y1 - psi(y1) = 1 / (2 y1) + 1 / (12 y1^2) - ...
__host__ __device__ inline double vmp_pmm_lgamma_psi_diff(double a0, double s)
{
    const double a = a0 + s, y0 = a0 + 16.0, y1 = y0 + s;
    double logs = 0.0, lost = 0.0, recip = 0.0;
    for (int i = 0; i < 16; ++i) {
        const double v = log1p(s / (a0 + i)), t = logs + v;
        lost += (logs >= v) ? (logs - t) + v : (v - t) + logs;
        logs = t;
        recip += 1.0 / (a + i);
    }
    const double inv = 1.0 / y1, inv2 = inv * inv;
    const double gap = 0.5 * inv + inv2 * (1.0 / 12 - inv2 * (1.0 / 120 - inv2 * (1.0 / 252 - inv2 * (1.0 / 240 - inv2 * (1.0 / 132 - inv2 * (691.0 / 32760 - inv2 * (1.0 / 12)))))));
    const double st = (y0 - 0.5) * log1p(s / y0) - s
                      + (vmp_dgmm_stirling_tail(y1) - vmp_dgmm_stirling_tail(y0));
    return ((st - logs) - lost) + s * (gap + recip);
}

// q = Gamma(a, b) that stands s = a - a0 and cnt = b - b0 away from its prior: par, mom and the
// bound term.  The update has s and cnt as they are; a natural-gradient step (vmp_mix_svi.hip) forms
// them from the stepped parameters.
__host__ __device__ inline double vmp_pmm_lam_state(double a0, double b0, double a, double b,
                                                    double s, double cnt, double *par, double *mom)
{
    const double psi = vmp_digamma(a), lam = a / b;
    par[0] = a;
    par[1] = b;
    mom[0] = lam;
    mom[1] = psi - log(b);
    return -a0 * log1p(cnt / b0) + vmp_pmm_lgamma_psi_diff(a0, s) + cnt * lam;
}

__host__ __device__ inline double vmp_pmm_update_lam(double a0, double b0, double s, double cnt,
                                                     double *par, double *mom)
{
    return vmp_pmm_lam_state(a0, b0, a0 + s, b0 + cnt, s, cnt, par, mom);
}
