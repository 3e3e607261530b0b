// vmp_binm.hip -- the pack, the tables and the plate pass of the fused binomial-mixture block
//
//     R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
//     P = Beta(a0, plates=(D, K));  X = Mixture(Z, Binomial, n, P);  X.observe(x[, mask=m])
//
// (the reference forms the (N, D, K) broadcast of the log-density and an (N, D, K, 2) message to P,
// mixture.py / binomial.py / beta.py).  One pass over the rows leaves the sufficient statistics only
// (vmp_binm_dev.h), with l1 = <log p> - <log(1-p)>, l0 = <log(1-p)>:
//
//   per tile of 64 rows   logit = Xt l1 + Nt l0 + c
//                         lse, r = exp(logit - lse)                 (r goes to LDS, never to memory)
//                         N_k += sum r, sum lse                     (rows with an observed entry)
//                         S += r^T Xt,  T += r^T Nt
//
// All products run on v_mfma_f64_16x16x4_f64 (operand layout: vmp_dgmm.hip).  The counts and the
// trials are 16 bits per entry each; the two tiles of a column block are staged in LDS as they are
// and become doubles, selected against 0xFFFF of the trials, when an operand is formed.  D is walked
// in column blocks of 64: 32 accumulator tiles at K = 64, eight per wavefront, held twice -- 128
// registers, as in the hidden form of vmp_pmm.hip, whose walk over the blocks, staging stride and
// partial layout this kernel keeps.  When the trials are constant along the rows and nothing is
// hidden, vmp_binm_pass runs the Poisson pass itself on the plane of counts (vmp_binm_dev.h).
//
// No floating-point atomics: a workgroup owns a chunk of consecutive rows and leaves one partial;
// binm_combine_kernel adds the partials in chunk order.
#include "vmp_common.h"
#include "vmp_binm_dev.h"

namespace {

constexpr int NT = VMP_PMM_NT;

struct BinmArgs {
    int64_t N, chunk;
    int D, K;
    const uint16_t *x, *n;     // N x D each, packed
    const int32_t *labels;     // fixed classes (r = one-hot, lse = 0) or null
    const double *l1, *l0;     // D x K
    const double *c;           // K
    double *part;              // chunks x vmp_pmm_partial_doubles(D, K, 1)
    double *dots;              // chunks: sum over the rows of r . (logit - c)
    double *r_out;             // N x K or null
};

template <int KT>
__global__ void __launch_bounds__(NT) binm_pass_kernel(BinmArgs a)
{
    constexpr int KP = KT * 16;
    constexpr int DB = VMP_BINM_DBLOCK;
    constexpr int STR = DB + 2;                      // halfwords of a staged row
    constexpr int NH = 2 * KT * (DB / 16) / 4;       // (column, statistic, k) tiles per wavefront
    __shared__ __attribute__((aligned(8))) uint16_t x_s[VMP_PMM_TILE * STR];
    __shared__ __attribute__((aligned(8))) uint16_t n_s[VMP_PMM_TILE * STR];
    __shared__ double r_s[VMP_PMM_TILE * KP];        // responsibilities of the tile, row-major
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int D = a.D, K = a.K;
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t r1 = (r0 + a.chunk < a.N) ? r0 + a.chunk : a.N;
    double *part = a.part + (int64_t)blockIdx.x * vmp_pmm_partial_doubles(D, K, 1);
    const int64_t DK = (int64_t)D * K;
    const int nblk = (D + DB - 1) / DB;
    const bool soft = a.labels == nullptr;

    double cval[KT], nk[KT];
#pragma unroll
    for (int kb = 0; kb < KT; ++kb) {
        const int k = kb * 16 + l15;
        cval[kb] = k < K ? a.c[k] : -INFINITY;
        nk[kb] = 0.0;
    }
    double lsum = 0.0, dsum = 0.0;
    v4f64 acc[NH];                                   // the chunk's running sums
#pragma unroll
    for (int j = 0; j < NH; ++j) acc[j] = v4f64{0.0, 0.0, 0.0, 0.0};

    // rows row0 .. of columns d0 .. d0 + DB - 1 of both planes into LDS; beyond the chunk and
    // beyond D a hidden entry (count 0, trials 0xFFFF)
    auto load_planes = [&](int64_t row0, int d0) {
        for (int i = tid; i < VMP_PMM_TILE * DB; i += NT) {
            const int t = i / DB, j = i % DB;
            const int64_t row = row0 + t;
            const int d = d0 + j;
            const bool in = row < r1 && d < D;
            const int64_t e = row * D + d;
            x_s[t * STR + j] = in ? a.x[e] : (uint16_t)0;
            n_s[t * STR + j] = in ? a.n[e] : (uint16_t)VMP_BINM_HIDDEN;
        }
    };

    for (int64_t row0 = r0; row0 < r1; row0 += VMP_PMM_TILE) {
        // -- logits of this wavefront's 16 rows, block after block; `seen` counts the observed
        // entries this lane met in its row (16 wave + l15)
        v4f64 lg[KT];
#pragma unroll
        for (int kb = 0; kb < KT; ++kb) lg[kb] = v4f64{0.0, 0.0, 0.0, 0.0};
        int seen = 0;
        for (int blk = 0; blk < nblk; ++blk) {
            const int d0 = blk * DB;
            if (blk > 0) __syncthreads();            // the block before has been read
            load_planes(row0, d0);
            __syncthreads();
            const int cols = (D - d0 < DB) ? D - d0 : DB;
            const int steps = (cols + 3) >> 2;
            for (int s = 0; s < steps; ++s) {
                const int j = 4 * s + l4, d = d0 + j;
                const uint16_t xp = x_s[(wave * 16 + l15) * STR + j];
                const uint16_t np = n_s[(wave * 16 + l15) * STR + j];
                seen += vmp_binm_observed(np) ? 1 : 0;
                if (!soft) continue;
                const double ax = vmp_binm_count(xp, np);
                const double an = vmp_binm_trials(np);
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) {
                    const int k = kb * 16 + l15;
                    const bool in = d < D && k < K;
                    const double b1 = in ? a.l1[(int64_t)d * K + k] : 0.0;
                    const double b0 = in ? a.l0[(int64_t)d * K + k] : 0.0;
                    lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(ax, b1, lg[kb], 0, 0, 0);
                    lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(an, b0, lg[kb], 0, 0, 0);
                }
            }
        }
        seen += __shfl_xor(seen, 16);                // the four lanes of a row add their counts
        seen += __shfl_xor(seen, 32);
        // -- softmax over the row; the constant of the column comes last, as one addition (-inf for
        // the padding), lg itself stays as it is for the row's part of scal[2]:: lane (l4, qq) holds columns l15, l15 + 16, ... of row l4 + 4 qq
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int t = wave * 16 + l4 + 4 * qq;
            const int64_t row = row0 + t;
            const bool valid = row < r1;
            const bool obs = __shfl(seen, l4 + 4 * qq) > 0;      // lane l15 = l4 + 4 qq has the row
            double lse = 0.0, s = 1.0, ex[KT];
            int lab = -1;
            if (soft) {
                double m = vmp_dgmm_logit_finish(lg[0][qq], cval[0]);
#pragma unroll
                for (int kb = 1; kb < KT; ++kb)
                    m = fmax(m, vmp_dgmm_logit_finish(lg[kb][qq], cval[kb]));
                m = group16_max(m);
                s = 0.0;
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) {
                    ex[kb] = vmp_dgmm_shifted_exp(vmp_dgmm_logit_finish(lg[kb][qq], cval[kb]), m);
                    s += ex[kb];
                }
                s = group16_sum(s);
                lse = vmp_dgmm_lse(m, s);
            } else if (valid) {
                lab = a.labels[row];
            }
            double rd = 0.0;                         // r . (logit - c) of the row, this lane's columns
#pragma unroll
            for (int kb = 0; kb < KT; ++kb) {
                const int k = kb * 16 + l15;
                double rv = 0.0;
                if (valid) rv = soft ? vmp_pmm_resp(ex[kb], s) : (k == lab ? 1.0 : 0.0);
                r_s[t * KP + k] = rv;
                if (obs) nk[kb] += rv;
                if (soft) rd = vmp_pmm_mac(rd, rv, lg[kb][qq]);
                if (a.r_out && valid && k < K) a.r_out[row * K + k] = rv;
            }
            if (soft) rd = group16_sum(rd);
            if (valid && obs) {
                lsum += lse;
                dsum += rd;
            }
        }
        __syncthreads();

        // -- (S, T) += r^T (Xt, Nt), block after block.  Tile tl of a block is (column tile ct,
        // statistic st, cluster tile kb) = (tl / (2 KT), (tl / KT) % 2, tl % KT), dealt out to the
        // wavefronts; the sums of the tile of rows start at zero and are added to the chunk's
        // running sums once per tile (vmp_pmm_dev.h).
        for (int blk = 0; blk < nblk; ++blk) {
            const int d0 = blk * DB;
            if (nblk > 1) {
                __syncthreads();                     // what the planes held has been read
                load_planes(row0, d0);
                __syncthreads();
            }
            const int cols = (D - d0 < DB) ? D - d0 : DB;
            const int ntile = 2 * KT * ((cols + 15) >> 4);
            v4f64 tacc[NH];
#pragma unroll
            for (int j = 0; j < NH; ++j) tacc[j] = v4f64{0.0, 0.0, 0.0, 0.0};
            if (nblk > 1) {
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int tl = wave + 4 * j;
                    if (tl >= ntile) continue;
                    const int kb = tl % KT, st = (tl / KT) % 2;
                    const int d = d0 + (tl / (2 * KT)) * 16 + l15;
                    const int64_t po = st * DK;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int k = kb * 16 + l4 + 4 * qq;
                        acc[j][qq] = (row0 > r0 && k < K && d < D) ? part[po + (int64_t)k * D + d]
                                                                   : 0.0;
                    }
                }
            }
            for (int s = 0; s < 16; ++s) {
                const int t = 4 * s + l4;
                const double *rrow = r_s + t * KP;
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int tl = wave + 4 * j;
                    if (tl >= ntile) continue;
                    const int kb = tl % KT, st = (tl / KT) % 2;
                    const int jc = (tl / (2 * KT)) * 16 + l15;
                    const double av = rrow[kb * 16 + l15];
                    const uint16_t xp = x_s[t * STR + jc], np = n_s[t * STR + jc];
                    const double bv = st == 0 ? vmp_binm_count(xp, np) : vmp_binm_trials(np);
                    tacc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, tacc[j], 0, 0, 0);
                }
            }
#pragma unroll
            for (int j = 0; j < NH; ++j)
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) acc[j][qq] += tacc[j][qq];
            if (nblk > 1 || row0 + VMP_PMM_TILE >= r1) {
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int tl = wave + 4 * j;
                    if (tl >= ntile) continue;
                    const int kb = tl % KT, st = (tl / KT) % 2;
                    const int d = d0 + (tl / (2 * KT)) * 16 + l15;
                    const int64_t po = st * DK;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int k = kb * 16 + l4 + 4 * qq;
                        if (k < K && d < D) part[po + (int64_t)k * D + d] = acc[j][qq];
                    }
                }
            }
        }
        __syncthreads();                 // r_s and the planes are free for the next tile
    }

    // -- N_k and sum lse: the 16 slots in slot order (they stand in r_s, which is free now) ------
    double *nk_s = r_s, *lse_s = r_s + 16 * KP, *dot_s = lse_s + 16;
#pragma unroll
    for (int kb = 0; kb < KT; ++kb) nk_s[(wave * 4 + l4) * KP + kb * 16 + l15] = nk[kb];
    if (l15 == 0) {
        lse_s[wave * 4 + l4] = lsum;
        dot_s[wave * 4 + l4] = dsum;
    }
    __syncthreads();
    if (tid < K) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += nk_s[s * KP + tid];
        part[2 * DK + tid] = t;
    }
    if (tid == 0) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += lse_s[s];
        part[2 * DK + K] = t;
        double u = 0.0;
        for (int s = 0; s < 16; ++s) u += dot_s[s];
        a.dots[blockIdx.x] = u;
    }
}

// one thread per (k, d): the partials in chunk order, then the message to P; `dots` (the chunks'
// parts of scal[2]) null: scal[2] is left to binm_dots_kernel
__global__ void __launch_bounds__(NT)
binm_combine_kernel(int64_t nc, int D, int K, const double *__restrict__ part,
                    const double *__restrict__ dots, double *__restrict__ S, double *__restrict__ T, double *__restrict__ Nk,
                    double *__restrict__ counts, double *__restrict__ sum_lse)
{
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx >= D * K) return;
    const int k = idx / D, d = idx - k * D;
    const int64_t per = vmp_pmm_partial_doubles(D, K, 1), DK = (int64_t)D * K;
    double s = 0.0, t = 0.0;
    for (int64_t c = 0; c < nc; ++c) {
        s += part[c * per + idx];
        t += part[c * per + DK + idx];
    }
    const int64_t e = (int64_t)d * K + k;
    S[e] = s;
    T[e] = t;
    counts[2 * e] = s;
    counts[2 * e + 1] = vmp_binm_failures(t, s);
    if (d == 0) {
        double n = 0.0;
        for (int64_t c = 0; c < nc; ++c) n += part[c * per + 2 * DK + k];
        Nk[k] = n;
    }
    if (idx == 0) {
        double v = 0.0;
        for (int64_t c = 0; c < nc; ++c) v += part[c * per + 2 * DK + K];
        sum_lse[0] = v;
        if (dots) {
            double u = 0.0;
            for (int64_t c = 0; c < nc; ++c) u += dots[c];
            sum_lse[2] = u;
        }
    }
}

// one plane: T[d, k] = n_d N_k and the message to P from the S and N_k of the Poisson pass
__global__ void __launch_bounds__(NT)
binm_const_kernel(int D, int K, const double *__restrict__ ncol, const double *__restrict__ S,
                  const double *__restrict__ Nk, double *__restrict__ T,
                  double *__restrict__ counts)
{
    const int e = blockIdx.x * NT + threadIdx.x;
    if (e >= D * K) return;
    const double t = vmp_binm_t_const(ncol[e / K], Nk[e % K]), s = S[e];
    T[e] = t;
    counts[2 * (int64_t)e] = s;
    counts[2 * (int64_t)e + 1] = vmp_binm_failures(t, s);
}

// scal[2] of the two-plane form under fixed labels (no logits are formed): one workgroup, element e belongs to thread e % 256; the 256 sums
// are halved eight times (vmp_binm_dev.h)
__global__ void __launch_bounds__(NT)
binm_dots_kernel(int n, const double *__restrict__ S, const double *__restrict__ l1,
                 const double *__restrict__ T, const double *__restrict__ l0,
                 double *__restrict__ out)
{
    __shared__ double bs[NT];
    const int tid = threadIdx.x;
    double t = 0.0, te = 0.0;
    for (int e = tid; e < n; e += NT) {
        double err;
        const double v = vmp_binm_dot_term(S[e], l1[e], T[e], l0[e], &err);
        vmp_pmm_sum_add(&t, &te, v);
        te += err;
    }
    bs[tid] = t + te;
    __syncthreads();
    block_halve_sum<NT>(bs, tid);
    if (tid == 0) out[0] = bs[0];
}

// l1, l0 (each less its column 0 where the form says so), c and, with ncol, cfold
__global__ void __launch_bounds__(NT)
binm_tables_kernel(int D, int K, int form, const double *__restrict__ elog_p,
                   const double *__restrict__ elog_pi, const double *__restrict__ ncol,
                   double *__restrict__ l1, double *__restrict__ l0, double *__restrict__ c,
                   double *__restrict__ cfold)
{
    __shared__ double cs[VMP_BINM_MAX_K], fs[VMP_BINM_MAX_K];
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx < D * K) {
        const int64_t i = idx, e0 = (int64_t)(idx / K) * K;     // e0: column 0 of the row
        l1[idx] = elog_p ? vmp_binm_table(vmp_binm_l1(elog_p[2 * i], elog_p[2 * i + 1]),
                                          vmp_binm_l1(elog_p[2 * e0], elog_p[2 * e0 + 1]), form)
                         : 0.0;
        l0[idx] = elog_p ? vmp_binm_table(elog_p[2 * i + 1], elog_p[2 * e0 + 1], form) : 0.0;
    }
    if (blockIdx.x == 0) {
        const bool fold = cfold && ncol;
        if (idx < K) {
            double t = 0.0;
            if (elog_p && fold)
                for (int d = 0; d < D; ++d)
                    t = vmp_pmm_mac(t, ncol[d],
                                    vmp_binm_table(elog_p[2 * ((int64_t)d * K + idx) + 1],
                                                   elog_p[2 * ((int64_t)d * K) + 1], form));
            cs[idx] = elog_pi[idx];
            fs[idx] = elog_pi[idx] + t;
        }
        __syncthreads();
        if (idx < K) {
            double m = cs[0], mf = fs[0];
            for (int k = 1; k < K; ++k) {
                m = fmax(m, cs[k]);
                mf = fmax(mf, fs[k]);
            }
            c[idx] = cs[idx] - m;
            if (fold) cfold[idx] = fs[idx] - mf;
        }
    }
}

// block b: the elements [b span, (b + 1) span); its sum of coefficients, its number of hidden entries
// and whether any of its trials differs from row 0's of the column go to the three arrays of ws
template <typename T>
__global__ void __launch_bounds__(NT)
binm_pack_kernel(int64_t n, int D, int64_t span, const T *__restrict__ x,
                 const int64_t *__restrict__ trials, int64_t ts_n, int64_t ts_d,
                 const uint8_t *__restrict__ mask, uint16_t *__restrict__ xp,
                 uint16_t *__restrict__ np, int32_t *flags, double *__restrict__ lc_part,
                 int64_t *__restrict__ hid_part, int64_t *__restrict__ var_part)
{
    __shared__ double ls[NT];
    __shared__ int hs[NT], vs[NT];
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * span;
    double lc = 0.0, lce = 0.0;
    int hid = 0, bad = 0, var = 0;
    for (int64_t i = tid; i < span; i += NT) {
        const int64_t e = e0 + i;
        if (e >= n) break;
        const int64_t row = e / D, d = e - row * D;
        const int64_t tn = trials[row * ts_n + d * ts_d];
        var |= tn != trials[d * ts_d] ? 1 : 0;
        const bool seen = mask ? mask[e] != 0 : true;
        uint16_t xo, no;
        vmp_binm_pack(x[e], tn, seen, &xo, &no, &bad);
        xp[e] = xo;
        np[e] = no;
        vmp_pmm_sum_add(&lc, &lce, vmp_binm_lchoose(xo, no));
        hid += vmp_binm_observed(no) ? 0 : 1;
    }
    if (bad & VMP_BINM_BAD_NEGATIVE) flags[0] = 1;
    if (bad & VMP_BINM_BAD_FRACTION) flags[1] = 1;
    if (bad & VMP_BINM_BAD_ABOVE) flags[2] = 1;
    if (bad & VMP_BINM_BAD_TRIALS) flags[3] = 1;
    ls[tid] = lc + lce;
    hs[tid] = hid;
    vs[tid] = var;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (tid < off) {
            ls[tid] += ls[tid + off];
            hs[tid] += hs[tid + off];
            vs[tid] |= vs[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        lc_part[blockIdx.x] = ls[0];
        hid_part[blockIdx.x] = hs[0];
        var_part[blockIdx.x] = vs[0];
    }
}

// the blocks' partials in block order
__global__ void binm_pack_finish_kernel(int64_t n, int64_t nb, const double *__restrict__ lc_part,
                                        const int64_t *__restrict__ hid_part,
                                        const int64_t *__restrict__ var_part,
                                        int64_t *__restrict__ counts, double *__restrict__ lcoef)
{
    double t = 0.0, te = 0.0;
    int64_t h = 0, v = 0;
    for (int64_t b = 0; b < nb; ++b) {
        vmp_pmm_sum_add(&t, &te, lc_part[b]);
        h += hid_part[b];
        v |= var_part[b];
    }
    counts[0] = n - h;
    counts[1] = h;
    counts[2] = v ? 0 : 1;
    lcoef[0] = t + te;
}

template <typename T>
void launch_pack(vmp_ctx *ctx, int64_t n, int D, const void *x, const int64_t *trials,
                 int64_t ts_n, int64_t ts_d, const uint8_t *mask, uint16_t *xp, uint16_t *np,
                 int32_t *flags, double *ws)
{
    hipLaunchKernelGGL(binm_pack_kernel<T>, dim3((unsigned)vmp_pmm_pack_blocks(n)), dim3(NT), 0,
                       ctx->stream, n, D, vmp_pmm_pack_span(n), (const T *)x, trials, ts_n, ts_d,
                       mask, xp, np, flags, ws, (int64_t *)(ws + VMP_PMM_PACK_BLOCKS),
                       (int64_t *)(ws + 2 * VMP_PMM_PACK_BLOCKS));
}

}  // namespace

#define BINM_SHAPE(ctx, D, K)                                                                     \
    VMP_REQUIRE(ctx, K <= VMP_BINM_MAX_K && D <= VMP_BINM_MAX_D, VMP_ERR_UNSUPPORTED,             \
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_BINM_MAX_D, VMP_BINM_MAX_K)

extern "C" {

int32_t vmp_binm_limits(int32_t *max_K, int32_t *max_D, int32_t *max_trials)
{
    if (!max_K || !max_D || !max_trials) return VMP_ERR_INVALID;
    *max_K = VMP_BINM_MAX_K;
    *max_D = VMP_BINM_MAX_D;
    *max_trials = VMP_BINM_MAX_TRIALS;
    return VMP_OK;
}

int32_t vmp_binm_plan(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                      int64_t *workspace_doubles)
{
    if (N < 0 || D < 1 || K < 1) return VMP_ERR_INVALID;
    if (K > VMP_BINM_MAX_K || D > VMP_BINM_MAX_D) return VMP_ERR_UNSUPPORTED;
    if (!chunk_rows || !workspace_doubles) return VMP_ERR_INVALID;
    *chunk_rows = vmp_pmm_chunk_rows(N, D, K);
    *workspace_doubles = vmp_binm_workspace_doubles(N, D, K);
    return VMP_OK;
}

int32_t vmp_binm_pack(vmp_ctx *ctx, int64_t N, int32_t D, int32_t dtype, const void *x,
                      const int64_t *trials, int64_t trials_stride_n, int64_t trials_stride_d,
                      const uint8_t *mask, uint16_t *x_packed, uint16_t *n_packed, int32_t *flags,
                      int64_t *counts, double *lcoef, double *ws)
{
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && dtype >= 0 && dtype <= 3 && trials_stride_n >= 0
                && trials_stride_d >= 0, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, D <= VMP_BINM_MAX_D, VMP_ERR_UNSUPPORTED, "D = %d exceeds the limit %d", D,
                VMP_BINM_MAX_D);
    VMP_REQUIRE(ctx, flags && counts && lcoef && ws
                && (N == 0 || (x && trials && x_packed && n_packed)), VMP_ERR_INVALID,
                "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int64_t n = N * D;
    if (n > 0) {
        switch (dtype) {
        case 0:
            launch_pack<double>(ctx, n, D, x, trials, trials_stride_n, trials_stride_d, mask,
                                x_packed, n_packed, flags, ws);
            break;
        case 1:
            launch_pack<int64_t>(ctx, n, D, x, trials, trials_stride_n, trials_stride_d, mask,
                                 x_packed, n_packed, flags, ws);
            break;
        case 2:
            launch_pack<uint8_t>(ctx, n, D, x, trials, trials_stride_n, trials_stride_d, mask,
                                 x_packed, n_packed, flags, ws);
            break;
        default:
            launch_pack<int32_t>(ctx, n, D, x, trials, trials_stride_n, trials_stride_d, mask,
                                 x_packed, n_packed, flags, ws);
            break;
        }
        VMP_HIP_CHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(binm_pack_finish_kernel, dim3(1), dim3(1), 0, ctx->stream, n,
                       n > 0 ? vmp_pmm_pack_blocks(n) : 0, ws,
                       (const int64_t *)(ws + VMP_PMM_PACK_BLOCKS),
                       (const int64_t *)(ws + 2 * VMP_PMM_PACK_BLOCKS), counts, lcoef);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_binm_tables(vmp_ctx *ctx, int32_t D, int32_t K, int32_t form, const double *elog_p,
                        const double *elog_pi, const double *ncol, double *l1, double *l0,
                        double *c, double *cfold)
{
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1 && (form == 0 || form == 1), VMP_ERR_INVALID,
                "bad arguments");
    BINM_SHAPE(ctx, D, K);
    VMP_REQUIRE(ctx, elog_pi && l1 && l0 && c, VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    hipLaunchKernelGGL(binm_tables_kernel, dim3((unsigned)((D * K + NT - 1) / NT)), dim3(NT), 0,
                       ctx->stream, D, K, form, elog_p, elog_pi, ncol, l1, l0, c, cfold);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_binm_pass(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, int32_t one_plane,
                      const uint16_t *x_packed, const uint16_t *n_packed, const double *ncol,
                      const int32_t *labels, const double *l1, const double *l0, const double *c,
                      double *ws, double *S, double *T, double *Nk, double *counts, double *scal,
                      double *r_out)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && K >= 1 && (one_plane == 0 || one_plane == 1),
                VMP_ERR_INVALID, "bad arguments");
    BINM_SHAPE(ctx, D, K);
    VMP_REQUIRE(ctx, l1 && l0 && c && ws && S && T && Nk && counts && scal
                && (one_plane ? ncol != nullptr : (N == 0 || n_packed))
                && (N == 0 || x_packed), VMP_ERR_INVALID, "null argument");
    const unsigned eblocks = (unsigned)((D * K + NT - 1) / NT);
    if (one_plane) {
        // the Poisson pass without hidden entries: logit = c + x l1, S = r^T x, scal[2] = S . l1
        const int32_t rc = vmp_pmm_pass(ctx, N, D, K, 0, x_packed, labels, l1, l0, c, ws, S, T, Nk,
                                        scal, r_out);
        if (rc != VMP_OK) return rc;
        hipLaunchKernelGGL(binm_const_kernel, dim3(eblocks), dim3(NT), 0, ctx->stream, D, K, ncol,
                           S, Nk, T, counts);
        VMP_HIP_CHECK(ctx, hipGetLastError());
        return VMP_OK;
    }
    VMP_FLUSH_SMALL(ctx);
    const int64_t nc = vmp_pmm_chunks(N, D, K);
    // behind the partials: the chunks' parts of scal[2] (at most VMP_PMM_MAX_CHUNKS = 1024), read by
    // the combine before vmp_lda_dot takes the same doubles for its partial sums
    double *dot_ws = ws + nc * vmp_pmm_partial_doubles(D, K, 1);
    if (nc > 0) {
        BinmArgs a = {N, vmp_pmm_chunk_rows(N, D, K), D, K, x_packed, n_packed, labels, l1, l0, c,
                      ws, dot_ws, r_out};
        const dim3 grid((unsigned)nc), block(NT);
        switch (vmp_pmm_kpad(K) / 16) {
        case 1: hipLaunchKernelGGL(binm_pass_kernel<1>, grid, block, 0, ctx->stream, a); break;
        case 2: hipLaunchKernelGGL(binm_pass_kernel<2>, grid, block, 0, ctx->stream, a); break;
        case 3: hipLaunchKernelGGL(binm_pass_kernel<3>, grid, block, 0, ctx->stream, a); break;
        default: hipLaunchKernelGGL(binm_pass_kernel<4>, grid, block, 0, ctx->stream, a); break;
        }
        VMP_HIP_CHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(binm_combine_kernel, dim3(eblocks), dim3(NT), 0, ctx->stream, nc, D, K, ws,
                       labels ? nullptr : dot_ws, S, T, Nk, counts, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    const int32_t rc = vmp_lda_dot(ctx, K, Nk, c, dot_ws, scal + 1);
    if (rc != VMP_OK) return rc;
    if (labels) {
        hipLaunchKernelGGL(binm_dots_kernel, dim3(1), dim3(NT), 0, ctx->stream, D * K, S, l1, T, l0,
                           scal + 2);
        VMP_HIP_CHECK(ctx, hipGetLastError());
    }
    return VMP_OK;
}

}  // extern "C"
