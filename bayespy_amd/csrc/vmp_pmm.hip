// vmp_pmm.hip -- the pack, the plate pass and the update of the fused Poisson-mixture block
//
//     R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
//     lam = Gamma(a0, b0, plates=(D, K));  X = Mixture(Z, Poisson, lam);  X.observe(x[, mask=m])
//
// (the reference forms the (N, D, K) broadcast of the log-density and two (N, D, K) messages to lam,
// mixture.py / poisson.py / gamma.py).  One pass over the rows leaves the sufficient statistics only
// (vmp_pmm_dev.h), with l = <log lam>, lb = <lam>:
//
//   per tile of 64 rows   logit = X l + c             or   Xt l + M (-lb) + c     (hidden entries)
//                         lse, r = exp(logit - lse)                 (r goes to LDS, never to memory)
//                         N_k += sum r, sum lse                     (rows with an observed entry)
//                         S += r^T X                   or   S += r^T Xt,  M += r^T M
//
// All products run on v_mfma_f64_16x16x4_f64 (operand layout: vmp_dgmm.hip).  x is 16 bits per
// entry; the tile of a column block is staged in LDS as it is and becomes a double, selected
// against 0xFFFF in the hidden form, when an operand is formed.  The pass reads no other array of
// size N D.
//
// D is walked in COLUMN BLOCKS: 128 columns with one statistic, 64 with two -- either way
// 32 accumulator tiles at K = 64, eight per wavefront, held twice (the sums of the present tile of
// 64 rows and the chunk's running sums): 128 registers.  With one block its x tile stays in LDS
// between the two products and the running sums live in registers through the chunk.  Above, the
// logits walk the blocks first, the second product walks them again (from L2) and each block's
// running sums are carried through the chunk's partial in memory.
//
// A row of the staged tile is DBLOCK + 2 halfwords: 65 (33) dwords, so the 16 rows of an A read
// and the 4 rows of a B read fall on different banks.
//
// No floating-point atomics: a workgroup owns a chunk of consecutive rows and leaves one partial;
// pmm_combine_kernel adds the partials in chunk order.
#include "vmp_common.h"
#include "vmp_pmm_dev.h"

namespace {

constexpr int NT = VMP_PMM_NT;

// PmmArgs: vmp_common.h
template <int KT, bool HIDDEN>
__global__ void __launch_bounds__(NT) pmm_pass_kernel(PmmArgs a)
{
    constexpr int KP = KT * 16;
    constexpr int DB = HIDDEN ? VMP_PMM_DBLOCK_HIDDEN : VMP_PMM_DBLOCK;
    constexpr int STR = DB + 2;                      // halfwords of a staged row
    constexpr int NS = HIDDEN ? 2 : 1;               // statistics
    constexpr int NH = NS * KT * (DB / 16) / 4;      // (column, statistic, k) tiles per wavefront
    constexpr uint16_t PAD = HIDDEN ? (uint16_t)VMP_PMM_HIDDEN : (uint16_t)0;
    __shared__ __attribute__((aligned(8))) uint16_t x_s[VMP_PMM_TILE * STR];
    __shared__ double r_s[VMP_PMM_TILE * KP];        // responsibilities of the tile, row-major
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int D = a.D, K = a.K;
    const int64_t r0 = (int64_t)blockIdx.x * a.chunk;
    const int64_t r1 = (r0 + a.chunk < a.N) ? r0 + a.chunk : a.N;
    double *part = a.part + (int64_t)blockIdx.x * vmp_pmm_partial_doubles(D, K, HIDDEN);
    const int64_t DK = (int64_t)D * K;
    const int nblk = (D + DB - 1) / DB;
    const bool soft = a.labels == nullptr;
    const bool x8 = ((uintptr_t)a.x & 7) == 0;

    double cval[KT], nk[KT];
#pragma unroll
    for (int kb = 0; kb < KT; ++kb) {
        const int k = kb * 16 + l15;
        cval[kb] = k < K ? a.c[k] : -INFINITY;
        nk[kb] = 0.0;
    }
    double lsum = 0.0;
    v4f64 acc[NH];                                   // the chunk's running sums
#pragma unroll
    for (int j = 0; j < NH; ++j) acc[j] = v4f64{0.0, 0.0, 0.0, 0.0};

    // rows row0 .. of columns d0 .. d0 + DB - 1 into x_s, four halfwords per thread and step;
    // PAD beyond the chunk and beyond D
    auto load_x = [&](int64_t row0, int d0) {
        for (int i = tid; i < VMP_PMM_TILE * (DB / 4); i += NT) {
            const int t = i / (DB / 4), j = 4 * (i % (DB / 4));
            const int64_t row = row0 + t;
            const int d = d0 + j;
            const int64_t e = row * D + d;
            uint32_t lo, hi;
            if (row < r1 && d + 3 < D && x8 && (e & 3) == 0) {
                const uint64_t v = *(const uint64_t *)(a.x + e);
                lo = (uint32_t)v;
                hi = (uint32_t)(v >> 32);
            } else {
                uint32_t h[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) h[b] = (row < r1 && d + b < D) ? a.x[e + b] : PAD;
                lo = h[0] | (h[1] << 16);
                hi = h[2] | (h[3] << 16);
            }
            uint32_t *dst = (uint32_t *)(x_s + t * STR + j);
            dst[0] = lo;
            dst[1] = hi;
        }
    };

    for (int64_t row0 = r0; row0 < r1; row0 += VMP_PMM_TILE) {
        // -- logits of this wavefront's 16 rows, block after block; `seen` counts the observed
        // entries this lane met in its row (16 wave + l15)
        v4f64 lg[KT];
#pragma unroll
        for (int kb = 0; kb < KT; ++kb) lg[kb] = v4f64{0.0, 0.0, 0.0, 0.0};
        int seen = 0;
        if (soft || HIDDEN || nblk == 1) {
            for (int blk = 0; blk < nblk; ++blk) {
                const int d0 = blk * DB;
                if (blk > 0) __syncthreads();        // the block before has been read
                load_x(row0, d0);
                __syncthreads();
                if (!soft && !HIDDEN) continue;
                const int cols = (D - d0 < DB) ? D - d0 : DB;
                const int steps = (cols + 3) >> 2;
                for (int s = 0; s < steps; ++s) {
                    const int j = 4 * s + l4, d = d0 + j;
                    const uint16_t p = x_s[(wave * 16 + l15) * STR + j];
                    if (HIDDEN) seen += vmp_pmm_observed(p) ? 1 : 0;
                    if (!soft) continue;
                    const double av = HIDDEN ? vmp_pmm_masked_count(p) : vmp_pmm_count(p);
                    const double am = vmp_pmm_mask_value(p);
#pragma unroll
                    for (int kb = 0; kb < KT; ++kb) {
                        const int k = kb * 16 + l15;
                        const bool in = d < D && k < K;
                        const double bl = in ? a.l[(int64_t)d * K + k] : 0.0;
                        lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bl, lg[kb], 0, 0, 0);
                        if (HIDDEN) {
                            const double bb = in ? vmp_pmm_neg(a.lb[(int64_t)d * K + k]) : 0.0;
                            lg[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, bb, lg[kb], 0, 0, 0);
                        }
                    }
                }
            }
        }
        if (HIDDEN) {                    // the four lanes of a row add their counts
            seen += __shfl_xor(seen, 16);
            seen += __shfl_xor(seen, 32);
        }
        // the constant of the column comes last, as one addition (-inf for the padding)
#pragma unroll
        for (int kb = 0; kb < KT; ++kb)
#pragma unroll
            for (int qq = 0; qq < 4; ++qq)
                lg[kb][qq] = vmp_dgmm_logit_finish(lg[kb][qq], cval[kb]);
        // -- softmax over the row: lane (l4, qq) holds columns l15, l15 + 16, ... of row l4 + 4 qq
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            const int t = wave * 16 + l4 + 4 * qq;
            const int64_t row = row0 + t;
            const bool valid = row < r1;
            // lane l15 = l4 + 4 qq has the row
            const bool obs = HIDDEN ? __shfl(seen, l4 + 4 * qq) > 0 : true;
            double lse = 0.0, s = 1.0, ex[KT];
            int lab = -1;
            if (soft) {
                double m = lg[0][qq];
#pragma unroll
                for (int kb = 1; kb < KT; ++kb) m = fmax(m, lg[kb][qq]);
                m = group16_max(m);
                s = 0.0;
#pragma unroll
                for (int kb = 0; kb < KT; ++kb) {
                    ex[kb] = vmp_dgmm_shifted_exp(lg[kb][qq], m);
                    s += ex[kb];
                }
                s = group16_sum(s);
                lse = vmp_dgmm_lse(m, s);
            } else if (valid) {
                lab = a.labels[row];
            }
#pragma unroll
            for (int kb = 0; kb < KT; ++kb) {
                const int k = kb * 16 + l15;
                double rv = 0.0;
                if (valid) rv = soft ? vmp_pmm_resp(ex[kb], s) : (k == lab ? 1.0 : 0.0);
                r_s[t * KP + k] = rv;
                if (obs) nk[kb] += rv;
                if (a.r_out && valid && k < K) a.r_out[row * K + k] = rv;
            }
            if (valid && obs) lsum += lse;
        }
        __syncthreads();

        // -- (S, M) += r^T (Xt, M), block after block.  Tile tl of a block is (column tile ct,
        // statistic st, cluster tile kb) = (tl / (NS KT), (tl / KT) % NS, tl % KT), dealt out to the
        // wavefronts; the sums of the tile of rows start at zero and are added to the chunk's
        // running sums once per tile (vmp_pmm_dev.h).
        for (int blk = 0; blk < nblk; ++blk) {
            const int d0 = blk * DB;
            if (nblk > 1) {
                __syncthreads();                     // what x_s held has been read
                load_x(row0, d0);
                __syncthreads();
            }
            const int cols = (D - d0 < DB) ? D - d0 : DB;
            const int ntile = NS * KT * ((cols + 15) >> 4);
            v4f64 tacc[NH];
#pragma unroll
            for (int j = 0; j < NH; ++j) tacc[j] = v4f64{0.0, 0.0, 0.0, 0.0};
            if (nblk > 1) {
#pragma unroll
                for (int j = 0; j < NH; ++j) {
                    const int tl = wave + 4 * j;
                    if (tl >= ntile) continue;
                    const int kb = tl % KT, st = (tl / KT) % NS;
                    const int d = d0 + (tl / (NS * KT)) * 16 + l15;
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
                    const int kb = tl % KT, st = (tl / KT) % NS;
                    const int jc = (tl / (NS * KT)) * 16 + l15;
                    const double av = rrow[kb * 16 + l15];
                    const uint16_t p = x_s[t * STR + jc];
                    const double bv = !HIDDEN ? vmp_pmm_count(p)
                                              : (st == 0 ? vmp_pmm_masked_count(p)
                                                         : vmp_pmm_mask_value(p));
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
                    const int kb = tl % KT, st = (tl / KT) % NS;
                    const int d = d0 + (tl / (NS * KT)) * 16 + l15;
                    const int64_t po = st * DK;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int k = kb * 16 + l4 + 4 * qq;
                        if (k < K && d < D) part[po + (int64_t)k * D + d] = acc[j][qq];
                    }
                }
            }
        }
        __syncthreads();                 // r_s and x_s are free for the next tile
    }

    // -- N_k and sum lse: the 16 slots in slot order (they stand in r_s, which is free now) ------
    double *nk_s = r_s, *lse_s = r_s + 16 * KP;
#pragma unroll
    for (int kb = 0; kb < KT; ++kb) nk_s[(wave * 4 + l4) * KP + kb * 16 + l15] = nk[kb];
    if (l15 == 0) lse_s[wave * 4 + l4] = lsum;
    __syncthreads();
    if (tid < K) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += nk_s[s * KP + tid];
        part[NS * DK + tid] = t;
    }
    if (tid == 0) {
        double t = 0.0;
        for (int s = 0; s < 16; ++s) t += lse_s[s];
        part[NS * DK + K] = t;
    }
}

// one thread per (k, d): the partials in chunk order.  M null: the form without hidden entries
__global__ void __launch_bounds__(NT)
pmm_combine_kernel(int64_t nc, int D, int K, const double *__restrict__ part,
                   double *__restrict__ S, double *__restrict__ M, double *__restrict__ Nk,
                   double *__restrict__ sum_lse)
{
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx >= D * K) return;
    const int k = idx / D, d = idx - k * D;
    const int ns = M ? 2 : 1;
    const int64_t per = vmp_pmm_partial_doubles(D, K, M != nullptr), DK = (int64_t)D * K;
    double s = 0.0, m = 0.0;
    for (int64_t c = 0; c < nc; ++c) {
        s += part[c * per + idx];
        if (M) m += part[c * per + DK + idx];
    }
    const int64_t e = (int64_t)d * K + k;
    S[e] = s;
    if (M) M[e] = m;
    if (d == 0) {
        double n = 0.0;
        for (int64_t c = 0; c < nc; ++c) n += part[c * per + ns * DK + k];
        Nk[k] = n;
    }
    if (idx == 0) {
        double t = 0.0;
        for (int64_t c = 0; c < nc; ++c) t += part[c * per + ns * DK + K];
        sum_lse[0] = t;
    }
}

// scal[2] of the hidden form: S . l - M . lb from the two dot products
__global__ void pmm_sub2_kernel(const double *__restrict__ two, double *__restrict__ out)
{
    out[0] = vmp_pmm_dots(two[0], two[1]);
}

// l = <log lam>, lb = <lam>, each less its column 0 where the form says so; lsum[k] = sum_d lb[d, k]
// in ascending d; c = <log pi> (- lsum, nothing hidden) less its largest element.  lam_mom: (D K, 2) or null (no observation term)
__global__ void __launch_bounds__(NT)
pmm_tables_kernel(int D, int K, int form, const double *__restrict__ lam_mom,
                  const double *__restrict__ elog_pi, double *__restrict__ l,
                  double *__restrict__ lb, double *__restrict__ c, double *__restrict__ lsum)
{
    __shared__ double cs[VMP_PMM_MAX_K];
    const int idx = blockIdx.x * NT + threadIdx.x;
    if (idx < D * K) {
        const int64_t e0 = (int64_t)(idx / K) * K;      // column 0 of the row
        l[idx] = lam_mom ? vmp_pmm_table(lam_mom[2 * (int64_t)idx + 1], lam_mom[2 * e0 + 1], form)
                         : 0.0;
        lb[idx] = lam_mom ? vmp_pmm_table(lam_mom[2 * (int64_t)idx], lam_mom[2 * e0], form) : 0.0;
    }
    if (blockIdx.x == 0) {
        if (idx < K) {
            double t = 0.0;
            if (lam_mom)
                for (int d = 0; d < D; ++d)
                    t += vmp_pmm_table(lam_mom[2 * ((int64_t)d * K + idx)],
                                       lam_mom[2 * ((int64_t)d * K)], form);
            if (lsum) lsum[idx] = t;
            cs[idx] = vmp_pmm_c_raw(elog_pi[idx], t, form);
        }
        __syncthreads();
        if (idx < K) {
            double m = cs[0];
            for (int k = 1; k < K; ++k) m = fmax(m, cs[k]);
            c[idx] = cs[idx] - m;
        }
    }
}

// block b: the elements [b span, (b + 1) span); its sum of lgamma(x + 1) and its number of hidden
// entries go to lg_part[b] and hid_part[b]
template <typename T>
__global__ void __launch_bounds__(NT)
pmm_pack_kernel(int64_t n, int64_t span, const T *__restrict__ x, const uint8_t *__restrict__ mask,
                uint16_t *__restrict__ xp, int32_t *flags, double *__restrict__ lg_part,
                int64_t *__restrict__ hid_part)
{
    __shared__ double ls[NT];
    __shared__ int hs[NT];
    const int tid = threadIdx.x;
    const int64_t e0 = (int64_t)blockIdx.x * span;
    double lg = 0.0, lge = 0.0;
    int hid = 0, bad = 0;
    for (int64_t i = tid; i < span; i += NT) {
        const int64_t e = e0 + i;
        if (e >= n) break;
        const bool seen = mask ? mask[e] != 0 : true;
        const uint16_t p = vmp_pmm_pack(x[e], seen, &bad);
        xp[e] = p;
        vmp_pmm_sum_add(&lg, &lge, vmp_pmm_lgamma1(p));
        hid += vmp_pmm_observed(p) ? 0 : 1;
    }
    if (bad & VMP_PMM_BAD_INVALID) flags[0] = 1;
    if (bad & VMP_PMM_BAD_ABOVE) flags[1] = 1;
    if (bad & VMP_PMM_BAD_FRACTION) flags[2] = 1;
    ls[tid] = lg + lge;
    hs[tid] = hid;
    __syncthreads();
    for (int off = NT / 2; off > 0; off >>= 1) {
        if (tid < off) {
            ls[tid] += ls[tid + off];
            hs[tid] += hs[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        lg_part[blockIdx.x] = ls[0];
        hid_part[blockIdx.x] = hs[0];
    }
}

// the blocks' partials in block order
__global__ void pmm_pack_finish_kernel(int64_t n, int64_t nb, const double *__restrict__ lg_part,
                                       const int64_t *__restrict__ hid_part,
                                       int64_t *__restrict__ counts, double *__restrict__ lgam)
{
    double t = 0.0, te = 0.0;
    int64_t h = 0;
    for (int64_t b = 0; b < nb; ++b) {
        vmp_pmm_sum_add(&t, &te, lg_part[b]);
        h += hid_part[b];
    }
    counts[0] = n - h;
    counts[1] = h;
    lgam[0] = t + te;
}

// one workgroup: element e belongs to thread e % 256; the 256 sums of the bound are halved eight
// times.  per_element: cnt is M (D x K), else N_k (K).  Null statistics: the prior
__global__ void __launch_bounds__(NT)
pmm_update_kernel(int D, int K, int per_element, const double *__restrict__ prior_a,
                  const double *__restrict__ prior_b, const double *__restrict__ S,
                  const double *__restrict__ cnt, double *__restrict__ par,
                  double *__restrict__ mom, double *__restrict__ bound)
{
    __shared__ double bs[NT];
    const int tid = threadIdx.x;
    const bool stats = S && cnt;
    double t = 0.0;
    for (int e = tid; e < D * K; e += NT) {
        const double s = stats ? S[e] : 0.0;
        const double n = stats ? (per_element ? cnt[e] : cnt[e % K]) : 0.0;
        t += vmp_pmm_update_lam(prior_a[e], prior_b[e], s, n, par + 2 * (int64_t)e,
                                mom + 2 * (int64_t)e);
    }
    bs[tid] = t;
    __syncthreads();
    block_halve_sum<NT>(bs, tid);
    if (tid == 0) bound[0] = bs[0];
}

template <int KT>
void launch_pass(vmp_ctx *ctx, int64_t nc, bool hidden, const PmmArgs &a)
{
    if (hidden)
        hipLaunchKernelGGL((pmm_pass_kernel<KT, true>), dim3((unsigned)nc), dim3(NT), 0,
                           ctx->stream, a);
    else
        hipLaunchKernelGGL((pmm_pass_kernel<KT, false>), dim3((unsigned)nc), dim3(NT), 0,
                           ctx->stream, a);
}

template <typename T>
void launch_pack(vmp_ctx *ctx, int64_t n, const void *x, const uint8_t *mask, uint16_t *xp,
                 int32_t *flags, double *ws)
{
    hipLaunchKernelGGL(pmm_pack_kernel<T>, dim3((unsigned)vmp_pmm_pack_blocks(n)), dim3(NT), 0,
                       ctx->stream, n, vmp_pmm_pack_span(n), (const T *)x, mask, xp, flags, ws,
                       (int64_t *)(ws + VMP_PMM_PACK_BLOCKS));
}

}  // namespace

// the pass kernel for a.K, on nc chunks (vmp_common.h; vmp_mmm.hip calls it as well)
void vmp_pmm_launch_pass(vmp_ctx *ctx, int64_t nc, bool hidden, const PmmArgs &a)
{
    switch (vmp_pmm_kpad(a.K) / 16) {
    case 1: launch_pass<1>(ctx, nc, hidden, a); break;
    case 2: launch_pass<2>(ctx, nc, hidden, a); break;
    case 3: launch_pass<3>(ctx, nc, hidden, a); break;
    default: launch_pass<4>(ctx, nc, hidden, a); break;
    }
}

#define PMM_SHAPE(ctx, D, K)                                                                      \
    VMP_REQUIRE(ctx, K <= VMP_PMM_MAX_K && D <= VMP_PMM_MAX_D, VMP_ERR_UNSUPPORTED,               \
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_PMM_MAX_D, VMP_PMM_MAX_K)

extern "C" {

int32_t vmp_pmm_limits(int32_t *max_K, int32_t *max_D, int32_t *max_count)
{
    if (!max_K || !max_D || !max_count) return VMP_ERR_INVALID;
    *max_K = VMP_PMM_MAX_K;
    *max_D = VMP_PMM_MAX_D;
    *max_count = VMP_PMM_MAX_COUNT;
    return VMP_OK;
}

int32_t vmp_pmm_plan(int64_t N, int32_t D, int32_t K, int64_t *chunk_rows,
                     int64_t *workspace_doubles)
{
    if (N < 0 || D < 1 || K < 1) return VMP_ERR_INVALID;
    if (K > VMP_PMM_MAX_K || D > VMP_PMM_MAX_D) return VMP_ERR_UNSUPPORTED;
    if (!chunk_rows || !workspace_doubles) return VMP_ERR_INVALID;
    *chunk_rows = vmp_pmm_chunk_rows(N, D, K);
    *workspace_doubles = vmp_pmm_workspace_doubles(N, D, K);
    return VMP_OK;
}

int32_t vmp_pmm_pack(vmp_ctx *ctx, int64_t N, int32_t D, int32_t dtype, const void *x,
                     const uint8_t *mask, uint16_t *x_packed, int32_t *flags, int64_t *counts,
                     double *lgam, double *ws)
{
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && dtype >= 0 && dtype <= 3, VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, D <= VMP_PMM_MAX_D, VMP_ERR_UNSUPPORTED, "D = %d exceeds the limit %d", D,
                VMP_PMM_MAX_D);
    VMP_REQUIRE(ctx, flags && counts && lgam && ws && (N == 0 || (x && x_packed)),
                VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int64_t n = N * D;
    if (n > 0) {
        switch (dtype) {
        case 0: launch_pack<double>(ctx, n, x, mask, x_packed, flags, ws); break;
        case 1: launch_pack<int64_t>(ctx, n, x, mask, x_packed, flags, ws); break;
        case 2: launch_pack<uint8_t>(ctx, n, x, mask, x_packed, flags, ws); break;
        default: launch_pack<int32_t>(ctx, n, x, mask, x_packed, flags, ws); break;
        }
        VMP_HIP_CHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(pmm_pack_finish_kernel, dim3(1), dim3(1), 0, ctx->stream, n,
                       n > 0 ? vmp_pmm_pack_blocks(n) : 0, ws,
                       (const int64_t *)(ws + VMP_PMM_PACK_BLOCKS), counts, lgam);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_pmm_tables(vmp_ctx *ctx, int32_t D, int32_t K, int32_t form, const double *lam_mom,
                       const double *elog_pi, double *l, double *lb, double *c, double *lsum)
{
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1 && form >= 0 && form <= 3, VMP_ERR_INVALID,
                "bad arguments");
    PMM_SHAPE(ctx, D, K);
    VMP_REQUIRE(ctx, elog_pi && l && lb && c, VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    hipLaunchKernelGGL(pmm_tables_kernel, dim3((unsigned)((D * K + NT - 1) / NT)), dim3(NT), 0,
                       ctx->stream, D, K, form, lam_mom, elog_pi, l, lb, c, lsum);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_pmm_pass(vmp_ctx *ctx, int64_t N, int32_t D, int32_t K, int32_t hidden,
                     const uint16_t *x_packed, const int32_t *labels, const double *l,
                     const double *lb, const double *c, double *ws, double *S, double *M,
                     double *Nk, double *scal, double *r_out)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, ctx && N >= 0 && D >= 1 && K >= 1 && (hidden == 0 || hidden == 1),
                VMP_ERR_INVALID, "bad arguments");
    PMM_SHAPE(ctx, D, K);
    VMP_REQUIRE(ctx, l && lb && c && ws && S && Nk && scal && (!hidden || M)
                && (N == 0 || x_packed), VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int64_t nc = vmp_pmm_chunks(N, D, K);
    if (nc > 0) {
        PmmArgs a = {N, vmp_pmm_chunk_rows(N, D, K), D, K, x_packed, labels, l, lb, c, ws, r_out};
        vmp_pmm_launch_pass(ctx, nc, hidden != 0, a);
    }
    hipLaunchKernelGGL(pmm_combine_kernel, dim3((unsigned)((D * K + NT - 1) / NT)), dim3(NT), 0,
                       ctx->stream, nc, D, K, ws, S, hidden ? M : nullptr, Nk, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    double *dot_ws = ws + nc * vmp_pmm_partial_doubles(D, K, hidden), *two = dot_ws + 1024;
    int32_t rc = vmp_lda_dot(ctx, K, Nk, c, dot_ws, scal + 1);
    if (rc != VMP_OK) return rc;
    if (!hidden) return vmp_lda_dot(ctx, (int64_t)D * K, S, l, dot_ws, scal + 2);
    rc = vmp_lda_dot(ctx, (int64_t)D * K, S, l, dot_ws, two);
    if (rc != VMP_OK) return rc;
    rc = vmp_lda_dot(ctx, (int64_t)D * K, M, lb, dot_ws, two + 1);
    if (rc != VMP_OK) return rc;
    hipLaunchKernelGGL(pmm_sub2_kernel, dim3(1), dim3(1), 0, ctx->stream, two, scal + 2);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_pmm_update(vmp_ctx *ctx, int32_t D, int32_t K, int32_t per_element,
                       const double *prior_a, const double *prior_b, const double *S,
                       const double *cnt, double *par, double *mom, double *bound)
{
    VMP_REQUIRE(ctx, ctx && D >= 1 && K >= 1 && (per_element == 0 || per_element == 1),
                VMP_ERR_INVALID, "bad arguments");
    PMM_SHAPE(ctx, D, K);
    VMP_REQUIRE(ctx, prior_a && prior_b && par && mom && bound, VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    hipLaunchKernelGGL(pmm_update_kernel, dim3(1), dim3(NT), 0, ctx->stream, D, K, per_element,
                       prior_a, prior_b, S, cnt, par, mom, bound);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
