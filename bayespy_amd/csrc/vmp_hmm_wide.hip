// vmp_hmm_wide.hip -- the wide-emission pass of the fused hidden-Markov-model block: the model of
// vmp_hmm_fused.hip with 1 <= D <= 32 dimensions.
//
// vmp_hmm_fused.hip forms e_t[j] inside the chain as a dot product over NF = D (D + 1) / 2 + D + 1
// features and keeps NF x KP coefficients and NF x 64 accumulators in LDS; at D = 32 NF is 561 and
// neither fits.  Here the two parts that are parallel over the (b, t) plate leave the chain:
//
//   hmmw_emit_kernel   E = phi(Y) C^T on the fp64 matrix cores, C streamed through LDS
//   hmmw_chain_kernel  the recursion alone: lane j of a chain reads e_t[j] from E (one coalesced
//                      load, requested one step ahead), gamma_t overwrites la_t in the workspace
//   hmmw_stats_kernel  T = Gamma^T phi(Y) on the fp64 matrix cores, split over feature slabs and
//                      row ranges, partials added in a fixed order
//   hmmw_combine_kernel adds every partial in workgroup order and lays T_k out as [1, y, y y^T]
//
// Splits, workspace and the order of the additions: vmp_hmm_wide_dev.h.  Matrix-core layout of
// v_mfma_f64_16x16x4f64 (lane l, l15 = l & 15, l4 = l >> 4): A[row l15][k l4], B[k l4][col l15],
// accumulator element r = D[row l4 + 4 r][col l15].
#include "vmp_common.h"
#include "vmp_hmm_wide_dev.h"

namespace {

// feature f as the two factors packed into an int; features past NF are 1 * 1 (their coefficient
// is zero in kernel 1 and their column is never stored in kernel 3)
__device__ __forceinline__ int hmmw_pair(int D, int NF, int f)
{
    int pa = D, pb = D;
    if (f < NF) vmp_hmmf_feature(D, f, &pa, &pb);
    return pa | (pb << 8);
}

// ---- kernel 1: the emission table -------------------------------------------------------------------
struct HmmwEmitArgs {
    int64_t R, nblk;              // rows of the (b, t) plate, blocks of 64 rows
    int D, K, KP, NF, ldc;
    const double *Y, *C;
    const uint8_t *mask;          // R bytes or null
    double *E;                    // R x KP
};

// Four wavefronts, each with one tile of 16 rows; NT column tiles of 16 states.  LDS: the rows' y
// (64 x (D + 1 | 1): the 1 of the constant feature behind each row), one chunk of C
// (VMP_HMMW_C_CHUNK x hmmw_stride(NT)) and the factor pairs of the features.
template <int NT>
__global__ __launch_bounds__(256) void hmmw_emit_kernel(HmmwEmitArgs a)
{
    extern __shared__ double hmmw_lds[];
    constexpr int KPC = NT * 16, CS = hmmw_stride(NT), FCH = VMP_HMMW_C_CHUNK;
    const int D = a.D, K = a.K, KP = a.KP, NF = a.NF, NFP = (NF + 3) & ~3, YS = (D + 1) | 1;
    double *ys = hmmw_lds;
    double *Cs = ys + 64 * YS;
    int *pair = (int *)(Cs + FCH * CS);
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    for (int f = tid; f < NFP; f += 256) pair[f] = hmmw_pair(D, NF, f);
    double *myy = ys + w * 16 * YS;
    const double *yr = myy + l15 * YS;

    for (int64_t blk = blockIdx.x; blk < a.nblk; blk += gridDim.x) {
        const int64_t row0 = blk * 64 + w * 16;
        // this wavefront's 16 rows: zeros for a masked row and past the end of the plate
        for (int e = lane; e < 16 * D; e += 64) {
            const int i = e / D, d = e - i * D;
            const int64_t r = row0 + i;
            const bool ok = r < a.R && (!a.mask || a.mask[r] != 0);
            myy[i * YS + d] = ok ? a.Y[r * D + d] : 0.0;
        }
        if (lane < 16) myy[lane * YS + D] = 1.0;
        v4f64 acc[NT];
#pragma unroll
        for (int ct = 0; ct < NT; ++ct) acc[ct] = v4f64{0.0, 0.0, 0.0, 0.0};
        for (int f0 = 0; f0 < NFP; f0 += FCH) {
            __syncthreads();                        // the readers of the previous chunk are done
            for (int e = tid; e < FCH * KPC; e += 256) {
                const int ff = e % FCH, k = e / FCH;
                Cs[ff * CS + k] = (k < K && f0 + ff < NF) ? a.C[(int64_t)k * a.ldc + f0 + ff] : 0.0;
            }
            __syncthreads();
            const int nq = ((NFP - f0 < FCH) ? NFP - f0 : FCH) >> 2;
            for (int q = 0; q < nq; ++q) {
                const int pr = pair[f0 + 4 * q + l4];
                const double phi = yr[pr & 255] * yr[pr >> 8];
                const double *cb = Cs + (4 * q + l4) * CS + l15;
#pragma unroll
                for (int ct = 0; ct < NT; ++ct)
                    acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(phi, cb[ct * 16], acc[ct], 0, 0, 0);
            }
        }
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
            const int64_t r = row0 + l4 + 4 * r4;
            if (r >= a.R) continue;
            const bool obs = !a.mask || a.mask[r] != 0;
#pragma unroll
            for (int ct = 0; ct < NT; ++ct) {
                const int k = ct * 16 + l15;
                if (k < KP) a.E[r * KP + k] = k >= K ? -INFINITY : (obs ? acc[ct][r4] : 0.0);
            }
        }
    }
}

// ---- kernel 2: the chain ----------------------------------------------------------------------------
struct HmmwChainArgs {
    int64_t B, cpw;
    int T, K;
    const double *E;          // B T x KP, or null (no emission term)
    const double *la0, *lA;
    const int32_t *labels;
    const uint8_t *mask;
    double *aw;               // B x T x K: la on the way forward, gamma on the way back
    double *part;
    double *gamma, *z0, *zz;
};

template <int KP>
__device__ __forceinline__ double hmmw_grp_max(double v)
{
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

template <int KP>
__device__ __forceinline__ double hmmw_grp_sum(double v)
{
#pragma unroll
    for (int m = 1; m < KP; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the value of lane (j, group g) added over the groups in group order; valid in lanes < KP
template <int KP>
__device__ __forceinline__ double hmmw_across_groups(double v, int lane)
{
    double t = v;
#pragma unroll
    for (int g = 1; g < 64 / KP; ++g) t += __shfl(v, (lane & (KP - 1)) + g * KP, 64);
    return t;
}

// The lane mapping, the recursion and the order of every addition of hmmf_pass_kernel; registers:
// the column of sum xi and the exponentials of the step (KP doubles each); LDS: <log A> and its
// transpose and the la / u vectors -- nothing that grows with D.  A masked step has E = 0, so the
// mask only gives the chain its weight here.
template <int KP>
__global__ __launch_bounds__(64) void hmmw_chain_kernel(HmmwChainArgs a)
{
    extern __shared__ double hmmw_lds[];
    constexpr int G = 64 / KP;
    const int T = a.T, K = a.K;
    double *As = hmmw_lds;                 // [i * KP + j]
    double *ATs = As + KP * KP;            // [j * KP + i]
    double *vec = ATs + KP * KP;           // [lane] = la of (group, i)
    double *uvec = vec + 64;               // [lane] = u of (group, j)
    const int lane = threadIdx.x, grp = lane / KP, j = lane % KP;
    const bool act = j < K;

    for (int e = lane; e < KP * KP; e += 64) {
        const int i = e / KP, c = e % KP;
        const double v = (i < K && c < K) ? a.lA[i * K + c] : -INFINITY;
        As[e] = v;
        ATs[c * KP + i] = v;
    }
    lds_fence();
    double *myv = vec + grp * KP, *myu = uvec + grp * KP;
    const double *Acol = As + j, *ATcol = ATs + j;
    const double la0 = act ? a.la0[j] : -INFINITY;

    double xi[KP];
#pragma unroll
    for (int i = 0; i < KP; ++i) xi[i] = 0.0;
    double z0acc = 0.0, logZ = 0.0, ge = 0.0;

    const int64_t c_begin = (int64_t)blockIdx.x * a.cpw;
    const int64_t c_end = (c_begin + a.cpw < a.B) ? c_begin + a.cpw : a.B;
    for (int64_t c0 = c_begin; c0 < c_end; c0 += G) {
        const int64_t c = c0 + grp;
        const bool live = c < c_end;
        const int64_t cc = live ? c : c_begin;
        const bool store = live && act;
        // the chain's weight: 0 past the end of the range and without an observed step
        double w = live ? 1.0 : 0.0;
        if (a.mask) {
            const uint8_t *mrow = a.mask + cc * (int64_t)T;
            int any = 0;
            for (int t = j; t < T; t += KP) any |= mrow[t];
#pragma unroll
            for (int m = 1; m < KP; m <<= 1) any |= __shfl_xor(any, m, 64);
            if (any == 0) w = 0.0;
        }
        double *aw = a.aw + cc * (int64_t)T * K;

        if (a.labels) {
            // fixed states: gamma and xi are one-hot, log Z = 0
            const int32_t *lab = a.labels + cc * (int64_t)T;
            int prev = -1;
            for (int t = 0; t < T; ++t) {
                const int cur = lab[t];
                const double g = (j == cur) ? 1.0 : 0.0;
                if (t == 0) {
                    z0acc += g * w;
                    if (a.z0 && store) a.z0[cc * K + j] = g;
                } else {
#pragma unroll
                    for (int i = 0; i < KP; ++i) {
                        const double x = (i == prev) ? g : 0.0;
                        xi[i] += x * w;
                        if (a.zz && store && i < K)
                            a.zz[((cc * (int64_t)(T - 1) + (t - 1)) * K + i) * K + j] = x;
                    }
                }
                if (store) aw[(int64_t)t * K + j] = g;
                if (a.gamma && store) a.gamma[(cc * (int64_t)T + t) * K + j] = g;
                prev = cur;
            }
            continue;
        }

        const double *Ec = a.E ? a.E + cc * (int64_t)T * KP + j : nullptr;
        auto emit = [&](int t) -> double { return Ec ? Ec[(int64_t)t * KP] : 0.0; };
        // ---- forward: e of step n + 1 is requested before the arithmetic of step n ----------------
        double e_next = emit(1);
        double la = la0 + emit(0);
        if (!act) la = -INFINITY;
        if (store) aw[j] = la;
        for (int n = 1; n < T; ++n) {
            const double e = e_next;
            if (n + 1 < T) e_next = emit(n + 1);
            myv[j] = la;
            lds_fence();
            double m, s;
            vmp_hmmf_column(myv, Acol, KP, K, &m, &s);
            const double q = act ? m + log(s) + e : -INFINITY;
            const double M = hmmw_grp_max<KP>(q);
            const double S = hmmw_grp_sum<KP>(vmp_hmmf_exp_shift(q, M));
            const double cn = M + log(S);
            logZ += cn * w;
            la = q - cn;
            if (store) aw[(int64_t)n * K + j] = la;
            lds_fence();
        }
        // ---- backward: gamma_{n+1} goes where la_{n+1} stood; la_n and e_{n+1} of the step to
        // come are requested first.  aw[n K + j] was written by this lane. ------------------------
        double lb = 0.0;
        double la_next = la;
        double e = emit(T - 1);
        double lan = act ? aw[(int64_t)(T - 2) * K + j] : -INFINITY;
        for (int n = T - 2; n >= 0; --n) {
            double e_prev = 0.0, lan_prev = -INFINITY;
            if (n > 0) {
                e_prev = emit(n);
                if (act) lan_prev = aw[(int64_t)(n - 1) * K + j];
            }
            const double gl = act ? la_next + lb : -INFINITY;
            const double M = hmmw_grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, M);
            const double gamma = ex / hmmw_grp_sum<KP>(ex);
            myv[j] = lan;
            myu[j] = act ? e + lb : -INFINITY;
            lds_fence();
            double m = -INFINITY;
#pragma unroll
            for (int i = 0; i < KP; ++i) m = fmax(m, myv[i] + Acol[i * KP]);
            double p[KP];
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                p[i] = vmp_hmmf_exp_shift(myv[i] + Acol[i * KP], m);
                s += p[i];
            }
            const double r = vmp_hmmf_ratio(gamma, s);
#pragma unroll
            for (int i = 0; i < KP; ++i) {
                const double x = p[i] * r;
                xi[i] += x * w;
                if (a.zz && store && i < K)
                    a.zz[((cc * (int64_t)(T - 1) + n) * K + i) * K + j] = x;
            }
            if (gamma * w != 0.0) ge += gamma * w * e;
            if (store) aw[(int64_t)(n + 1) * K + j] = gamma;
            if (a.gamma && store) a.gamma[(cc * (int64_t)T + n + 1) * K + j] = gamma;
            // lb_n[i] on lane i: the row of <log A> is a column of its transpose
            double mr, sr;
            vmp_hmmf_column(myu, ATcol, KP, K, &mr, &sr);
            const double lbn = act ? mr + log(sr) : -INFINITY;
            lb = lbn - hmmw_grp_max<KP>(lbn);
            la_next = lan;
            lan = lan_prev;
            e = e_prev;
            lds_fence();
        }
        {
            e = emit(0);
            const double gl = act ? la_next + lb : -INFINITY;
            const double M = hmmw_grp_max<KP>(gl);
            const double ex = vmp_hmmf_exp_shift(gl, M);
            const double gamma = ex / hmmw_grp_sum<KP>(ex);
            z0acc += gamma * w;
            if (gamma * w != 0.0) ge += gamma * w * e;
            if (store) aw[j] = gamma;
            if (a.gamma && store) a.gamma[cc * (int64_t)T * K + j] = gamma;
            if (a.z0 && store) a.z0[cc * K + j] = gamma;
        }
    }

    // ---- the partial of this workgroup: groups in group order -----------------------------------
    const int64_t per = vmp_hmmw_chain_partial_doubles(K);
    double *part = a.part + (int64_t)blockIdx.x * per;
    const double z0s = hmmw_across_groups<KP>(z0acc, lane);
    if (lane < K) part[lane] = z0s;
#pragma unroll
    for (int i = 0; i < KP; ++i) {
        const double v = hmmw_across_groups<KP>(xi[i], lane);
        if (i < K && lane < K) part[K + i * K + lane] = v;
    }
    // log Z is the same in every lane of a group; gamma . e is a lane's own share
    double zs = 0.0, gs = 0.0;
    for (int g = 0; g < G; ++g) zs += __shfl(logZ, g * KP, 64);
    for (int l = 0; l < 64; ++l) gs += __shfl(ge, l, 64);
    if (lane == 0) {
        part[per - 2] = zs;
        part[per - 1] = gs;
    }
}

// ---- kernel 3: the emission statistics --------------------------------------------------------------
struct HmmwStatsArgs {
    int64_t R, rpw;               // rows of the plate, rows of a workgroup
    int D, K, NF;
    const double *Y;
    const double *gam;            // R x K (the in-place gamma of the chain kernel)
    const uint8_t *mask;
    double *part;                 // row ranges x K x NF (compact features)
};

// Workgroup (blockIdx.x = row range, blockIdx.y = feature slab), four wavefronts with three
// 16-feature tiles each and all NT state tiles: 3 NT accumulators.  A step stages
// VMP_HMMW_ROWS rows of y and gamma in LDS (zeros for masked rows and past the end); the
// A operand is gamma^T, the B operand the product of the two factors of the lane's feature,
// read from the staged y.  The factors of a lane's three features are fixed for the whole kernel.
template <int NT>
__global__ __launch_bounds__(256) void hmmw_stats_kernel(HmmwStatsArgs a)
{
    extern __shared__ double hmmw_lds[];
    constexpr int GS = hmmw_stride(NT), RW = VMP_HMMW_ROWS, FPW = VMP_HMMW_SLAB_TILES / 4;
    const int D = a.D, K = a.K, NF = a.NF, YS = (D + 1) | 1;
    double *ys = hmmw_lds;            // [RW][YS]
    double *gs = ys + RW * YS;        // [RW][GS]
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, l15 = lane & 15, l4 = lane >> 4;
    const int NFT = (NF + 15) / 16;
    const int tile0 = blockIdx.y * VMP_HMMW_SLAB_TILES + w * FPW;
    int fa[FPW], fb[FPW];
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
        const int pr = hmmw_pair(D, NF, (tile0 + i) * 16 + l15);
        fa[i] = pr & 255;
        fb[i] = pr >> 8;
    }
    v4f64 acc[NT][FPW];
#pragma unroll
    for (int kt = 0; kt < NT; ++kt)
#pragma unroll
        for (int i = 0; i < FPW; ++i) acc[kt][i] = v4f64{0.0, 0.0, 0.0, 0.0};

    const int64_t r_begin = (int64_t)blockIdx.x * a.rpw;
    const int64_t r_end = (r_begin + a.rpw < a.R) ? r_begin + a.rpw : a.R;
    for (int64_t r0 = r_begin; r0 < r_end; r0 += RW) {
        __syncthreads();
        for (int e = tid; e < RW * D; e += 256) {
            const int i = e / D, d = e - i * D;
            const int64_t r = r0 + i;
            const bool ok = r < r_end && (!a.mask || a.mask[r] != 0);
            ys[i * YS + d] = ok ? a.Y[r * D + d] : 0.0;
        }
        if (tid < RW) ys[tid * YS + D] = 1.0;
        for (int e = tid; e < RW * NT * 16; e += 256) {
            const int i = e / (NT * 16), k = e % (NT * 16);
            const int64_t r = r0 + i;
            const bool ok = r < r_end && k < K && (!a.mask || a.mask[r] != 0);
            gs[i * GS + k] = ok ? a.gam[r * K + k] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < RW / 4; ++q) {
            const double *yr = ys + (4 * q + l4) * YS;
            const double *gr = gs + (4 * q + l4) * GS + l15;
#pragma unroll
            for (int i = 0; i < FPW; ++i) {
                if (tile0 + i >= NFT) continue;             // uniform over the wavefront
                const double b = yr[fa[i]] * yr[fb[i]];
#pragma unroll
                for (int kt = 0; kt < NT; ++kt)
                    acc[kt][i] = __builtin_amdgcn_mfma_f64_16x16x4f64(gr[kt * 16], b, acc[kt][i], 0, 0, 0);
            }
        }
    }
    double *part = a.part + (int64_t)blockIdx.x * K * NF;
#pragma unroll
    for (int i = 0; i < FPW; ++i) {
        const int f = (tile0 + i) * 16 + l15;
        if (f >= NF) continue;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int k = kt * 16 + l4 + 4 * r4;
                if (k < K) part[(int64_t)k * NF + f] = acc[kt][i][r4];
            }
    }
}

// ---- combine: every partial in workgroup order ------------------------------------------------------
// element e < per_c: the chain partials (z0sum, xisum, scal[0], scal[1]); then K x NF elements of
// kernel 3, from the compact order to rows [1, y, y y^T] of length 1 + D + D^2
__global__ void __launch_bounds__(256)
hmmw_combine_kernel(int64_t nwc, int64_t nwr, int D, int K, const double *__restrict__ cpart,
                    const double *__restrict__ spart, double *__restrict__ z0sum,
                    double *__restrict__ xisum, double *__restrict__ Tst, double *__restrict__ scal)
{
    const int64_t per = vmp_hmmw_chain_partial_doubles(K);
    const int NF = vmp_hmmf_nfeat(D), FS = 1 + D + D * D;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= per + (int64_t)K * NF) return;
    double v = 0.0;
    if (e < per) {
        for (int64_t w = 0; w < nwc; ++w) v += cpart[w * per + e];
        if (e < K) z0sum[e] = v;
        else if (e < per - 2) xisum[e - K] = v;
        else scal[e - (per - 2)] = v;
        return;
    }
    const int64_t r = e - per;
    for (int64_t w = 0; w < nwr; ++w) v += spart[w * (int64_t)K * NF + r];
    const int k = (int)(r / NF), f = (int)(r - (int64_t)k * NF);
    int pa, pb;
    vmp_hmmf_feature(D, f, &pa, &pb);
    double *Tk = Tst + (int64_t)k * FS;
    if (pb < D) {
        Tk[1 + D + pa * D + pb] = v;
        Tk[1 + D + pb * D + pa] = v;
    } else if (pa < D) {
        Tk[1 + pa] = v;
    } else {
        Tk[0] = v;
    }
}

template <int NT>
int32_t launch_emit(vmp_ctx *ctx, const HmmwEmitArgs &a)
{
    const int YS = (a.D + 1) | 1, NFP = (a.NF + 3) & ~3;
    const size_t lds = (size_t)(64 * YS + VMP_HMMW_C_CHUNK * hmmw_stride(NT)) * sizeof(double)
                       + (size_t)NFP * sizeof(int);
    const int64_t grid = a.nblk < 2048 ? a.nblk : 2048;
    hipLaunchKernelGGL((hmmw_emit_kernel<NT>), dim3((unsigned)grid), dim3(256), lds, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

template <int KP>
int32_t launch_chain(vmp_ctx *ctx, int64_t nw, const HmmwChainArgs &a)
{
    const size_t lds = (size_t)(2 * KP * KP + 128) * sizeof(double);
    static bool raised[64] = {false};
    const int dev = ctx->device & 63;
    if (lds > 48 * 1024 && !raised[dev]) {
        VMP_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)hmmw_chain_kernel<KP>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               160 * 1024));
        raised[dev] = true;
    }
    hipLaunchKernelGGL((hmmw_chain_kernel<KP>), dim3((unsigned)nw), dim3(64), lds, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

template <int NT>
int32_t launch_stats(vmp_ctx *ctx, int64_t nwr, const HmmwStatsArgs &a)
{
    const int YS = (a.D + 1) | 1;
    const size_t lds = (size_t)(VMP_HMMW_ROWS * (YS + hmmw_stride(NT))) * sizeof(double);
    hipLaunchKernelGGL((hmmw_stats_kernel<NT>), dim3((unsigned)nwr, (unsigned)vmp_hmmw_slabs(a.D)),
                       dim3(256), lds, ctx->stream, a);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // namespace

// ---- the plate-parallel stages as host calls (vmp_hmm_wide_dev.h): vmp_hmm_wide_pass below and
// the passes that bring another stage of their own (vmp_hmm_seg.hip, vmp_hmm_mult.hip) launch the
// same instances ----------------------------------------------------------------------------------
int32_t vmp_hmmw_emit(vmp_ctx *ctx, int64_t R, int D, int K, const double *Y, const double *C,
                      int ldc, const uint8_t *mask, double *E)
{
    const int NT = (K + 15) / 16;
    HmmwEmitArgs ea = {R, (R + 63) / 64, D, K, vmp_hmmf_kpad(K), vmp_hmmf_nfeat(D), ldc, Y, C, mask, E};
    return NT == 1 ? launch_emit<1>(ctx, ea) : NT == 2 ? launch_emit<2>(ctx, ea)
           : NT == 3 ? launch_emit<3>(ctx, ea) : launch_emit<4>(ctx, ea);
}

int32_t vmp_hmmw_chain(vmp_ctx *ctx, int64_t B, int T, int K, const double *E, const double *la0,
                       const double *lA, const int32_t *labels, const uint8_t *mask, double *aw,
                       double *cpart, double *gamma, double *z0, double *zz)
{
    const int64_t nwc = vmp_hmmw_chain_wgs(B, K);
    HmmwChainArgs ca = {B, vmp_hmmw_chains_per_wg(B, K), T, K, E, la0, lA, labels, mask, aw, cpart,
                        gamma, z0, zz};
    switch (vmp_hmmf_kpad(K)) {
    case 2: return launch_chain<2>(ctx, nwc, ca);
    case 4: return launch_chain<4>(ctx, nwc, ca);
    case 8: return launch_chain<8>(ctx, nwc, ca);
    case 16: return launch_chain<16>(ctx, nwc, ca);
    case 32: return launch_chain<32>(ctx, nwc, ca);
    default: return launch_chain<64>(ctx, nwc, ca);
    }
}

int32_t vmp_hmmw_stats(vmp_ctx *ctx, int64_t R, int D, int K, const double *Y, const double *gam,
                       const uint8_t *mask, double *spart)
{
    const int NT = (K + 15) / 16;
    const int64_t nwr = vmp_hmmw_row_wgs(R, D, K);
    HmmwStatsArgs sa = {R, vmp_hmmw_rows_per_wg(R, D, K), D, K, vmp_hmmf_nfeat(D), Y, gam, mask, spart};
    return NT == 1 ? launch_stats<1>(ctx, nwr, sa) : NT == 2 ? launch_stats<2>(ctx, nwr, sa)
           : NT == 3 ? launch_stats<3>(ctx, nwr, sa) : launch_stats<4>(ctx, nwr, sa);
}

int32_t vmp_hmmw_combine(vmp_ctx *ctx, int64_t nwc, int64_t nwr, int D, int K, const double *cpart,
                         const double *spart, const double *elog_a0, const double *elog_A,
                         double *dot_ws, double *z0sum, double *xisum, double *Tstat, double *scal)
{
    const int64_t ne = vmp_hmmw_chain_partial_doubles(K) + (int64_t)K * vmp_hmmf_nfeat(D);
    hipLaunchKernelGGL(hmmw_combine_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0,
                       ctx->stream, nwc, nwr, D, K, cpart, spart, z0sum, xisum, Tstat, scal);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    const int32_t rc = vmp_lda_dot(ctx, K, z0sum, elog_a0, dot_ws, scal + 2);
    if (rc != VMP_OK) return rc;
    return vmp_lda_dot(ctx, (int64_t)K * K, xisum, elog_A, dot_ws, scal + 3);
}

extern "C" {

int32_t vmp_hmm_wide_limits(int32_t *max_K, int32_t *max_D)
{
    if (!max_K || !max_D) return VMP_ERR_INVALID;
    *max_K = VMP_HMMW_MAX_K;
    *max_D = VMP_HMMW_MAX_D;
    return VMP_OK;
}

int32_t vmp_hmm_wide_plan(int64_t B, int32_t T, int32_t D, int32_t K, int64_t *chains_per_wg,
                          int64_t *workspace_doubles)
{
    if (B < 0 || T < 2 || D < 1 || K < 1 || !chains_per_wg || !workspace_doubles)
        return VMP_ERR_INVALID;
    if (K > VMP_HMMW_MAX_K || D > VMP_HMMW_MAX_D) return VMP_ERR_UNSUPPORTED;
    *chains_per_wg = vmp_hmmw_chains_per_wg(B, K);
    *workspace_doubles = vmp_hmmw_workspace_doubles(B, T, D, K);
    return VMP_OK;
}

int32_t vmp_hmm_wide_pass(vmp_ctx *ctx, int64_t B, int32_t T, int32_t D, int32_t K,
                          const double *Y, const double *C, int32_t ldc, const double *elog_a0,
                          const double *elog_A, const int32_t *labels, const uint8_t *mask,
                          double *ws, double *z0sum, double *xisum, double *Tstat, double *scal,
                          double *gamma, double *z0, double *zz)
{
    // the shape first, so that the answer for a shape does not depend on the other arguments
    VMP_REQUIRE(ctx, B >= 0 && T >= 2 && D >= 1 && K >= 1, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= VMP_HMMW_MAX_K && D <= VMP_HMMW_MAX_D, VMP_ERR_UNSUPPORTED,
                "D = %d, K = %d exceed the limits (%d, %d)", D, K, VMP_HMMW_MAX_D, VMP_HMMW_MAX_K);
    const int NF = vmp_hmmf_nfeat(D);
    VMP_REQUIRE(ctx, !C || ldc >= NF, VMP_ERR_INVALID, "ldc = %d is below the %d features", ldc, NF);
    VMP_REQUIRE(ctx, ctx && elog_a0 && elog_A && ws && z0sum && xisum && Tstat && scal
                     && (B == 0 || Y), VMP_ERR_INVALID, "null argument");
    VMP_FLUSH_SMALL(ctx);
    const int KP = vmp_hmmf_kpad(K);
    const int64_t R = B * (int64_t)T;
    const int64_t nwc = vmp_hmmw_chain_wgs(B, K), nwr = vmp_hmmw_row_wgs(R, D, K);
    const int64_t per = vmp_hmmw_chain_partial_doubles(K);
    double *E = ws, *aw = E + R * KP, *cpart = aw + R * K, *spart = cpart + nwc * per;
    double *dot_ws = spart + nwr * (int64_t)K * NF;
    int32_t rc = VMP_OK;
    if (R > 0) {
        const bool emit = C && !labels;
        if (emit) {
            rc = vmp_hmmw_emit(ctx, R, D, K, Y, C, ldc, mask, E);
            if (rc != VMP_OK) return rc;
        }
        rc = vmp_hmmw_chain(ctx, B, T, K, emit ? E : nullptr, elog_a0, elog_A, labels, mask, aw,
                            cpart, gamma, z0, zz);
        if (rc != VMP_OK) return rc;
        rc = vmp_hmmw_stats(ctx, R, D, K, Y, aw, mask, spart);
        if (rc != VMP_OK) return rc;
    }
    return vmp_hmmw_combine(ctx, nwc, nwr, D, K, cpart, spart, elog_a0, elog_A, dot_ws, z0sum,
                            xisum, Tstat, scal);
}

}  // extern "C"
