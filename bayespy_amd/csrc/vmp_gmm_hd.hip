// vmp_gmm_hd.hip -- the fused full-covariance Gaussian-mixture block for 1 <= D <= 64, K <= 64
// (the plan, plans/gmm_hd.py, uses it for 33 <= D <= 64; D <= 32 is accepted so that the pass can
// be compared with vmp_gmm_pass on the same inputs).
//
// The model, the state (vmp_gmm_layout) and the formulas are those of vmp_gmm.hip; what differs:
//   * the coefficient table at off_C is in the NATURAL order of the statistics,
//     row k = [c_k, h_k (D), A_k = -1/2 <Lambda_k> (D x D, symmetric)], row stride F2P = FS rounded
//     up to 8, so that sum_nk r phi = <C, T> stays one contraction of two tables with one indexing;
//   * the pass is two plate kernels (vmp_gmm_hd_dev.h) and a fixed-order reduce;
//   * the per-cluster kernels keep the D x D matrix of their cluster in LDS, one workgroup per
//     cluster and D*D / 256 elements per thread, where those of vmp_gmm.hip hold one element per lane.
#include "vmp_gmm_hd_dev.h"

namespace {

constexpr int NT = 256;

inline void hd_fill_layout(int D, int K, vmp_gmm_layout *L)
{
    int64_t KP = 16;
    while (KP < K) KP <<= 1;
    const int64_t DP = (D + 15) / 16 * 16;
    const int64_t FS = 1 + D + (int64_t)D * D;
    const int64_t F2P = (FS + 7) / 8 * 8;
    int64_t o = 0;
    L->DP = DP; L->KP = KP; L->FS = FS; L->FP = F2P; L->F2P = F2P;
    L->off_T = o;         L->len_T = KP * FS; o += L->len_T;
    L->off_zs = o;        o += 8;
    L->off_alpha = o;     o += 2 * KP;
    L->off_mu = o;        o += KP * D;
    L->off_Cmu = o;       o += KP * D * D;
    L->off_logdetLmu = o; o += KP;
    L->off_nk = o;        o += KP;
    L->off_Vk = o;        o += KP * D * D;
    L->off_Lam = o;       o += KP * D * D;
    L->off_logdetLam = o; o += KP;
    L->off_logdetV = o;   o += KP;
    L->off_C = o;         o += KP * F2P;
    L->off_prior = o;     o += KP + 8 + (int64_t)D * D;   // alpha0[KP], beta0, n0, logdetV0, -, V0
    L->off_scal = o;      o += 8;
    L->off_L = o;         o += 8;
    L->total = (o + 7) / 8 * 8;
}

// ---- the pass: one-hot R, the reduce, <C, T> ---------------------------------------------------
__global__ void __launch_bounds__(NT)
gmm_hd_onehot_kernel(const int64_t *__restrict__ labels, int64_t N, int K, double *__restrict__ R)
{
    const int64_t total = N * K;
    for (int64_t e = (int64_t)blockIdx.x * NT + threadIdx.x; e < total; e += (int64_t)gridDim.x * NT) {
        const int64_t n = e / K;
        R[e] = labels[n] == e - n * K ? 1.0 : 0.0;
    }
}

// T_k[f] <- sum over the point chunks, in order, of the partials of gmm_hd_s2_kernel.  Element
// (i, j) of S2 is read at (min, max) of its upper tile, so S2 is symmetric bit for bit.
__global__ void __launch_bounds__(NT)
gmm_hd_reduce_kernel(vmp_gmm_layout L, int D, const double *__restrict__ P, int nchunk, int KP8,
                     double *__restrict__ st)
{
    const int f = blockIdx.x * NT + threadIdx.x, k = blockIdx.y;
    if (f >= (int)L.FS) return;
    const int DP = (int)L.DP, DT = DP / 16;
    const int64_t PS = 8 + DP + 256 * (DT * (DT + 1) / 2);
    int off = 0;
    if (f >= 1 && f <= D) {
        off = 8 + f - 1;
    } else if (f > D) {
        const int e = f - 1 - D, i = e / D, j = e - i * D;
        const int ii = i < j ? i : j, jj = i < j ? j : i;
        const int a = ii >> 4, b = jj >> 4;
        const int tix = a * DT - a * (a - 1) / 2 + (b - a);
        off = 8 + DP + 256 * tix + (ii & 15) * 16 + (jj & 15);
    }
    double s = 0.0;
    for (int c = 0; c < nchunk; ++c) s += P[((int64_t)c * KP8 + k) * PS + off];
    st[L.off_T + (int64_t)k * L.FS + f] = s;
}

// sum_n lse_n (workgroup partials in order) and sum_nk r phi = <C, T>: both tables in the natural
// order, products added with their rounding errors carried (K FS is up to 266 305 terms); 0 * -inf
// (impossible clusters) counts as 0 like the p != 0 guard of the reference (expfamily.py:455-460).
constexpr int NTR = 1024;
__global__ void __launch_bounds__(NTR)
gmm_hd_rphi_kernel(vmp_gmm_layout L, int K, const double *__restrict__ Plse, int nb,
                   double *__restrict__ st)
{
    __shared__ double red[NTR / 64];
    const int FS = (int)L.FS;
    double acc = 0.0, lo = 0.0;
    for (int k = 0; k < K; ++k) {
        const double *C = st + L.off_C + (int64_t)k * L.F2P;
        const double *T = st + L.off_T + (int64_t)k * L.FS;
        for (int f = threadIdx.x; f < FS; f += NTR) {
            const double t = T[f];
            if (t != 0.0) {
                double e;
                acc = vmp_two_sum(acc, C[f] * t, &e);
                lo += e;
            }
        }
    }
    acc = block_sum<NTR>(acc + lo, red);
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < nb; ++b) s += Plse[b];
        st[L.off_zs + 0] = s;
        st[L.off_zs + 1] = acc;
    }
}

// ---------------------------------------------------------------------------
// Per-cluster kernels: one workgroup of 256 threads per cluster, the D x D matrix in LDS (row
// stride D), thread `tid` owning the elements tid, tid + 256, ...
//
// SPD inverse in place by Gauss-Jordan sweeps over the pivots in order (grp_spd_inverse of
// vmp_gmm.hip; tests/gmm_pass_host.spd_inverse): column and row p are copied out (cv, rv), then
// every element is rewritten.  Returns log|M|; a pivot <= 0 sets *bad and the sweep goes on with
// whatever the arithmetic gives (no fault).  Every thread computes the same pivots.
// ---------------------------------------------------------------------------
__device__ inline double hd_spd_inverse(double *M, int D, double *cv, double *rv, int *bad)
{
    const int tid = threadIdx.x;
    double ld = 0.0, prod = 1.0;
    for (int p = 0; p < D; ++p) {
        for (int e = tid; e < D; e += NT) {
            cv[e] = M[e * D + p];
            rv[e] = M[p * D + e];
        }
        __syncthreads();
        const double piv = rv[p];
        if (!(piv > 0.0)) *bad = 1;
        logdet_accumulate(piv, prod, ld);
        const double d = fast_recip(piv);
        for (int e = tid; e < D * D; e += NT) {
            const int i = e / D, j = e - i * D;
            const double ci = cv[i], rj = rv[j];
            double v;
            if (i == p) v = (j == p) ? d : rj * d;
            else if (j == p) v = -ci * d;
            else v = M[e] - ci * rj * d;
            M[e] = v;
        }
        __syncthreads();
    }
    return logdet_finish(prod, ld);
}

inline size_t hd_cluster_lds(int D) { return (size_t)(D * D + 3 * D) * sizeof(double); }

// every node at its prior (ExponentialFamily.initialize_from_prior, expfamily.py:168-184)
__global__ void __launch_bounds__(NT)
gmm_hd_init_state_kernel(vmp_gmm_layout L, int D, int K, double beta0, double n0, double *st)
{
    extern __shared__ double Ms[];
    double *cv = Ms + D * D, *rv = cv + D;
    const int tid = threadIdx.x, k = blockIdx.x;
    const double *pr = st + L.off_prior;
    const double *V0 = pr + L.KP + 8;
    if (tid == 0) {
        double sa = 0.0;
        for (int c = 0; c < K; ++c) sa += pr[c];
        st[L.off_alpha + k] = pr[k];
        st[L.off_alpha + L.KP + k] = vmp_digamma(pr[k]) - vmp_digamma(sa);
        st[L.off_nk + k] = n0;
        st[L.off_logdetLmu + k] = (double)D * log(beta0);
    }
    for (int e = tid; e < D * D; e += NT) {
        const int i = e / D, j = e - i * D;
        st[L.off_Cmu + (int64_t)k * D * D + e] = (i == j) ? 1.0 / beta0 : 0.0;
        st[L.off_Vk + (int64_t)k * D * D + e] = V0[e];
        Ms[e] = V0[e];
    }
    for (int e = tid; e < D; e += NT) st[L.off_mu + (int64_t)k * D + e] = 0.0;
    __syncthreads();
    int bad = 0;
    const double ld = hd_spd_inverse(Ms, D, cv, rv, &bad);
    for (int e = tid; e < D * D; e += NT) st[L.off_Lam + (int64_t)k * D * D + e] = n0 * Ms[e];
    if (tid == 0) {
        double md = 0.0;
        for (int c = 0; c < D; ++c) md += vmp_digamma(0.5 * n0 - 0.5 * c);
        st[L.off_logdetV + k] = ld;
        st[L.off_logdetLam + k] = md + (double)D * log(2.0) - ld;
        if (bad) st[L.off_scal + 3] = (double)VMP_ERR_NOT_POSDEF;
        if (k == 0) st[L.off_prior + L.KP + 2] = ld;               // log|V0|
    }
}

// mu.update(): Lambda_mu = beta0 I + R_k <Lambda_k>, Cov, mean = Cov <Lambda_k> S1_k
// (gaussian.py:649-706 with the messages gaussian.py:2451-2454 weighted by r, mixture.py:126-158)
__global__ void __launch_bounds__(NT)
gmm_hd_update_mu_kernel(vmp_gmm_layout L, int D, int K, double *st)
{
    extern __shared__ double Ms[];
    double *cv = Ms + D * D, *rv = cv + D, *bs = rv + D;
    const int tid = threadIdx.x, k = blockIdx.x;
    const double beta0 = st[L.off_prior + L.KP + 0];
    const double *T = st + L.off_T + (int64_t)k * L.FS;
    const double *Lam = st + L.off_Lam + (int64_t)k * D * D;
    const double R = T[0];
    for (int e = tid; e < D * D; e += NT) {
        const int i = e / D, j = e - i * D;
        Ms[e] = R * Lam[e] + ((i == j) ? beta0 : 0.0);
    }
    for (int e = tid; e < D; e += NT) {
        double s = 0.0;
        for (int c = 0; c < D; ++c) s += Lam[e * D + c] * T[1 + c];     // <Lambda> S1
        bs[e] = s;
    }
    __syncthreads();
    int bad = 0;
    const double ld = hd_spd_inverse(Ms, D, cv, rv, &bad);
    for (int e = tid; e < D * D; e += NT) st[L.off_Cmu + (int64_t)k * D * D + e] = Ms[e];
    for (int e = tid; e < D; e += NT) {
        double s = 0.0;
        for (int c = 0; c < D; ++c) s += Ms[e * D + c] * bs[c];
        st[L.off_mu + (int64_t)k * D + e] = s;
    }
    if (tid == 0) {
        st[L.off_logdetLmu + k] = ld;
        if (bad) st[L.off_scal + 3] = (double)VMP_ERR_NOT_POSDEF;
    }
}

// Lambda.update(): n_k = n0 + R_k, V_k = V0 + S2 - S1 mu^T - mu S1^T + R <mu mu^T>, stored as
// formed; the moments are those of its symmetric part
// (wishart.py:153-188 with the message gaussian.py:2516-2520 weighted by r)
__global__ void __launch_bounds__(NT)
gmm_hd_update_lambda_kernel(vmp_gmm_layout L, int D, int K, double *st)
{
    extern __shared__ double Ms[];
    double *cv = Ms + D * D, *rv = cv + D;
    const int tid = threadIdx.x, k = blockIdx.x;
    const double n0 = st[L.off_prior + L.KP + 1];
    const double *V0 = st + L.off_prior + L.KP + 8;
    const double *T = st + L.off_T + (int64_t)k * L.FS;
    const double *mu = st + L.off_mu + (int64_t)k * D;
    const double *Cmu = st + L.off_Cmu + (int64_t)k * D * D;
    const double R = T[0];
    const double nk = n0 + R;
    auto formed = [&](int i, int j) {
        const int e = i * D + j;
        const double mm = Cmu[e] + mu[i] * mu[j];
        return V0[e] + T[1 + D + e] - T[1 + i] * mu[j] - mu[i] * T[1 + j] + R * mm;
    };
    for (int e = tid; e < D * D; e += NT) {
        const int i = e / D, j = e - i * D;
        const double v = formed(i, j);
        st[L.off_Vk + (int64_t)k * D * D + e] = v;
        Ms[e] = 0.5 * (v + formed(j, i));
    }
    __syncthreads();
    int bad = 0;
    const double ld = hd_spd_inverse(Ms, D, cv, rv, &bad);
    for (int e = tid; e < D * D; e += NT)
        st[L.off_Lam + (int64_t)k * D * D + e] = nk * Ms[e];                // wishart.py:184
    if (tid == 0) {
        double md = 0.0;
        for (int c = 0; c < D; ++c) md += vmp_digamma(0.5 * nk - 0.5 * c);  // utils/misc.py:1146
        st[L.off_nk + k] = nk;
        st[L.off_logdetV + k] = ld;
        st[L.off_logdetLam + k] = md + (double)D * log(2.0) - ld;           // wishart.py:185
        if (bad) st[L.off_scal + 3] = (double)VMP_ERR_NOT_POSDEF;
    }
}

// z.update(), replicated half: row k of the coefficient table,
//   ell_nk = c_k + h_k . y + y^T A_k y,  c_k = <log pi_k> + 1/2 <log|Lam_k|> - D/2 log 2 pi
//   - 1/2 tr(Lam_k <mu mu^T>),  h_k = Lam_k mu_k,  A_k = -1/4 (Lam_k + Lam_k^T)
// (mixture.py:67-104); prior_only: <log pi_k> alone; padded clusters: -inf and zeros.
__global__ void __launch_bounds__(NT)
gmm_hd_prepare_z_kernel(vmp_gmm_layout L, int D, int K, int prior_only, double *st)
{
    __shared__ double red[NT / 64];
    const int tid = threadIdx.x, k = blockIdx.x;
    const int FS = (int)L.FS, F2P = (int)L.F2P;
    double *Crow = st + L.off_C + (int64_t)k * F2P;
    if (k >= K || prior_only) {
        const double c0 = k >= K ? -INFINITY : st[L.off_alpha + L.KP + k];
        for (int f = tid; f < F2P; f += NT) Crow[f] = f == 0 ? c0 : 0.0;
        return;
    }
    const double *Lam = st + L.off_Lam + (int64_t)k * D * D;
    const double *mu = st + L.off_mu + (int64_t)k * D;
    const double *Cmu = st + L.off_Cmu + (int64_t)k * D * D;
    double tr = 0.0;
    for (int e = tid; e < D * D; e += NT) {
        const int i = e / D, j = e - i * D;
        tr += Lam[e] * (Cmu[e] + mu[i] * mu[j]);
    }
    tr = block_sum<NT>(tr, red);
    for (int f = tid; f < F2P; f += NT) {
        double v = 0.0;
        if (f == 0) {
            v = st[L.off_alpha + L.KP + k]
                + (0.5 * st[L.off_logdetLam + k] - 0.5 * (double)D * log(2.0 * M_PI) - 0.5 * tr);
        } else if (f <= D) {
            const int d = f - 1;
            for (int c = 0; c < D; ++c) v += Lam[d * D + c] * mu[c];
        } else if (f < FS) {
            const int e = f - 1 - D, i = e / D, j = e - i * D;
            v = -0.25 * (Lam[i * D + j] + Lam[j * D + i]);
        }
        Crow[f] = v;
    }
}

// ---- launches -----------------------------------------------------------------------------------
int64_t hd_max_grid(vmp_ctx *ctx) { return ctx->num_cu > 0 ? ctx->num_cu : 1; }

// point chunks of the second-moment kernel: cluster groups x chunks fill the chip once
int64_t hd_max_chunks(vmp_ctx *ctx, int K)
{
    const int64_t groups = (K + HD_NW2 - 1) / HD_NW2, c = hd_max_grid(ctx) / groups;
    return c < 1 ? 1 : c;
}

int64_t hd_partial_doubles(vmp_ctx *ctx, int K, const vmp_gmm_layout &L)
{
    const int64_t groups = (K + HD_NW2 - 1) / HD_NW2;
    return hd_max_chunks(ctx, K) * groups * HD_NW2 * hd_ps((int)(L.DP / 16));
}

template <typename Kern>
int32_t hd_allow_lds(vmp_ctx *ctx, Kern kern, size_t bytes)
{
    if (bytes > 64 * 1024)
        VMP_HIP_CHECK(ctx, hipFuncSetAttribute((const void *)kern,
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               160 * 1024));
    return VMP_OK;
}

template <int DT, int KT>
int32_t hd_launch_resp(vmp_ctx *ctx, const double *Y, int64_t N, int D, int K, const double *C,
                       int64_t F2P, double *R, double *Plse, int *nb)
{
    int64_t g = (N + HD_WGP - 1) / HD_WGP;
    if (g > hd_max_grid(ctx)) g = hd_max_grid(ctx);
    // tests only: fewer workgroups, so that a workgroup walks many trips at a small N
    const int cap = vmp_tune_get("gmm_grid_cap", 0);
    if (cap > 0 && g > cap) g = cap;
    if (g < 1) g = 1;
    const int64_t ntrips = (N + g * HD_WGP - 1) / (g * HD_WGP);
    auto kern = gmm_hd_resp_kernel<DT, KT>;
    const size_t lds = hd_resp_lds(DT, KT);
    static bool allowed = false;                  // once per instance
    if (!allowed) {
        const int32_t rc = hd_allow_lds(ctx, kern, lds);
        if (rc != VMP_OK) return rc;
        allowed = true;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)g), dim3(64 * HD_NW), lds, ctx->stream, Y, N, D, K, C,
                       F2P, R, Plse, ntrips);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    *nb = (int)g;
    return VMP_OK;
}

template <int DT>
int32_t hd_launch_resp_k(vmp_ctx *ctx, int KT, const double *Y, int64_t N, int D, int K,
                         const double *C, int64_t F2P, double *R, double *Plse, int *nb)
{
    if (KT == 1) return hd_launch_resp<DT, 1>(ctx, Y, N, D, K, C, F2P, R, Plse, nb);
    if (KT == 2) return hd_launch_resp<DT, 2>(ctx, Y, N, D, K, C, F2P, R, Plse, nb);
    return hd_launch_resp<DT, 4>(ctx, Y, N, D, K, C, F2P, R, Plse, nb);
}

template <int DT>
int32_t hd_launch_s2(vmp_ctx *ctx, const double *Y, int64_t N, int D, int K, const double *R,
                     double *P, int *nchunk_out)
{
    const int64_t nslabs = (N + HD_SLAB - 1) / HD_SLAB;
    const int groups = (K + HD_NW2 - 1) / HD_NW2;
    int64_t nchunk = nslabs < hd_max_chunks(ctx, K) ? nslabs : hd_max_chunks(ctx, K);
    const int cap = vmp_tune_get("gmm_grid_cap", 0);
    if (cap > 0 && nchunk > cap) nchunk = cap;
    if (nchunk < 1) nchunk = 1;
    const size_t lds = (size_t)HD_SLAB * hd_ys(16 * DT) * sizeof(double);
    hipLaunchKernelGGL(gmm_hd_s2_kernel<DT>, dim3((unsigned)groups, (unsigned)nchunk),
                       dim3(64 * HD_NW2), lds, ctx->stream, Y, N, D, K, R, P, nslabs,
                       groups * HD_NW2);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    *nchunk_out = (int)nchunk;
    return VMP_OK;
}

int32_t hd_run_pass(vmp_ctx *ctx, bool from_labels, const double *Y, int64_t N, int D, int K,
                    const int64_t *labels, double *R, double *state, void *workspace)
{
    VMP_REQUIRE(ctx, ctx && Y && R && state && workspace, VMP_ERR_INVALID, "null argument");
    VMP_REQUIRE(ctx, !from_labels || labels, VMP_ERR_INVALID, "null labels");
    VMP_REQUIRE(ctx, D >= 1 && K >= 1 && N >= 0, VMP_ERR_INVALID, "bad dims");
    VMP_REQUIRE(ctx, D <= HD_MAXD && K <= HD_MAXK, VMP_ERR_UNSUPPORTED,
                "high-dimensional fused GMM block supports D <= %d, K <= %d (got D=%d, K=%d)",
                HD_MAXD, HD_MAXK, D, K);
    vmp_gmm_layout L;
    hd_fill_layout(D, K, &L);
    const int DT = (int)(L.DP / 16), KT = (int)(L.KP / 16);
    // workspace: [sum lse partials of the responsibility kernel | partials of the second moments]
    double *Plse = reinterpret_cast<double *>(workspace);
    double *P = Plse + (hd_max_grid(ctx) + 7) / 8 * 8;
    const double *C = state + L.off_C;
    hipStream_t s = ctx->stream;
    hipEvent_t *ev = ctx->timing ? vmp_next_events(ctx) : nullptr;
    if (ev) VMP_HIP_CHECK(ctx, hipEventRecord(ev[0], s));
    int nb = 0, nchunk = 0;
    int32_t rc = VMP_OK;
    if (from_labels) {
        // one-hot responsibilities, bit-exact (categorical.py:30-46)
        int64_t g = (N * K + NT - 1) / NT;
        if (g > 4 * hd_max_grid(ctx)) g = 4 * hd_max_grid(ctx);
        if (g > 0)
            hipLaunchKernelGGL(gmm_hd_onehot_kernel, dim3((unsigned)g), dim3(NT), 0, s, labels, N,
                               K, R);
    } else if (DT == 1) rc = hd_launch_resp_k<1>(ctx, KT, Y, N, D, K, C, L.F2P, R, Plse, &nb);
    else if (DT == 2) rc = hd_launch_resp_k<2>(ctx, KT, Y, N, D, K, C, L.F2P, R, Plse, &nb);
    else if (DT == 3) rc = hd_launch_resp_k<3>(ctx, KT, Y, N, D, K, C, L.F2P, R, Plse, &nb);
    else rc = hd_launch_resp_k<4>(ctx, KT, Y, N, D, K, C, L.F2P, R, Plse, &nb);
    if (rc != VMP_OK) return rc;
    if (DT == 1) rc = hd_launch_s2<1>(ctx, Y, N, D, K, R, P, &nchunk);
    else if (DT == 2) rc = hd_launch_s2<2>(ctx, Y, N, D, K, R, P, &nchunk);
    else if (DT == 3) rc = hd_launch_s2<3>(ctx, Y, N, D, K, R, P, &nchunk);
    else rc = hd_launch_s2<4>(ctx, Y, N, D, K, R, P, &nchunk);
    if (rc != VMP_OK) return rc;
    if (ev) VMP_HIP_CHECK(ctx, hipEventRecord(ev[1], s));
    const int groups = (K + HD_NW2 - 1) / HD_NW2;
    hipLaunchKernelGGL(gmm_hd_reduce_kernel, dim3((unsigned)((L.FS + NT - 1) / NT), (unsigned)K),
                       dim3(NT), 0, s, L, D, P, nchunk, groups * HD_NW2, state);
    if (!from_labels)
        hipLaunchKernelGGL(gmm_hd_rphi_kernel, dim3(1), dim3(NTR), 0, s, L, K, Plse, nb, state);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    if (ev) VMP_HIP_CHECK(ctx, hipEventRecord(ev[2], s));
    return VMP_OK;
}

}  // namespace

extern "C" {

int32_t vmp_gmm_hd_get_layout(int32_t D, int32_t K, vmp_gmm_layout *out)
{
    if (!out || D < 1 || K < 1) return VMP_ERR_INVALID;
    if (D > HD_MAXD || K > HD_MAXK) return VMP_ERR_UNSUPPORTED;
    hd_fill_layout(D, K, out);
    return VMP_OK;
}

int32_t vmp_gmm_hd_workspace_bytes(vmp_ctx *ctx, int32_t D, int32_t K, size_t *bytes)
{
    VMP_REQUIRE(ctx, ctx && bytes, VMP_ERR_INVALID, "null argument");
    vmp_gmm_layout L;
    int32_t rc = vmp_gmm_hd_get_layout(D, K, &L);
    VMP_REQUIRE(ctx, rc == VMP_OK, rc, "high-dimensional fused GMM block supports D <= %d, K <= %d",
                HD_MAXD, HD_MAXK);
    *bytes = (size_t)((hd_max_grid(ctx) + 7) / 8 * 8 + hd_partial_doubles(ctx, K, L) + 64)
             * sizeof(double);
    return VMP_OK;
}

int32_t vmp_gmm_hd_init_state(vmp_ctx *ctx, int32_t D, int32_t K, const double *alpha0_host,
                              double beta0, double n0, const double *V0_host, double *state)
{
    VMP_REQUIRE(ctx, ctx && alpha0_host && V0_host && state, VMP_ERR_INVALID, "null argument");
    vmp_gmm_layout L;
    int32_t rc = vmp_gmm_hd_get_layout(D, K, &L);
    VMP_REQUIRE(ctx, rc == VMP_OK, rc, "high-dimensional fused GMM block supports D <= %d, K <= %d",
                HD_MAXD, HD_MAXK);
    VMP_REQUIRE(ctx, beta0 > 0 && n0 > D - 1, VMP_ERR_INVALID, "bad prior parameters");
    for (int k = 0; k < K; ++k)
        VMP_REQUIRE(ctx, alpha0_host[k] > 0, VMP_ERR_NOT_POSITIVE,
                    "Natural parameters should be positive");
    hipStream_t s = ctx->stream;
    VMP_HIP_CHECK(ctx, hipMemsetAsync(state, 0, (size_t)L.total * sizeof(double), s));
    double hdr[8] = {beta0, n0, 0, 0, 0, 0, 0, 0};
    VMP_HIP_CHECK(ctx, hipMemcpyAsync(state + L.off_prior, alpha0_host, K * sizeof(double),
                                      hipMemcpyHostToDevice, s));
    VMP_HIP_CHECK(ctx, hipMemcpyAsync(state + L.off_prior + L.KP, hdr, sizeof(hdr),
                                      hipMemcpyHostToDevice, s));
    VMP_HIP_CHECK(ctx, hipMemcpyAsync(state + L.off_prior + L.KP + 8, V0_host,
                                      (size_t)D * D * sizeof(double), hipMemcpyHostToDevice, s));
    VMP_HIP_CHECK(ctx, hipStreamSynchronize(s));   // host buffers may be temporaries
    hipLaunchKernelGGL(gmm_hd_init_state_kernel, dim3(K), dim3(NT), hd_cluster_lds(D), s, L, D, K,
                       beta0, n0, state);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_gmm_hd_stats_from_labels(vmp_ctx *ctx, const double *Y, int64_t N, int32_t D, int32_t K,
                                     const int64_t *labels, double *R, double *state,
                                     void *workspace)
{
    return hd_run_pass(ctx, true, Y, N, D, K, labels, R, state, workspace);
}

int32_t vmp_gmm_hd_pass(vmp_ctx *ctx, const double *Y, int64_t N, int32_t D, int32_t K, double *R,
                        double *state, void *workspace)
{
    return hd_run_pass(ctx, false, Y, N, D, K, nullptr, R, state, workspace);
}

#define VMP_GMM_HD_PROLOGUE()                                                        \
    VMP_REQUIRE(ctx, ctx && state, VMP_ERR_INVALID, "null argument");                \
    vmp_gmm_layout L;                                                                \
    {                                                                                \
        int32_t rc__ = vmp_gmm_hd_get_layout(D, K, &L);                              \
        VMP_REQUIRE(ctx, rc__ == VMP_OK, rc__, "unsupported dims D=%d K=%d", D, K);  \
    }

int32_t vmp_gmm_hd_update_mu(vmp_ctx *ctx, int32_t D, int32_t K, double *state)
{
    VMP_GMM_HD_PROLOGUE();
    hipLaunchKernelGGL(gmm_hd_update_mu_kernel, dim3(K), dim3(NT), hd_cluster_lds(D), ctx->stream,
                       L, D, K, state);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_gmm_hd_update_lambda(vmp_ctx *ctx, int32_t D, int32_t K, double *state)
{
    VMP_GMM_HD_PROLOGUE();
    hipLaunchKernelGGL(gmm_hd_update_lambda_kernel, dim3(K), dim3(NT), hd_cluster_lds(D),
                       ctx->stream, L, D, K, state);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_gmm_hd_prepare_z(vmp_ctx *ctx, int32_t D, int32_t K, int32_t prior_only, double *state)
{
    VMP_GMM_HD_PROLOGUE();
    hipLaunchKernelGGL(gmm_hd_prepare_z_kernel, dim3((unsigned)L.KP), dim3(NT), 0, ctx->stream, L,
                       D, K, (int)prior_only, state);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_gmm_hd_update_alpha(vmp_ctx *ctx, int32_t D, int32_t K, double *state)
{
    VMP_GMM_HD_PROLOGUE();
    return vmp_gmm_launch_update_alpha(ctx, L, D, K, state);
}

int32_t vmp_gmm_hd_lower_bound(vmp_ctx *ctx, int32_t D, int32_t K, double *state)
{
    VMP_GMM_HD_PROLOGUE();
    return vmp_gmm_launch_lower_bound_hd(ctx, L, D, K, state);
}

}  // extern "C"
