// vmp_lda_wide.hip -- the token pass of the latent-Dirichlet-allocation block for 65 .. 1024 topics
//
// The same two passes and the same contract as csrc/vmp_lda.hip (pass A in document order writes
// lse, N_dk and the per-chunk sum of lse; pass B in word order forms phi again from the same two
// addends and the stored lse and writes N_vk; phi is stored only on request; no floating-point
// atomics; segments that cross chunks go through head / tail partials and a combine kernel that
// adds them in chunk order and writes empty segments as zeros).  What differs is the layout
// (vmp_lda_wide_dev.h): one wavefront owns a chunk, lane j holds the topics j + 64 r in R registers,
// so a table row of K contiguous doubles is R coalesced loads of 512 bytes.
//
// Two things keep the traffic at one gathered row per token and pass:
//   * the row indexed by the SEGMENT (the document's row of <log theta> in pass A, the word's row
//     of <log beta>^T in pass B) stays in registers for the whole run of a segment and is loaded
//     again only when the segment changes;
//   * the gathered row of the NEXT token (indexed by `oth`) is requested before the exp / log
//     arithmetic of the present token; the indices run one token further ahead, as in the narrow
//     pass, and so does the stored lse that pass B reads through `pos`.
// Neither changes a bit of any output.  The chunk size is a function of n alone, so the bits of
// every output depend on (inputs, n, K, layouts) only.
#include "vmp_common.h"
#include "vmp_lda_wide_dev.h"

namespace {

constexpr int LDAW_NT = 256;         // four wavefronts = four chunks per workgroup
constexpr int LDAW_RED_NT = 1024;    // the one workgroup that adds the chunk sums in index order
constexpr int LDAW_MAX_PART = 1024;  // partial sums of vmp_lda_dot

__device__ __forceinline__ double wave_max_bfly(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ double wave_sum_bfly(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

struct WideArgs {
    int64_t n;
    int64_t nchunks;
    int K, T;
    const int32_t *seg;        // segment of token i in walk order (document in A, word in B)
    const int32_t *oth;        // its other index (word in A, document in B)
    const int64_t *seg_off;    // first token of every segment, and n
    const int32_t *pos;        // pass B: where token i stands in document order; null = pass A
    const int32_t *labels;     // fixed topics in document order (phi = one-hot, lse = 0) or null
    const double *Tseg;        // table rows indexed by seg; null = no such term
    const double *Toth;        // table rows indexed by oth; null = no such term
    double *lse;               // document order: written by A, read by B
    double *N;                 // segments x K
    double *head, *tail;       // chunks x K
    double *chunk_lse;         // pass A: sum of lse over the chunk
    const int32_t *orig;       // pass A, with phi: position of token i in the caller's order
    double *phi;               // n x K in the caller's order, or null
};

// a wave-uniform value as a scalar
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// row `idx` of a table of K contiguous doubles as R registers per lane; kc is the lane's topic per
// register, clamped into the row (the caller drops what lies beyond K)
template <int R>
__device__ __forceinline__ void load_row(double (&dst)[R], const double *__restrict__ table,
                                         int idx, int K, const int (&kc)[R])
{
    if (table) {
        const double *row = table + (int64_t)idx * K;
#pragma unroll
        for (int r = 0; r < R; ++r) dst[r] = row[kc[r]];
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) dst[r] = 0.0;
    }
}

template <int R>
__global__ void __launch_bounds__(LDAW_NT) lda_wide_pass_kernel(WideArgs a)
{
    const int64_t c = ((int64_t)blockIdx.x * LDAW_NT + threadIdx.x) / VMP_LDA_WIDE_LANES;
    const int lane = threadIdx.x & (VMP_LDA_WIDE_LANES - 1);
    if (c >= a.nchunks) return;                  // whole wavefronts leave together
    const int K = a.K;
    bool act[R];
    int kc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int k = lane + VMP_LDA_WIDE_LANES * r;
        act[r] = k < K;
        kc[r] = act[r] ? k : K - 1;
    }
    const int64_t cs = c * a.T;
    const int64_t ce = (cs + a.T < a.n) ? cs + a.T : a.n;
    const bool passA = a.pos == nullptr;
    const bool tables = a.labels == nullptr;     // fixed labels read no table
    int cur = uni(a.seg[cs]);
    bool inside = a.seg_off[cur] >= cs;          // the first run began in this chunk
    double acc[R], row[R], g[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0;
    double lsum = 0.0;
    // token i: (s, o, li), its gathered row g and (pass B) its stored lse; token i + 1: (s1, o1, li1)
    const int64_t i1 = (cs + 1 < ce) ? cs + 1 : cs;
    int s = cur, o = uni(a.oth[cs]);
    int s1 = uni(a.seg[i1]), o1 = uni(a.oth[i1]);
    int li = passA ? (int)cs : uni(a.pos[cs]);
    int li1 = passA ? (int)i1 : uni(a.pos[i1]);
    double lcur = 0.0;
    if (tables) {
        load_row<R>(row, a.Tseg, s, K, kc);
        load_row<R>(g, a.Toth, o, K, kc);
        if (!passA) lcur = a.lse[li];
    }
    for (int64_t i = cs; i < ce; ++i) {
        // indices of token i + 2 and the gathered row of token i + 1: issued before this token's
        // arithmetic
        const int64_t i2 = (i + 2 < ce) ? i + 2 : ce - 1;
        const int s2 = uni(a.seg[i2]), o2 = uni(a.oth[i2]);
        const int li2 = passA ? (int)i2 : uni(a.pos[i2]);
        double gn[R], lnext = 0.0;
        if (tables) {
            load_row<R>(gn, a.Toth, o1, K, kc);
            if (!passA) lnext = a.lse[li1];
        }
        if (s != cur) {
            double *dst = inside ? a.N + (int64_t)cur * K : a.head + c * K;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (act[r]) dst[lane + VMP_LDA_WIDE_LANES * r] = acc[r];
                acc[r] = 0.0;
            }
            cur = s;
            inside = true;
            if (tables) load_row<R>(row, a.Tseg, s, K, kc);   // kept until the segment changes
        }
        double p[R];
        if (!tables) {
            const int lab = a.labels[li];
#pragma unroll
            for (int r = 0; r < R; ++r)
                p[r] = (lane + VMP_LDA_WIDE_LANES * r == lab) ? 1.0 : 0.0;
            if (passA && lane == 0) a.lse[i] = 0.0;
        } else {
            double l[R];
#pragma unroll
            for (int r = 0; r < R; ++r)
                l[r] = act[r] ? vmp_lda_logit(row[r], g[r]) : -INFINITY;
            double lse;
            if (passA) {
                double m = l[0];
#pragma unroll
                for (int r = 1; r < R; ++r) m = fmax(m, l[r]);
                m = wave_max_bfly(m);
                double sum = act[0] ? vmp_lda_shifted_exp(l[0], m) : 0.0;
#pragma unroll
                for (int r = 1; r < R; ++r) sum += act[r] ? vmp_lda_shifted_exp(l[r], m) : 0.0;
                lse = vmp_lda_lse(m, wave_sum_bfly(sum));
                if (lane == 0) a.lse[i] = lse;
                lsum += lse;
            } else {
                lse = lcur;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) p[r] = act[r] ? vmp_lda_phi(l[r], lse) : 0.0;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] += p[r];
        if (a.phi) {
            double *dst = a.phi + (int64_t)a.orig[i] * K;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (act[r]) dst[lane + VMP_LDA_WIDE_LANES * r] = p[r];
        }
        s = s1;
        o = o1;
        li = li1;
        s1 = s2;
        o1 = o2;
        li1 = li2;
        lcur = lnext;
        if (tables) {
#pragma unroll
            for (int r = 0; r < R; ++r) g[r] = gn[r];
        }
    }
    const bool ends = a.seg_off[cur + 1] <= ce;  // the last run ends in this chunk
    double *dst = (inside && ends) ? a.N + (int64_t)cur * K
                                   : (!inside ? a.head + c * K : a.tail + c * K);
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (act[r]) dst[lane + VMP_LDA_WIDE_LANES * r] = acc[r];
    if (passA && lane == 0) a.chunk_lse[c] = lsum;
}

// the combine step of csrc/vmp_lda.hip, restated: one thread per (segment, topic) -- zeros for an
// empty segment, the partials of a segment that crosses chunks in chunk order; a segment inside
// one chunk was written by the pass
__global__ void __launch_bounds__(LDAW_NT)
lda_wide_combine_kernel(int64_t nseg, int K, int T, const int64_t *__restrict__ seg_off,
                        const double *__restrict__ head, const double *__restrict__ tail,
                        double *__restrict__ N)
{
    const int64_t idx = (int64_t)blockIdx.x * LDAW_NT + threadIdx.x;
    if (idx >= nseg * K) return;
    const int64_t s = idx / K;
    const int k = (int)(idx - s * K);
    const int64_t b = seg_off[s], e = seg_off[s + 1];
    if (b == e) {
        N[idx] = 0.0;
        return;
    }
    const int64_t c0 = b / T, c1 = (e - 1) / T;
    if (c0 == c1) return;
    double sum = tail[c0 * K + k];
    for (int64_t c = c0 + 1; c < c1; ++c) sum += head[c * K + k];
    sum += head[c1 * K + k];
    N[idx] = sum;
}

__global__ void __launch_bounds__(LDAW_RED_NT)
lda_wide_sum_final_kernel(int64_t cnt, const double *__restrict__ x, double *__restrict__ out)
{
    __shared__ double red[LDAW_RED_NT / 64];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < cnt; i += LDAW_RED_NT) v += x[i];
    v = block_sum<LDAW_RED_NT>(v, red);
    if (threadIdx.x == 0) out[0] = v;
}

inline int64_t chunks_of(int64_t n, int T) { return n > 0 ? (n + T - 1) / T : 0; }

template <int R>
void launch_pass_r(vmp_ctx *ctx, const WideArgs &a)
{
    const int64_t waves_per_block = LDAW_NT / VMP_LDA_WIDE_LANES;
    const int64_t grid = (a.nchunks + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL(lda_wide_pass_kernel<R>, dim3((unsigned)grid), dim3(LDAW_NT), 0, ctx->stream,
                       a);
}

void launch_pass(vmp_ctx *ctx, const WideArgs &a)
{
    switch (vmp_lda_wide_regs(a.K)) {
    case 2: launch_pass_r<2>(ctx, a); break;
    case 4: launch_pass_r<4>(ctx, a); break;
    case 8: launch_pass_r<8>(ctx, a); break;
    default: launch_pass_r<16>(ctx, a); break;
    }
}

void launch_combine(vmp_ctx *ctx, int64_t nseg, int K, int T, const int64_t *off,
                    const double *head, const double *tail, double *N)
{
    const int64_t tot = nseg * K;
    if (tot == 0) return;
    hipLaunchKernelGGL(lda_wide_combine_kernel, dim3((unsigned)((tot + LDAW_NT - 1) / LDAW_NT)),
                       dim3(LDAW_NT), 0, ctx->stream, nseg, K, T, off, head, tail, N);
}

}  // namespace

extern "C" {

int32_t vmp_lda_wide_limits(int32_t *min_K, int32_t *max_K, int32_t *max_chunk)
{
    if (!min_K || !max_K || !max_chunk) return VMP_ERR_INVALID;
    *min_K = VMP_LDA_WIDE_MIN_K;
    *max_K = VMP_LDA_WIDE_MAX_K;
    *max_chunk = 256;
    return VMP_OK;
}

int32_t vmp_lda_wide_plan(int64_t n, int32_t K, int32_t *regs, int32_t *chunk,
                          int64_t *workspace_doubles)
{
    if (n < 0 || !regs || !chunk || !workspace_doubles) return VMP_ERR_INVALID;
    if (K < VMP_LDA_WIDE_MIN_K || K > VMP_LDA_WIDE_MAX_K || n > 0x7fffffffLL)
        return VMP_ERR_UNSUPPORTED;
    *regs = vmp_lda_wide_regs(K);
    *chunk = vmp_lda_wide_chunk_tokens(n);
    *workspace_doubles = chunks_of(n, *chunk) * (2 * (int64_t)K + 1) + LDAW_MAX_PART;
    return VMP_OK;
}

int32_t vmp_lda_wide_token_pass(vmp_ctx *ctx, int64_t n, int64_t D, int64_t V, int32_t K,
                                const int32_t *doc_d, const int32_t *word_d,
                                const int64_t *doc_off, const int32_t *word_w,
                                const int32_t *doc_w, const int32_t *pos_w,
                                const int64_t *word_off, const int32_t *labels,
                                const double *elog_theta, const double *elog_beta_t,
                                int32_t phases, double *lse, double *ws, double *Ndk, double *Nvk,
                                double *scal, const int32_t *orig, double *phi)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && n >= 0 && D >= 0 && V >= 0 && K >= 1 && phases >= 0 && phases <= 7,
                VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K >= VMP_LDA_WIDE_MIN_K && K <= VMP_LDA_WIDE_MAX_K, VMP_ERR_UNSUPPORTED,
                "K = %d is outside %d .. %d (vmp_lda_token_pass takes K <= 64)", K,
                VMP_LDA_WIDE_MIN_K, VMP_LDA_WIDE_MAX_K);
    VMP_REQUIRE(ctx, n <= 0x7fffffffLL, VMP_ERR_UNSUPPORTED, "more than 2^31 - 1 tokens");
    VMP_REQUIRE(ctx, doc_off && word_off && ws && Ndk && Nvk && scal && elog_theta,
                VMP_ERR_INVALID, "null argument");
    VMP_REQUIRE(ctx, n == 0 || (doc_d && word_d && word_w && doc_w && pos_w && lse),
                VMP_ERR_INVALID, "null argument");
    VMP_REQUIRE(ctx, (phi == nullptr) == (orig == nullptr), VMP_ERR_INVALID,
                "phi and orig go together");
    VMP_REQUIRE(ctx, n == 0 || (D >= 1 && V >= 1), VMP_ERR_INVALID, "tokens without segments");
    const int T = vmp_lda_wide_chunk_tokens(n);
    const int64_t nc = chunks_of(n, T);
    double *head = ws, *tail = ws + nc * K, *chunk_lse = ws + 2 * nc * K;
    double *partial = chunk_lse + nc;
    const bool prior_only = elog_beta_t == nullptr;
    if (phases & 1) {
        if (n > 0) {
            WideArgs a = {n, nc, K, T, doc_d, word_d, doc_off, nullptr, labels, elog_theta,
                          elog_beta_t, lse, Ndk, head, tail, chunk_lse, orig, phi};
            launch_pass(ctx, a);
        }
        launch_combine(ctx, D, K, T, doc_off, head, tail, Ndk);
        if (n > 0) {
            hipLaunchKernelGGL(lda_wide_sum_final_kernel, dim3(1), dim3(LDAW_RED_NT), 0,
                               ctx->stream, nc, chunk_lse, scal);
        } else {
            VMP_HIP_CHECK(ctx, hipMemsetAsync(scal, 0, sizeof(double), ctx->stream));
        }
    }
    if (phases & 2) {
        if (n > 0) {
            // without the word table the logits are the document rows alone (read through `oth`)
            WideArgs b = {n, nc, K, T, word_w, doc_w, word_off, pos_w, labels, elog_beta_t,
                          elog_theta, lse, Nvk, head, tail, chunk_lse, nullptr, nullptr};
            launch_pass(ctx, b);
        }
        launch_combine(ctx, V, K, T, word_off, head, tail, Nvk);
    }
    VMP_HIP_CHECK(ctx, hipGetLastError());
    if (phases & 4) {
        // the dot products are general in their length: the entry point of the narrow block
        int32_t rc = vmp_lda_dot(ctx, D * K, Ndk, elog_theta, partial, scal + 1);
        if (rc != VMP_OK) return rc;
        if (prior_only) {
            VMP_HIP_CHECK(ctx, hipMemsetAsync(scal + 2, 0, sizeof(double), ctx->stream));
        } else {
            rc = vmp_lda_dot(ctx, V * K, Nvk, elog_beta_t, partial, scal + 2);
            if (rc != VMP_OK) return rc;
        }
    }
    return VMP_OK;
}

}  // extern "C"
