// vmp_lda.hip -- the token pass of the fused latent-Dirichlet-allocation block
//
//     p_topic = Dirichlet(a, plates=(D,));  p_word = Dirichlet(b, plates=(K,))
//     topics  = Categorical(Gate(document_indices, p_topic), plates=(n,))
//     words   = Categorical(Gate(topics, p_word));  words.observe(corpus)
//
// (doc/source/examples/lda.rst; the reference forms tokens x documents, tokens x vocabulary and
// tokens x topics arrays for it, gate.py:20-205, categorical.py:30-46).  Here a sweep over the
// tokens is an integer-indexed gather, a softmax over the topics and two segmented sums:
//
//   pass A  walks the tokens in DOCUMENT order: l_k = <log theta>[d, k] + <log beta>^T[w, k],
//           lse over the lane group, phi_k = exp(l_k - lse); writes lse (8 B per token) and the
//           document x topic counts N_dk = sum over the document's tokens of phi;
//   pass B  walks the tokens in WORD order, forms phi again from the same two addends and the
//           stored lse (the same bits as in pass A) and sums the word x topic counts N_vk.
//
// phi is never stored (2 * 8 * K bytes per token).  Both tables are read as rows of K contiguous
// doubles (<log beta> is kept transposed, V x K).
//
// No floating-point atomics.  A lane group (vmp_lda_dev.h) walks a CHUNK of consecutive tokens in
// order; a segment (document / word) that lies inside one chunk is summed there in token order and
// written once.  A segment that crosses chunks leaves one partial per chunk (`head`: the run that
// came in from the previous chunk, `tail`: the run that goes on into the next), and a second
// kernel adds them per segment in chunk order.  The chunk size depends on (n, K) alone, so the bits
// of every output depend on (inputs, n, K, layouts) only.  Empty segments are written as zeros by
// the second kernel; nothing needs clearing beforehand.
#include "vmp_common.h"
#include "vmp_lda_dev.h"
#include "vmp_table_dev.h"

namespace {

constexpr int LDA_NT = VMP_TABLE_NT; // token pass, combine kernel, dot partials, Dirichlet rows
constexpr int LDA_RED_NT = 1024;     // the one workgroup that adds partial sums in index order
constexpr int LDA_MAX_K = 64;
constexpr int LDA_MAX_PART = 1024;   // partial sums of a dot product

template <int G>
__device__ __forceinline__ double group_max(double v)
{
#pragma unroll
    for (int off = G >> 1; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

template <int G>
__device__ __forceinline__ double group_sum(double v)
{
#pragma unroll
    for (int off = G >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

struct PassArgs {
    int64_t n;
    int64_t nchunks;
    int K, T;
    const int32_t *seg;        // segment of token i in walk order (document in A, word in B)
    const int32_t *oth;        // its other index (word in A, document in B)
    const int64_t *seg_off;    // first token of every segment, and n
    const int32_t *pos;        // pass B: where token i stands in document order; null = pass A
    const int32_t *labels;     // fixed topics in document order (phi = one-hot, lse = 0) or null
    const double *Tseg;        // table rows indexed by seg; null = no such term
    const double *Toth;        // table rows indexed by oth; null = no such term (prior only: the
                               // word table is missing in both passes)
    double *lse;               // document order: written by A, read by B
    double *N;                 // segments x K
    double *head, *tail;       // chunks x K
    double *chunk_lse;         // pass A: sum of lse over the chunk
    const int32_t *orig;       // pass A, with phi: position of token i in the caller's order
    double *phi;               // n x K in the caller's order, or null
};

template <int G>
__global__ void __launch_bounds__(LDA_NT) lda_pass_kernel(PassArgs a)
{
    const int64_t c = ((int64_t)blockIdx.x * LDA_NT + threadIdx.x) / G;
    const int k = threadIdx.x & (G - 1);
    if (c >= a.nchunks) return;                  // whole lane groups leave together
    const int K = a.K;
    const bool act = k < K;
    const int64_t cs = c * a.T;
    const int64_t ce = (cs + a.T < a.n) ? cs + a.T : a.n;
    const bool passA = a.pos == nullptr;
    int cur = a.seg[cs];
    bool inside = a.seg_off[cur] >= cs;          // the first run began in this chunk
    double acc = 0.0, lsum = 0.0;
    int s = cur, o = a.oth[cs];
    for (int64_t i = cs; i < ce; ++i) {
        // indices of the next token: issued before this token's arithmetic
        const int64_t inext = (i + 1 < ce) ? i + 1 : i;
        const int sn = a.seg[inext], on = a.oth[inext];
        if (s != cur) {
            if (act) (inside ? a.N + (int64_t)cur * K : a.head + c * K)[k] = acc;
            acc = 0.0;
            cur = s;
            inside = true;
        }
        const int64_t li = passA ? i : (int64_t)a.pos[i];
        double p;
        if (a.labels) {
            p = (k == a.labels[li]) ? 1.0 : 0.0;
            if (passA && k == 0) a.lse[i] = 0.0;
        } else {
            double logit = -INFINITY;
            if (act)
                logit = vmp_lda_logit(a.Tseg ? a.Tseg[(int64_t)s * K + k] : 0.0,
                                      a.Toth ? a.Toth[(int64_t)o * K + k] : 0.0);
            double l;
            if (passA) {
                const double m = group_max<G>(logit);
                const double e = act ? vmp_lda_shifted_exp(logit, m) : 0.0;
                l = vmp_lda_lse(m, group_sum<G>(e));
                if (k == 0) a.lse[i] = l;
                lsum += l;
            } else {
                l = a.lse[li];
            }
            p = act ? vmp_lda_phi(logit, l) : 0.0;
        }
        acc += p;
        if (a.phi && act) a.phi[(int64_t)a.orig[i] * K + k] = p;
        s = sn;
        o = on;
    }
    const bool ends = a.seg_off[cur + 1] <= ce;  // the last run ends in this chunk
    if (act) {
        double *dst = (inside && ends) ? a.N + (int64_t)cur * K
                                       : (!inside ? a.head + c * K : a.tail + c * K);
        dst[k] = acc;
    }
    if (passA && k == 0) a.chunk_lse[c] = lsum;
}

// one thread per (segment, topic): zeros for an empty segment, the partials of a segment that
// crosses chunks in chunk order; a segment inside one chunk was written by the pass
__global__ void __launch_bounds__(LDA_NT)
lda_combine_kernel(int64_t nseg, int K, int T, const int64_t *__restrict__ seg_off,
                   const double *__restrict__ head, const double *__restrict__ tail,
                   double *__restrict__ N)
{
    const int64_t idx = (int64_t)blockIdx.x * LDA_NT + threadIdx.x;
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

// partial[j] = sum over slice j of a * b (b null: of a); slices are contiguous, the grid is a
// function of m alone
__global__ void __launch_bounds__(LDA_NT)
lda_dot_partial_kernel(int64_t m, int64_t slice, const double *__restrict__ a,
                       const double *__restrict__ b, double *__restrict__ partial)
{
    __shared__ double red[LDA_NT / 64];
    const int64_t lo = (int64_t)blockIdx.x * slice;
    const int64_t hi = (lo + slice < m) ? lo + slice : m;
    double v = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += LDA_NT) v += b ? a[i] * b[i] : a[i];
    v = block_sum<LDA_NT>(v, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

__global__ void __launch_bounds__(LDA_RED_NT)
lda_sum_final_kernel(int64_t cnt, const double *__restrict__ x, double *__restrict__ out)
{
    __shared__ double red[LDA_RED_NT / 64];
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < cnt; i += LDA_RED_NT) v += x[i];
    v = block_sum<LDA_RED_NT>(v, red);
    if (threadIdx.x == 0) out[0] = v;
}

// Dirichlet rows with few columns: one thread per row (vmp_table_dev.h).  STEP: alpha moves by
// vmp_table_step_value instead of being set to prior + counts.
template <bool STEP>
__global__ void __launch_bounds__(LDA_NT)
lda_dirichlet_rows_kernel(int64_t rows, int cols, int64_t rs, int64_t cs,
                          const double *__restrict__ prior, const double *__restrict__ counts,
                          double mult, double scale, double *alpha, double *__restrict__ elog,
                          double *__restrict__ rowL)
{
    const int64_t r = (int64_t)blockIdx.x * LDA_NT + threadIdx.x;
    if (r >= rows) return;
    rowL[r] = vmp_dirichlet_row_thread<STEP>(r, cols, rs, cs, prior, counts, mult, scale, alpha,
                                             elog);
}

// Dirichlet rows with many columns: one workgroup per row
template <bool STEP>
__global__ void __launch_bounds__(LDA_NT)
lda_dirichlet_wide_kernel(int64_t cols, int64_t rs, int64_t cs, const double *__restrict__ prior,
                          const double *__restrict__ counts, double mult, double scale,
                          double *alpha, double *__restrict__ elog, double *__restrict__ rowL)
{
    __shared__ double red[LDA_NT / 64];
    const int64_t r = blockIdx.x;
    const double L = vmp_dirichlet_row_block<STEP, LDA_NT>(r, cols, rs, cs, prior, counts, mult,
                                                           scale, alpha, elog, red);
    if (threadIdx.x == 0) rowL[r] = L;
}

// -- the step on a transposed table ------------------------------------------------------------------
// `p_word` is kept as V x K (vocabulary entry c, topic r at c * K + r): the Dirichlet rows run down
// the strided axis, the memory along K.  A workgroup owns `cpb` consecutive vocabulary entries, i.e.
// one contiguous piece of cpb * K doubles, and walks it with the first per * K of its threads
// (per = LDA_NT / K whole vocabulary entries per sweep): consecutive lanes touch consecutive
// doubles and a thread keeps the topic r = t % K throughout, so its running sums belong to one
// Dirichlet row.  The grid is a function of (V, K) alone and every sum has a fixed order.
constexpr int LDA_T_MAX_BLOCKS = 2048;
constexpr int LDA_T_MIN_SWEEPS = 4;

struct TGrid {
    int per;            // vocabulary entries per sweep of a workgroup
    int64_t cpb, nb;    // vocabulary entries per workgroup, workgroups
};

inline TGrid lda_t_grid(int64_t V, int K)
{
    TGrid g;
    g.per = LDA_NT / K;
    g.cpb = (V + LDA_T_MAX_BLOCKS - 1) / LDA_T_MAX_BLOCKS;
    if (g.cpb < (int64_t)LDA_T_MIN_SWEEPS * g.per) g.cpb = (int64_t)LDA_T_MIN_SWEEPS * g.per;
    g.nb = (V + g.cpb - 1) / g.cpb;
    return g;
}

// ws of the transposed step: [nb] bound partials, [K] row constants, [K] psi(row sum),
// [nb x 2 x K] partial row sums of alpha and of the prior
inline int64_t lda_t_ws_doubles(int64_t V, int K)
{
    const TGrid g = lda_t_grid(V, K);
    return g.nb + 2 * (int64_t)K + 2 * g.nb * K;
}

// first pass: alpha, and per workgroup the partial sums over its vocabulary entries
__global__ void __launch_bounds__(LDA_NT)
lda_step_t_alpha_kernel(int64_t V, int K, int64_t cpb, const double *__restrict__ prior,
                        const double *__restrict__ counts, double mult, double scale,
                        double *alpha, double *__restrict__ part)
{
    __shared__ double sh[2][LDA_NT];
    const int t = threadIdx.x;
    const int per = LDA_NT / K;
    const int64_t c0 = (int64_t)blockIdx.x * cpb;
    const int64_t c1 = (c0 + cpb < V) ? c0 + cpb : V;
    double s = 0.0, s0 = 0.0;
    if (t < per * K) {
        const int64_t end = c1 * K, stride = (int64_t)per * K;
        for (int64_t e = c0 * K + t; e < end; e += stride) {
            const double p = prior[e];
            const double v = vmp_table_step_value(p, counts, e, mult, scale, alpha);
            alpha[e] = v;
            s += v;
            s0 += p;
        }
    }
    sh[0][t] = s;
    sh[1][t] = s0;
    __syncthreads();
    if (t < K) {
        double a = 0.0, b = 0.0;
        for (int i = 0; i < per; ++i) {
            a += sh[0][t + i * K];
            b += sh[1][t + i * K];
        }
        part[((int64_t)blockIdx.x * 2) * K + t] = a;
        part[((int64_t)blockIdx.x * 2 + 1) * K + t] = b;
    }
}

// one workgroup per Dirichlet row: the partials in a fixed order, then what the second pass needs
// of the row sums
__global__ void __launch_bounds__(LDA_NT)
lda_step_t_combine_kernel(int64_t nb, int K, const double *__restrict__ part,
                          double *__restrict__ rowc, double *__restrict__ psis)
{
    __shared__ double red[LDA_NT / 64];
    const int r = blockIdx.x;
    double s = 0.0, s0 = 0.0;
    for (int64_t b = threadIdx.x; b < nb; b += LDA_NT) {
        s += part[(b * 2) * K + r];
        s0 += part[(b * 2 + 1) * K + r];
    }
    s = block_sum<LDA_NT>(s, red);
    s0 = block_sum<LDA_NT>(s0, red);
    if (threadIdx.x == 0) {
        psis[r] = vmp_digamma(s);
        rowc[r] = vmp_lgamma(s0) - vmp_lgamma(s);
    }
}

// second pass: <log> and the partial sums of the bound
__global__ void __launch_bounds__(LDA_NT)
lda_step_t_elog_kernel(int64_t V, int K, int64_t cpb, const double *__restrict__ prior,
                       const double *__restrict__ alpha, const double *__restrict__ psis,
                       double *__restrict__ elog, double *__restrict__ bpart)
{
    __shared__ double red[LDA_NT / 64];
    const int t = threadIdx.x;
    const int per = LDA_NT / K;
    const int64_t c0 = (int64_t)blockIdx.x * cpb;
    const int64_t c1 = (c0 + cpb < V) ? c0 + cpb : V;
    double g = 0.0, g0 = 0.0, L = 0.0;
    if (t < per * K) {
        const double psi_row = psis[t % K];
        const int64_t end = c1 * K, stride = (int64_t)per * K;
        for (int64_t e = c0 * K + t; e < end; e += stride) {
            const double p = prior[e], v = alpha[e];
            const double el = vmp_digamma(v) - psi_row;
            elog[e] = el;
            g += vmp_lgamma(v);
            g0 += vmp_lgamma(p);
            L += (p - v) * el;
        }
    }
    g = block_sum<LDA_NT>(g, red);
    g0 = block_sum<LDA_NT>(g0, red);
    L = block_sum<LDA_NT>(L, red);
    if (t == 0) bpart[blockIdx.x] = L + (g - g0);
}

inline int64_t chunks_of(int64_t n, int T) { return n > 0 ? (n + T - 1) / T : 0; }

template <int G>
void launch_pass_g(vmp_ctx *ctx, const PassArgs &a)
{
    const int64_t groups_per_block = LDA_NT / G;
    const int64_t grid = (a.nchunks + groups_per_block - 1) / groups_per_block;
    hipLaunchKernelGGL(lda_pass_kernel<G>, dim3((unsigned)grid), dim3(LDA_NT), 0, ctx->stream, a);
}

void launch_pass(vmp_ctx *ctx, const PassArgs &a)
{
    switch (vmp_lda_group(a.K)) {
    case 1: launch_pass_g<1>(ctx, a); break;
    case 2: launch_pass_g<2>(ctx, a); break;
    case 4: launch_pass_g<4>(ctx, a); break;
    case 8: launch_pass_g<8>(ctx, a); break;
    case 16: launch_pass_g<16>(ctx, a); break;
    case 32: launch_pass_g<32>(ctx, a); break;
    default: launch_pass_g<64>(ctx, a); break;
    }
}

void launch_combine(vmp_ctx *ctx, int64_t nseg, int K, int T, const int64_t *off,
                    const double *head, const double *tail, double *N)
{
    const int64_t tot = nseg * K;
    if (tot == 0) return;
    hipLaunchKernelGGL(lda_combine_kernel, dim3((unsigned)((tot + LDA_NT - 1) / LDA_NT)),
                       dim3(LDA_NT), 0, ctx->stream, nseg, K, T, off, head, tail, N);
}

// out[0] = sum a * b over m elements in a fixed order (b null: sum a); `partial`: LDA_MAX_PART
void launch_dot(vmp_ctx *ctx, int64_t m, const double *a, const double *b, double *partial,
                double *out)
{
    int64_t parts = (m + 4095) / 4096;
    if (parts < 1) parts = 1;
    if (parts > LDA_MAX_PART) parts = LDA_MAX_PART;
    const int64_t slice = (m + parts - 1) / parts;
    hipLaunchKernelGGL(lda_dot_partial_kernel, dim3((unsigned)parts), dim3(LDA_NT), 0, ctx->stream,
                       m, slice, a, b, partial);
    hipLaunchKernelGGL(lda_sum_final_kernel, dim3(1), dim3(LDA_RED_NT), 0, ctx->stream, parts,
                       partial, out);
}

}  // namespace

extern "C" {

int32_t vmp_lda_limits(int32_t *max_K, int32_t *max_chunk)
{
    if (!max_K || !max_chunk) return VMP_ERR_INVALID;
    *max_K = LDA_MAX_K;
    *max_chunk = 256;
    return VMP_OK;
}

int32_t vmp_lda_plan(int64_t n, int32_t K, int32_t *group, int32_t *chunk,
                     int64_t *workspace_doubles)
{
    if (n < 0 || K < 1 || !group || !chunk || !workspace_doubles) return VMP_ERR_INVALID;
    if (K > LDA_MAX_K || n > 0x7fffffffLL) return VMP_ERR_UNSUPPORTED;
    *group = vmp_lda_group(K);
    *chunk = vmp_lda_chunk_tokens(n, K);
    *workspace_doubles = chunks_of(n, *chunk) * (2 * (int64_t)K + 1) + LDA_MAX_PART;
    return VMP_OK;
}

int32_t vmp_lda_token_pass(vmp_ctx *ctx, int64_t n, int64_t D, int64_t V, int32_t K,
                           const int32_t *doc_d, const int32_t *word_d, const int64_t *doc_off,
                           const int32_t *word_w, const int32_t *doc_w, const int32_t *pos_w,
                           const int64_t *word_off, const int32_t *labels,
                           const double *elog_theta, const double *elog_beta_t, int32_t phases,
                           double *lse, double *ws, double *Ndk, double *Nvk, double *scal,
                           const int32_t *orig, double *phi)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && n >= 0 && D >= 0 && V >= 0 && K >= 1 && phases >= 0 && phases <= 7,
                VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, K <= LDA_MAX_K, VMP_ERR_UNSUPPORTED, "K = %d exceeds the limit %d", K,
                LDA_MAX_K);
    VMP_REQUIRE(ctx, n <= 0x7fffffffLL, VMP_ERR_UNSUPPORTED, "more than 2^31 - 1 tokens");
    VMP_REQUIRE(ctx, doc_off && word_off && ws && Ndk && Nvk && scal && elog_theta,
                VMP_ERR_INVALID, "null argument");
    VMP_REQUIRE(ctx, n == 0 || (doc_d && word_d && word_w && doc_w && pos_w && lse),
                VMP_ERR_INVALID, "null argument");
    VMP_REQUIRE(ctx, (phi == nullptr) == (orig == nullptr), VMP_ERR_INVALID,
                "phi and orig go together");
    VMP_REQUIRE(ctx, n == 0 || (D >= 1 && V >= 1), VMP_ERR_INVALID, "tokens without segments");
    const int T = vmp_lda_chunk_tokens(n, K);
    const int64_t nc = chunks_of(n, T);
    double *head = ws, *tail = ws + nc * K, *chunk_lse = ws + 2 * nc * K;
    double *partial = chunk_lse + nc;
    const bool prior_only = elog_beta_t == nullptr;
    if (phases & 1) {
        if (n > 0) {
            PassArgs a = {n, nc, K, T, doc_d, word_d, doc_off, nullptr, labels, elog_theta,
                          elog_beta_t, lse, Ndk, head, tail, chunk_lse, orig, phi};
            launch_pass(ctx, a);
        }
        launch_combine(ctx, D, K, T, doc_off, head, tail, Ndk);
        if (n > 0) {
            hipLaunchKernelGGL(lda_sum_final_kernel, dim3(1), dim3(LDA_RED_NT), 0, ctx->stream, nc,
                               chunk_lse, scal);
        } else {
            VMP_HIP_CHECK(ctx, hipMemsetAsync(scal, 0, sizeof(double), ctx->stream));
        }
    }
    if (phases & 2) {
        if (n > 0) {
            // without the word table the logits are the document rows alone (read through `oth`)
            PassArgs b = {n, nc, K, T, word_w, doc_w, word_off, pos_w, labels, elog_beta_t,
                          elog_theta, lse, Nvk, head, tail, chunk_lse, nullptr, nullptr};
            launch_pass(ctx, b);
        }
        launch_combine(ctx, V, K, T, word_off, head, tail, Nvk);
    }
    if (phases & 4) {
        launch_dot(ctx, D * K, Ndk, elog_theta, partial, scal + 1);
        if (prior_only)
            VMP_HIP_CHECK(ctx, hipMemsetAsync(scal + 2, 0, sizeof(double), ctx->stream));
        else
            launch_dot(ctx, V * K, Nvk, elog_beta_t, partial, scal + 2);
    }
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_lda_dirichlet(vmp_ctx *ctx, int64_t rows, int64_t cols, int64_t row_stride,
                          int64_t col_stride, const double *prior, const double *counts,
                          double *alpha, double *elog, double *ws, double *bound)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && rows >= 0 && cols >= 1 && row_stride >= 1 && col_stride >= 1,
                VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, bound && ws && (rows == 0 || (prior && alpha && elog)), VMP_ERR_INVALID,
                "null argument");
    if (rows == 0) {
        VMP_HIP_CHECK(ctx, hipMemsetAsync(bound, 0, sizeof(double), ctx->stream));
        return VMP_OK;
    }
    if (cols <= VMP_TABLE_THREAD_COLS)
        hipLaunchKernelGGL(lda_dirichlet_rows_kernel<false>,
                           dim3((unsigned)((rows + LDA_NT - 1) / LDA_NT)), dim3(LDA_NT), 0,
                           ctx->stream, rows, (int)cols, row_stride, col_stride, prior, counts, 1.0,
                           1.0, alpha, elog, ws);
    else
        hipLaunchKernelGGL(lda_dirichlet_wide_kernel<false>, dim3((unsigned)rows), dim3(LDA_NT), 0,
                           ctx->stream, cols, row_stride, col_stride, prior, counts, 1.0, 1.0,
                           alpha, elog, ws);
    hipLaunchKernelGGL(lda_sum_final_kernel, dim3(1), dim3(LDA_RED_NT), 0, ctx->stream, rows, ws,
                       bound);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

// the table is stored transposed (the rows run down the strided axis) and has few enough rows for
// the kernel pair that walks the memory in order
static inline bool lda_step_transposed(int64_t rows, int64_t row_stride, int64_t col_stride)
{
    return row_stride == 1 && col_stride == rows && rows <= LDA_MAX_K;
}

int32_t vmp_lda_dirichlet_step_workspace(int64_t rows, int64_t cols, int64_t row_stride,
                                         int64_t col_stride, int64_t *workspace_doubles)
{
    if (rows < 0 || cols < 1 || row_stride < 1 || col_stride < 1 || !workspace_doubles)
        return VMP_ERR_INVALID;
    if (rows > 0 && lda_step_transposed(rows, row_stride, col_stride))
        *workspace_doubles = lda_t_ws_doubles(cols, (int)rows);
    else
        *workspace_doubles = rows > 0 ? rows : 1;
    return VMP_OK;
}

int32_t vmp_lda_dirichlet_step(vmp_ctx *ctx, int64_t rows, int64_t cols, int64_t row_stride,
                               int64_t col_stride, const double *prior, const double *counts,
                               double mult, double scale, double *alpha, double *elog, double *ws,
                               double *bound)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && rows >= 0 && cols >= 1 && row_stride >= 1 && col_stride >= 1,
                VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, mult > 0.0 && scale == scale && mult == mult, VMP_ERR_INVALID,
                "mult must be positive, scale a number");
    VMP_REQUIRE(ctx, bound && ws && (rows == 0 || (prior && alpha && elog)), VMP_ERR_INVALID,
                "null argument");
    if (rows == 0) {
        VMP_HIP_CHECK(ctx, hipMemsetAsync(bound, 0, sizeof(double), ctx->stream));
        return VMP_OK;
    }
    if (lda_step_transposed(rows, row_stride, col_stride)) {
        const int K = (int)rows;
        const TGrid g = lda_t_grid(cols, K);
        double *bpart = ws, *rowc = ws + g.nb, *psis = rowc + K, *part = psis + K;
        hipLaunchKernelGGL(lda_step_t_alpha_kernel, dim3((unsigned)g.nb), dim3(LDA_NT), 0,
                           ctx->stream, cols, K, g.cpb, prior, counts, mult, scale, alpha, part);
        hipLaunchKernelGGL(lda_step_t_combine_kernel, dim3((unsigned)K), dim3(LDA_NT), 0,
                           ctx->stream, g.nb, K, part, rowc, psis);
        hipLaunchKernelGGL(lda_step_t_elog_kernel, dim3((unsigned)g.nb), dim3(LDA_NT), 0,
                           ctx->stream, cols, K, g.cpb, prior, alpha, psis, elog, bpart);
        // bound partials and row constants stand side by side
        hipLaunchKernelGGL(lda_sum_final_kernel, dim3(1), dim3(LDA_RED_NT), 0, ctx->stream,
                           g.nb + K, ws, bound);
    } else {
        if (cols <= VMP_TABLE_THREAD_COLS)
            hipLaunchKernelGGL(lda_dirichlet_rows_kernel<true>,
                               dim3((unsigned)((rows + LDA_NT - 1) / LDA_NT)), dim3(LDA_NT), 0,
                               ctx->stream, rows, (int)cols, row_stride, col_stride, prior, counts,
                               mult, scale, alpha, elog, ws);
        else
            hipLaunchKernelGGL(lda_dirichlet_wide_kernel<true>, dim3((unsigned)rows), dim3(LDA_NT),
                               0, ctx->stream, cols, row_stride, col_stride, prior, counts, mult,
                               scale, alpha, elog, ws);
        hipLaunchKernelGGL(lda_sum_final_kernel, dim3(1), dim3(LDA_RED_NT), 0, ctx->stream, rows,
                           ws, bound);
    }
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_lda_dot(vmp_ctx *ctx, int64_t m, const double *a, const double *b, double *ws,
                    double *out)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && m >= 0, VMP_ERR_INVALID, "bad arguments");
    VMP_REQUIRE(ctx, out && ws && (m == 0 || (a && b)), VMP_ERR_INVALID, "null argument");
    launch_dot(ctx, m, a, b, ws, out);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
