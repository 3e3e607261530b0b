// vmp_hmm_vocab_dev.h -- sizes, the segment walk and the combine rule of the large-vocabulary pass
// of the fused hidden-Markov-model block with categorical emissions (csrc/vmp_hmm_vocab.hip).
// Host and device share these functions; g++ compiles this header for the CPU tests
// (tests/host/hmm_vocab_host.cpp).
//
// The chain recursion is that of vmp_hmm_fused_dev.h, word for word; its kernel leaves gamma_t in
// place of la_t in the (B, T, K) workspace array.  What differs from vmp_hmm_cat.hip is the count
//     S[m][j] = sum over the observed (b, t) with y_{b,t} = m of gamma_{b,t}[j],
// which is no histogram here but a segmented sum over a WORD LAYOUT the caller provides:
//   order         n_obs int32 positions b T + t of the observed steps whose word lies in [0, M),
//                 sorted by word and, inside a word, by ascending position;
//   word_offsets  M + 1 int32: the entries of word m are order[word_offsets[m] ..
//                 word_offsets[m + 1]), word_offsets[0] = 0, word_offsets[M] = n_obs.
// ORDER OF THE ADDITIONS.  The layout is cut into chunks of CH = vmp_hmmv_chunk_entries(n_obs, K)
// consecutive entries.  One lane group walks a chunk in order; lane j adds gamma[order[i]][j] from
// zero, entry by entry.  A run of one word that begins and ends inside the chunk is stored to
// S[m] once.  The run that came in from the previous chunk goes to head[c], the run that goes on
// into the next to tail[c] (a chunk that lies wholly inside one word has a head and nothing
// else).  A word that crosses chunks c0 < c1 is then tail[c0] + head[c0 + 1] + ... + head[c1],
// added in that order; a word without an entry is written as zero.  S needs no clearing, nothing
// is atomic, and the bits depend on gamma, the layout and (n_obs, K) alone.
#pragma once

#include "vmp_hmm_fused_dev.h"
#include "vmp_lda_dev.h"

// int32 addressing of the table (M K doubles) and of the offsets; 32 MB of <log P> at K = 64
#define VMP_HMMV_MAX_M 65536

// doubles one workgroup of the chain kernel leaves behind: sum gamma_0 (K), sum xi (K x K),
// sum log Z, sum gamma . e -- the partial of the categorical pass without its M x K counts
__host__ __device__ inline int64_t vmp_hmmv_partial_doubles(int K)
{
    return vmp_hmmf_cat_partial_doubles(0, K);
}

__host__ __device__ inline int64_t vmp_hmmv_chains_per_wg(int64_t B, int K)
{
    return vmp_hmmf_cat_chains_per_wg(B, 0, K);
}

__host__ __device__ inline int64_t vmp_hmmv_wgs(int64_t B, int K)
{
    return vmp_hmmf_cat_wgs(B, 0, K);
}

// entries of a chunk: the rule of vmp_lda_chunk_tokens for n_obs entries and KP lanes per group
__host__ __device__ inline int vmp_hmmv_chunk_entries(int64_t n_obs, int K)
{
    return vmp_lda_chunk_tokens(n_obs, vmp_hmmf_kpad(K));
}

__host__ __device__ inline int64_t vmp_hmmv_chunks(int64_t n_obs, int K)
{
    const int ch = vmp_hmmv_chunk_entries(n_obs, K);
    return (n_obs + ch - 1) / ch;
}

// an upper bound of vmp_hmmv_chunks(n, K) over every n <= n_obs, monotone in n_obs: a chunk below
// 256 entries keeps n KP / CH at or below 2^17, one of 256 has n / 256 chunks, none has fewer than
// 16 entries.  The workspace is sized with it, so that one allocation for n_obs = B T serves every
// mask of the same plates.
__host__ __device__ inline int64_t vmp_hmmv_max_chunks(int64_t n_obs, int K)
{
    const int64_t by16 = (n_obs + 15) / 16;
    int64_t c = ((int64_t)1 << 17) / vmp_hmmf_kpad(K);
    if ((n_obs + 255) / 256 > c) c = (n_obs + 255) / 256;
    c += 1;
    return by16 < c ? by16 : c;
}

// workspace of the pass: gamma / la (B T K), the chain partials, head and tail (K doubles per
// chunk each), 1024 doubles for the dot products
__host__ __device__ inline int64_t vmp_hmmv_workspace_doubles(int64_t B, int T, int K,
                                                              int64_t n_obs)
{
    return B * (int64_t)T * K + vmp_hmmv_wgs(B, K) * vmp_hmmv_partial_doubles(K)
           + 2 * vmp_hmmv_max_chunks(n_obs, K) * K + 1024;
}

// the word of entry i: the m with word_offsets[m] <= i < word_offsets[m + 1] (0 <= i < n_obs)
__host__ __device__ inline int vmp_hmmv_word_of(const int32_t *off, int M, int64_t i)
{
    int lo = 0, hi = M - 1;             // the answer lies in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid + 1] > i) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// lane j's walk over chunk c (see the top of the file): gam (B T, K) row-major, S (M, K), head and
// tail (chunks, K).  The position of the entry after next and the row of the next entry are
// requested before the add of the present one.
__host__ __device__ inline void vmp_hmmv_walk_chunk(int64_t c, int CH, int64_t n_obs, int M, int K,
                                                    int j, const int32_t *order,
                                                    const int32_t *off, const double *gam,
                                                    double *S, double *head, double *tail)
{
    const int64_t cs = c * CH;
    const int64_t ce = (cs + CH < n_obs) ? cs + CH : n_obs;
    int cur = vmp_hmmv_word_of(off, M, cs);
    int64_t end = off[cur + 1];
    bool inside = off[cur] >= cs;       // the first run began in this chunk
    double acc = 0.0;
    double g = gam[(int64_t)order[cs] * K + j];
    int64_t pn = order[(cs + 1 < ce) ? cs + 1 : cs];
    for (int64_t i = cs; i < ce; ++i) {
        const int64_t i2 = (i + 2 < ce) ? i + 2 : ce - 1;
        const int64_t pnn = order[i2];
        const double gn = gam[pn * K + j];
        if (i == end) {
            (inside ? S + (int64_t)cur * K : head + c * K)[j] = acc;
            acc = 0.0;
            inside = true;
            while (cur + 1 < M && off[++cur + 1] <= i) {}   // past the words without an entry
            end = off[cur + 1];
        }
        acc += g;
        g = gn;
        pn = pnn;
    }
    const bool ends = end <= ce;        // the last run ends in this chunk
    double *dst = (inside && ends) ? S + (int64_t)cur * K : (!inside ? head + c * K : tail + c * K);
    dst[j] = acc;
}

// element (m, k) of S after the walk: zero for a word without an entry, the partials in chunk
// order for a word that crosses chunks; a word inside one chunk was written by the walk
__host__ __device__ inline void vmp_hmmv_combine_word(int m, int k, int CH, int K, int64_t n_obs,
                                                      const int32_t *off, const double *head,
                                                      const double *tail, double *S)
{
    const int64_t b = n_obs > 0 ? off[m] : 0, e = n_obs > 0 ? off[m + 1] : 0;
    if (b == e) {
        S[(int64_t)m * K + k] = 0.0;
        return;
    }
    const int64_t c0 = b / CH, c1 = (e - 1) / CH;
    if (c0 == c1) return;
    double sum = tail[c0 * K + k];
    for (int64_t c = c0 + 1; c <= c1; ++c) sum += head[c * K + k];
    S[(int64_t)m * K + k] = sum;
}
