// TEST DOUBLE: the count of csrc/vmp_hmm_vocab.hip on the host, built with g++ from the very header
// the kernels include (csrc/vmp_hmm_vocab_dev.h): every chunk's walk for every lane j < K, then
// the combine rule for every (word, state).  S, head and tail come in as the caller filled them
// (NaN in the tests): the count clears nothing beforehand.
#include <math.h>
#include <stdint.h>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_hmm_vocab_dev.h"

extern "C" {

int hmmv_chunk_entries(int64_t n_obs, int K) { return vmp_hmmv_chunk_entries(n_obs, K); }

int64_t hmmv_max_chunks(int64_t n_obs, int K) { return vmp_hmmv_max_chunks(n_obs, K); }

void hmmv_count(int64_t n_obs, int M, int K, const int32_t *order, const int32_t *off,
                const double *gam, double *S, double *head, double *tail)
{
    const int CH = vmp_hmmv_chunk_entries(n_obs, K);
    const int64_t nc = vmp_hmmv_chunks(n_obs, K);
    for (int64_t c = 0; c < nc; ++c)
        for (int j = 0; j < K; ++j)
            vmp_hmmv_walk_chunk(c, CH, n_obs, M, K, j, order, off, gam, S, head, tail);
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < K; ++k)
            vmp_hmmv_combine_word(m, k, CH, K, n_obs, off, head, tail, S);
}

}  // extern "C"
