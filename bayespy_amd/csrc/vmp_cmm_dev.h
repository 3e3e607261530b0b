// vmp_cmm_dev.h -- per-row arithmetic of the categorical-mixture pass (csrc/vmp_cmm.hip), shared
// with the host build of the CPU tests (tests/host/cmm_host.cpp).
//
// A row n of D categorical observations x_nd in [0, M) is kept as D BYTES; the byte VMP_CMM_HIDDEN
// (255, above every category since M <= 32) marks a hidden position.  With the category-major
// table L[m, d, k] = <log P_dk[m]> (element at (m D + d) K + k) and c[k] = <log pi_k> less its
// maximum the logits of the row are
//     l_k = c[k] + sum over the observed d of L[x_nd, d, k],          k = 0 .. K-1
// (mixture.py: the (N, D, K) broadcast of <log P>[x] summed over D plus the message of the
// Categorical parent; categorical.py).  r_k = exp(l_k - lse), lse = m + log(sum_k exp(l_k - m)),
// m = max_k l_k.  The constant taken out of c is the one of vmp_bmm_dev.h, for the same reason:
// r, the statistics and the entropy sum lse - N_k . c - S . L do not depend on it.
//
// A byte is OBSERVED when (unsigned) byte < M: the one unsigned compare of vmp_hmmf_cat_observed.
// The pack kernel writes VMP_CMM_HIDDEN wherever the mask is zero or the value fails its check, so
// a value that is not a category never becomes an address.
//
// ORDER OF THE ADDITIONS (what the host build restates), with KP = vmp_cmm_kpad(K) in {16, 32, 64}
// the lanes of a lane group, G = 64 / KP groups per wavefront and NG = 4 G groups per workgroup:
//   * logit: starts at zero, adds L[x_nd, d, k] for the observed d in ascending d and c[k] last;
//     lanes k >= K hold -inf and give r = 0 exactly;
//   * the sum under the logarithm runs over the KP lanes by the butterfly (partner k ^ off,
//     off = KP / 2, ..., 1);
//   * rows are walked in TILES of 64; row t of a tile belongs to group t % NG.  N_k and sum lse
//     are kept per group in row order over a CHUNK and the NG groups are added in group order at
//     its end.  A row with nothing observed keeps r = softmax(c) for r_out and adds exactly
//     nothing to any sum;
//   * S[m, d, k]: one cell of the workgroup's LDS table, owned by one lane, adds r_k of the rows
//     with x_nd = m in ascending row order through the chunk;
//   * a workgroup owns one chunk of vmp_cmm_chunk_rows consecutive rows; the chunks' partial S,
//     N_k and sum lse are added in chunk order by a second kernel.
// The bits of every output therefore depend on the inputs and (N, D, K, M) only.
//
// THE COUNT TABLE IN LDS.  Column d belongs to wavefront (d / G) % 4 and to group d % G of it; its
// cell (m, k) is at ((d / G) M + m) 64 + (d % G) KP + k doubles, that is at a multiple of 64 plus
// the lane (d % G) KP + k that owns it: the bank depends on the lane alone, no two lanes share a
// cell, and nothing but that lane ever touches it -- no atomics.  D is padded to a multiple of G in
// this layout, so the cells that count against the cap are vmp_cmm_cells = roundup(D, G) M KP.
#pragma once

#include <math.h>
#include <stdint.h>

#define VMP_CMM_MAX_K 64
#define VMP_CMM_MIN_M 2
#define VMP_CMM_MAX_M 32
#define VMP_CMM_MAX_CELLS 14336   // doubles of the count table of a workgroup (112 KB)
#define VMP_CMM_HIDDEN 255
#define VMP_CMM_TILE 64           // rows per tile
#define VMP_CMM_NT 256            // threads of a workgroup: four wavefronts
#define VMP_CMM_MIN_CHUNK 256
#define VMP_CMM_MAX_CHUNKS 1024

__host__ __device__ inline int vmp_cmm_kpad(int K) { return K <= 16 ? 16 : (K <= 32 ? 32 : 64); }

// lane groups of a workgroup
__host__ __device__ inline int vmp_cmm_groups(int K) { return VMP_CMM_NT / vmp_cmm_kpad(K); }

// columns of the LDS table: D padded to the groups of a wavefront
__host__ __device__ inline int vmp_cmm_dpad(int D, int K)
{
    const int G = 64 / vmp_cmm_kpad(K);
    return (D + G - 1) / G * G;
}

__host__ __device__ inline int64_t vmp_cmm_cells(int D, int K, int M)
{
    return (int64_t)vmp_cmm_dpad(D, K) * M * vmp_cmm_kpad(K);
}

__host__ __device__ inline bool vmp_cmm_supported(int D, int K, int M)
{
    return K <= VMP_CMM_MAX_K && M >= VMP_CMM_MIN_M && M <= VMP_CMM_MAX_M && D <= VMP_CMM_MAX_CELLS
        && vmp_cmm_cells(D, K, M) <= VMP_CMM_MAX_CELLS;
}

// LDS cell of (column d, category m, cluster k)
__host__ __device__ inline int vmp_cmm_cell(int d, int m, int k, int M, int KP)
{
    const int G = 64 / KP;
    return ((d / G) * M + m) * 64 + (d % G) * KP + k;
}

// dynamic LDS of the pass in bytes: the count table, the r tile, N_k and sum lse of the groups,
// the staged bytes of a tile
__host__ __device__ inline int64_t vmp_cmm_lds_bytes(int D, int K, int M)
{
    const int KP = vmp_cmm_kpad(K);
    return 8 * (vmp_cmm_cells(D, K, M) + (int64_t)VMP_CMM_TILE * KP + VMP_CMM_NT + 16)
           + (((int64_t)VMP_CMM_TILE * D + 7) & ~(int64_t)7);
}

// doubles one chunk leaves behind: S (M x D x K, category-major), N_k (K), sum lse (1)
__host__ __device__ inline int64_t vmp_cmm_partial_doubles(int D, int K, int M)
{
    return (int64_t)M * D * K + K + 1;
}

// rows of a chunk: a function of (N, D, K, M) alone.  At most VMP_CMM_MAX_CHUNKS chunks and at most
// 2^25 doubles (256 MB) of partials; a multiple of the tile, at least VMP_CMM_MIN_CHUNK.
__host__ __device__ inline int64_t vmp_cmm_chunk_rows(int64_t N, int D, int K, int M)
{
    int64_t maxc = ((int64_t)1 << 25) / vmp_cmm_partial_doubles(D, K, M);
    if (maxc > VMP_CMM_MAX_CHUNKS) maxc = VMP_CMM_MAX_CHUNKS;
    if (maxc < 1) maxc = 1;
    int64_t rows = (N + maxc - 1) / maxc;
    rows = (rows + VMP_CMM_TILE - 1) / VMP_CMM_TILE * VMP_CMM_TILE;
    if (rows < VMP_CMM_MIN_CHUNK) rows = VMP_CMM_MIN_CHUNK;
    return rows;
}

__host__ __device__ inline int64_t vmp_cmm_chunks(int64_t N, int D, int K, int M)
{
    const int64_t rows = vmp_cmm_chunk_rows(N, D, K, M);
    return N > 0 ? (N + rows - 1) / rows : 0;
}

// the one unsigned compare: hidden (255) and anything else outside [0, M) index nothing
__host__ __device__ inline bool vmp_cmm_observed(uint8_t byte, int M)
{
    return (uint32_t)byte < (uint32_t)M;
}

// the byte of one entry.  `seen`: the mask says observed.  A hidden entry gets VMP_CMM_HIDDEN by a
// select, whatever its value; an observed value that is no integer in [0, M) gets it as well and
// sets *bad.  The conversion to an integer happens only after the range check, so NaN and 1e300
// are never converted.
__host__ __device__ inline uint8_t vmp_cmm_byte_f64(double v, bool seen, int M, bool *bad)
{
    const bool in = v >= 0.0 && v < (double)M;
    const int iv = in ? (int)v : 0;
    const bool ok = in && (double)iv == v;
    if (seen && !ok) *bad = true;
    return (seen && ok) ? (uint8_t)iv : (uint8_t)VMP_CMM_HIDDEN;
}

__host__ __device__ inline uint8_t vmp_cmm_byte_i64(int64_t v, bool seen, int M, bool *bad)
{
    const bool ok = (uint64_t)v < (uint64_t)M;
    if (seen && !ok) *bad = true;
    return (seen && ok) ? (uint8_t)v : (uint8_t)VMP_CMM_HIDDEN;
}

// one step of the logit
__host__ __device__ inline double vmp_cmm_logit_step(double logit, double l_xdk)
{
    return logit + l_xdk;
}

// the cluster's constant, added last
__host__ __device__ inline double vmp_cmm_logit_finish(double sum_l, double c_k) { return sum_l + c_k; }

__host__ __device__ inline double vmp_cmm_shifted_exp(double logit, double m) { return exp(logit - m); }

__host__ __device__ inline double vmp_cmm_lse(double m, double s) { return m + log(s); }

__host__ __device__ inline double vmp_cmm_resp(double logit, double lse) { return exp(logit - lse); }

#ifndef __HIPCC__
// the butterfly of a KP-lane group over v[0 .. KP-1]; every element ends with the result
inline void vmp_cmm_group_sum_host(double *v, int KP)
{
    double t[64];
    for (int off = KP / 2; off > 0; off >>= 1) {
        for (int l = 0; l < KP; ++l) t[l] = v[l] + v[l ^ off];
        for (int l = 0; l < KP; ++l) v[l] = t[l];
    }
}
#endif
