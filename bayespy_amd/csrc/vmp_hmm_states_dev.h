// vmp_hmm_states_dev.h -- shapes, splits and workspace of the wide-state pass of the fused
// hidden-Markov-model block (csrc/vmp_hmm_states.hip): multinomial emissions, 65 to 128 states.
// Host and device share these functions.
//
// The emission, statistics, combine and shift kernels are those of vmp_hmm_mult_dev.h with eight
// state tiles (KP = 128).  What this pass brings is the chain stage: the lane-per-state kernel of
// vmp_hmm_wide_dev.h stops at 64 states, so the recursion runs here in the domain of scaled
// probabilities with its K x K products on the fp64 matrix cores (v_mfma_f64_16x16x4f64):
//
//   P = exp(<log A>) (-inf gives an exact 0), b_t = exp(E_t) (E is stored less its row maximum,
//   so b_t <= 1 with a 1 in every observed row; 1 for every state at a masked step)
//   forward   x_0 = exp(<log a0> - max) o b_0;  x_t = (ah_{t-1} P) o b_t;  c_t = sum_j x_t[j],
//             ah_t = x_t / c_t,  sum log Z = sum_t log c_t (+ the maximum of <log a0>)
//   backward  bh_{T-1} = 1;  v_{t+1} = b_{t+1} o bh_{t+1};  u_t = v_{t+1} P^T;
//             s_t = sum_i ah_t[i] u_t[i];  gamma_t = ah_t o u_t / s_t;  bh_t = u_t / sum_i u_t[i]
//             xi_t[i, j] = ah_t[i] P[i, j] v_{t+1}[j] / s_t   (adds up to 1)
//   sum xi    = P o sum over chains and steps of (o_b ah_t / s_t)^T v_{t+1}: one product contracted
//             over the 16 chains of a tile per step, kept in accumulator registers over all steps
//             and tiles of a workgroup, multiplied by P once at the end
//
// A workgroup of four wavefronts owns vmp_hmms_chains_per_wg(B) consecutive chains and walks them
// in tiles of 16: the chains are the rows of the matrix instruction, a wavefront owns the column
// tiles 2 w and 2 w + 1 of 16 states.  One partial per workgroup in the layout of
// vmp_hmmw_chain_partial_doubles, added in workgroup order: no atomics, the bits of every output
// depend on the inputs and (B, T, M, K) alone.
//
// RANGE.  What the probability domain gives up against the logarithms of vmp_hmm_fused_dev.h: an
// entry of <log A> below about -745 underflows to 0 and acts as -inf; <log a0> is taken less its
// maximum first, so only its spread counts.  A step whose predicted mass c_t underflows entirely
// (every reachable state has b_t = 0, or ah_{t-1} P o b_t < 1e-308 throughout) gives c_t = 0 and
// NaN from there on, exactly what an impossible observation gives.  There is no log-domain fallback.
#pragma once

#include "vmp_hmm_mult_dev.h"

#define VMP_HMMS_MIN_K 65
#define VMP_HMMS_MAX_K 128
#define VMP_HMMS_KP 128
#define VMP_HMMS_TILE 16          // chains of a tile: the rows of the matrix instruction
#define VMP_HMMS_P_STRIDE 130     // doubles per row of P in LDS
#define VMP_HMMS_XF_STRIDE 18     // forward: the tile state-major, X[state][chain]
#define VMP_HMMS_XB_STRIDE 130    // backward: the tile chain-major, X[chain][state]

// doubles of LDS: P, the tile of the step, the sums of the four wavefronts (two per chain), the
// chains' weights
__host__ __device__ constexpr int vmp_hmms_lds_doubles()
{
    return VMP_HMMS_KP * VMP_HMMS_P_STRIDE + VMP_HMMS_KP * VMP_HMMS_XF_STRIDE
           + 4 * VMP_HMMS_TILE * 2 + VMP_HMMS_TILE;
}

// chains of a workgroup: a multiple of the tile, a function of B alone (K does not enter: KP is
// 128 throughout), at most VMP_HMMF_MAX_WGS workgroups
__host__ __device__ inline int64_t vmp_hmms_chains_per_wg(int64_t B)
{
    int64_t c = (B + VMP_HMMF_MAX_WGS - 1) / VMP_HMMF_MAX_WGS;
    c = (c + VMP_HMMS_TILE - 1) / VMP_HMMS_TILE * VMP_HMMS_TILE;
    return c < VMP_HMMS_TILE ? VMP_HMMS_TILE : c;
}

__host__ __device__ inline int64_t vmp_hmms_chain_wgs(int64_t B)
{
    const int64_t c = vmp_hmms_chains_per_wg(B);
    return B > 0 ? (B + c - 1) / c : 0;
}

// workspace of the pass: that of vmp_hmmm_workspace_doubles with this chain stage's partials
__host__ __device__ inline int64_t vmp_hmms_workspace_doubles(int64_t B, int T, int M, int K)
{
    const int64_t R = B * (int64_t)T;
    return R * VMP_HMMS_KP + R * K + vmp_hmms_chain_wgs(B) * vmp_hmmw_chain_partial_doubles(K)
           + vmp_hmmm_row_wgs(R, M, K) * (int64_t)M * K + 4 * vmp_hmmm_emit_wgs(R) + 1024;
}

#ifdef __HIPCC__
// the chain stage as a host call: the arguments and the outputs of vmp_hmmw_chain
// (vmp_hmm_wide_dev.h) for VMP_HMMS_MIN_K <= K <= VMP_HMMS_MAX_K, E with row stride 128,
// vmp_hmms_chain_wgs(B) partials in cpart
int32_t vmp_hmms_chain(vmp_ctx *ctx, int64_t B, int T, int K, const double *E, const double *la0,
                       const double *lA, const int32_t *labels, const uint8_t *mask, double *aw,
                       double *cpart, double *gamma, double *z0, double *zz);
#endif
