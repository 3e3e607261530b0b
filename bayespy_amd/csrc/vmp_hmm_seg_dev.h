// vmp_hmm_seg_dev.h -- shapes, splits and workspace of the segmented (time-parallel) chain stage of
// the fused hidden-Markov-model block (csrc/vmp_hmm_seg.hip).  Host and device share these
// functions; g++ compiles this header for the host side of the C ABI (vmp_hmm_seg_plan).
//
// The pass is vmp_hmm_wide_pass (vmp_hmm_wide_dev.h) with its chain kernel replaced: the emission
// table E, the statistics kernel and the combine kernel are the same instances.  The T - 1
// transitions of a chain are cut into S = ceil((T - 1) / L) segments; segment s covers the
// transitions s L + 1 ... min((s + 1) L, T - 1), from step n0 = s L to step n1.  With
// M_t[i, j] = <log A>[i, j] + e_t[j]:
//
//   transfer  for every (chain, segment, start state i): the forward recursion of
//             vmp_hmm_fused_dev.h over the segment from the unit vector at i, normalised per step,
//             the scales carried.  log W_s[i, j] = sum of the scales + final log vector: the log of
//             entry (i, j) of the product of the segment's M_t, per entry, each column with its
//             own maximum.  Every step first subtracts b_t = max_j e_t[j], which all start states
//             share, so that the scales stay of the size of a transition's log-probability and
//             log W keeps its digits; sum_t b_t of the segment is stored beside it and enters
//             log Z only.  Also stored: "any step of the segment observed" (step 0 with segment 0).
//   scan      one lane group per chain, S dependent steps each way.  Forward: la at every segment
//             start, la_{s+1}[j] = lse_i (la_s[i] + log W_s[i, j]), normalised; the scales and the
//             segments' sum b are the chain's log Z -- the only place it is formed.  Backward: lb at
//             every segment end, lb_s[i] = lse_j (log W_s[i, j] + lb_{s+1}[j]) less its largest
//             element.  The chain's weight is the OR of its segments' flags.
//   sweep     for every (chain, segment): the forward and backward loops of hmmw_chain_kernel from
//             the stored la at n0 and lb at n1.  la, then gamma in place, for the steps
//             n0 + 1 ... n1: the step at a shared boundary belongs to the segment that ENDS there,
//             step 0 to segment 0.  xi of the segment's own transitions.  Nothing is counted twice
//             and no two segments write the same element.
//   partials  a workgroup of the sweep owns vmp_hmms_items_per_wg consecutive (chain, segment)
//             items; lane group (wave w, group g) takes items g + G w, + 4 G, ... of the range in
//             ascending order, each in the order of its backward loop; the groups are added in
//             group order, the four wavefronts in wavefront order, the workgroups by the combine
//             kernel in workgroup order.  log Z_b joins the partial of the workgroup that owns
//             segment 0 of chain b.  No atomics: the bits depend on the inputs and
//             (B, T, D, K, L) alone.
#pragma once

#include "vmp_hmm_wide_dev.h"

#define VMP_HMMS_MAX_K 64
#define VMP_HMMS_MAX_D 32
#define VMP_HMMS_WAVES 4                  // wavefronts of a workgroup (transfer and sweep)
#define VMP_HMMS_MAX_SWEEP_WGS 2048
#define VMP_HMMS_MAX_TRANSFER_WGS 16384

// The library's segment length, a function of (B, T, K) alone.  The scan costs S = (T - 1) / L
// dependent steps and the transfer and the sweep L each, so the sum is smallest near
// L = sqrt(T x scan step / (transfer step + sweep step)).  Measured at T = 2e5, K = 16, B = 1 and 4
//  the powers of two 128, 256, 512, 1024 take 11.0, 8.6, 9.8, 14.8 ms: the rule is
// the smallest power of two with 4 L^2 >= T, not below 16.  B and K do not enter today: the form
// is meant for few chains.
__host__ __device__ inline int vmp_hmms_seg_len(int64_t B, int T, int K)
{
    (void)B;
    (void)K;
    int64_t L = 16;
    while (4 * L * L < T) L <<= 1;
    return (int)L;
}

// the segment length in use: the request (0 = the library's choice), at most T - 1
__host__ __device__ inline int vmp_hmms_clamp_len(int64_t B, int T, int K, int seg_len)
{
    int L = seg_len > 0 ? seg_len : vmp_hmms_seg_len(B, T, K);
    if (L > T - 1) L = T - 1;
    return L;
}

__host__ __device__ inline int64_t vmp_hmms_segments(int T, int L) { return ((int64_t)T - 2) / L + 1; }

// (chain, segment) items of a workgroup of the sweep: a multiple of the 4 x 64 / KP lane groups of
// the workgroup, at most VMP_HMMS_MAX_SWEEP_WGS workgroups and 2^23 doubles of partials
__host__ __device__ inline int64_t vmp_hmms_items_per_wg(int64_t B, int T, int K, int L)
{
    const int64_t unit = VMP_HMMS_WAVES * (64 / vmp_hmmf_kpad(K));
    int64_t maxw = ((int64_t)1 << 23) / vmp_hmmw_chain_partial_doubles(K);
    if (maxw > VMP_HMMS_MAX_SWEEP_WGS) maxw = VMP_HMMS_MAX_SWEEP_WGS;
    const int64_t items = B * vmp_hmms_segments(T, L);
    int64_t c = (items + maxw - 1) / maxw;
    c = (c + unit - 1) / unit * unit;
    if (c < unit) c = unit;
    return c;
}

__host__ __device__ inline int64_t vmp_hmms_sweep_wgs(int64_t B, int T, int K, int L)
{
    const int64_t c = vmp_hmms_items_per_wg(B, T, K, L);
    const int64_t items = B * vmp_hmms_segments(T, L);
    return items > 0 ? (items + c - 1) / c : 0;
}

// workspace of the pass: E (B T KP), the forward state that becomes gamma (B T K), the partials of
// the sweep and of the statistics kernel, 1024 doubles for the dot products, then log W
// (B S K KP), la at the segment starts and lb at the segment ends (B S KP each), the flag and the
// sum b of every segment (B S 2), the weight and log Z of every chain (B 2).  Not below the
// workspace of the wide pass, which serves fixed labels.
__host__ __device__ inline int64_t vmp_hmms_workspace_doubles(int64_t B, int T, int D, int K, int L)
{
    const int64_t R = B * (int64_t)T, KP = vmp_hmmf_kpad(K), BS = B * vmp_hmms_segments(T, L);
    const int64_t n = R * KP + R * K
                      + vmp_hmms_sweep_wgs(B, T, K, L) * vmp_hmmw_chain_partial_doubles(K)
                      + vmp_hmmw_row_wgs(R, D, K) * (int64_t)K * vmp_hmmf_nfeat(D) + 1024
                      + BS * K * KP + 2 * BS * KP + 2 * BS + 2 * B;
    const int64_t wide = vmp_hmmw_workspace_doubles(B, T, D, K);
    return n > wide ? n : wide;
}
