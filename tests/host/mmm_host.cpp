// TEST DOUBLE: the pack, the tables and the plate pass of csrc/vmp_mmm.hip on the host, built with
// g++ from the very header the kernels include (csrc/vmp_mmm_dev.h); the special functions of
// vmp_common.h come in ahead of this file (host_build.special_functions_text).  The chunks'
// partials are those of tests/host/pmm_host.cpp, nothing hidden, as vmp_mmm_pass runs the Poisson
// block's pass kernel; the combine into S (K x M), scal[1] and scal[2] are this block's own -- the
// order of every addition is the one the header states.
#include "pmm_host.cpp"
#include "../../bayespy_amd/csrc/vmp_mmm_dev.h"

extern "C" {

int mmm_max_k() { return VMP_MMM_MAX_K; }
int mmm_max_m() { return VMP_MMM_MAX_M; }
int mmm_max_count() { return VMP_MMM_MAX_COUNT; }
int mmm_mblock() { return VMP_MMM_MBLOCK; }
int64_t mmm_chunk_rows(int64_t N, int M, int K) { return vmp_mmm_chunk_rows(N, M, K); }
int64_t mmm_chunks(int64_t N, int M, int K) { return vmp_mmm_chunks(N, M, K); }
int64_t mmm_workspace_doubles(int64_t N, int M, int K) { return vmp_mmm_workspace_doubles(N, M, K); }

// xp (N x M), flags (4), lcoef (1)
void mmm_pack(int64_t N, int M, int dtype, const void *x, const int64_t *trials, uint16_t *xp,
              int32_t *flags, double *lcoef)
{
    const int64_t span = vmp_pmm_pack_span(N), nb = N > 0 ? vmp_pmm_pack_blocks(N) : 0;
    double total = 0.0, total_e = 0.0;
    int bad = 0;
    for (int64_t b = 0; b < nb; ++b) {
        double v[VMP_MMM_NT];
        for (int t = 0; t < VMP_MMM_NT; ++t) {
            double lg = 0.0, lge = 0.0;
            for (int64_t i = t; i < span; i += VMP_MMM_NT) {
                const int64_t row = b * span + i;
                if (row >= N) break;
                int bad_row = 0;
                int64_t sum = 0;
                vmp_pmm_sum_add(&lg, &lge, vmp_mmm_lgamma1_trials(trials[row]));
                for (int m = 0; m < M; ++m) {
                    const uint16_t p =
                        vmp_mmm_entry(vmp_pmm_pack_at(dtype, x, row * M + m, true, &bad_row));
                    xp[row * M + m] = p;
                    sum += p;
                    vmp_pmm_sum_add(&lg, &lge, -vmp_pmm_lgamma1(p));
                }
                if (vmp_mmm_sum_mismatch(sum, trials[row], bad_row)) bad_row |= VMP_MMM_BAD_SUM;
                bad |= bad_row;
            }
            v[t] = lg + lge;
        }
        for (int off = VMP_MMM_NT / 2; off > 0; off >>= 1)
            for (int i = 0; i < off; ++i) v[i] += v[i + off];
        vmp_pmm_sum_add(&total, &total_e, v[0]);
    }
    if (bad & VMP_PMM_BAD_INVALID) flags[0] = 1;
    if (bad & VMP_PMM_BAD_ABOVE) flags[1] = 1;
    if (bad & VMP_PMM_BAD_FRACTION) flags[2] = 1;
    if (bad & VMP_MMM_BAD_SUM) flags[3] = 1;
    lcoef[0] = total + total_e;
}

// L (M x K) from elog_p (K x M) or null, c (K)
void mmm_tables(int M, int K, const double *elog_p, const double *elog_pi, double *L, double *c)
{
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < K; ++k)
            L[m * K + k] = elog_p ? vmp_mmm_table(elog_p[k * M + m], elog_p[m]) : 0.0;
    double mx = elog_pi[0];
    for (int k = 1; k < K; ++k) mx = fmax(mx, elog_pi[k]);
    for (int k = 0; k < K; ++k) c[k] = elog_pi[k] - mx;
}

// S (K x M), Nk (K), scal[0] = sum lse, scal[1] = Nk . c, scal[2] = S . L; r_out (N x K) or null
void mmm_pass(int64_t N, int M, int K, const uint16_t *x, const int32_t *labels, const double *L,
              const double *c, double *S, double *Nk, double *scal, double *r_out)
{
    // the chunks' partials are the Poisson pass's, nothing hidden: words for columns, L for l
    const std::vector<double> part = pmm_pass_partials(N, M, K, 0, x, labels, L, L, c, r_out);
    const int64_t nc = vmp_mmm_chunks(N, M, K);
    const int64_t per = vmp_mmm_partial_doubles(M, K), MK = (int64_t)M * K;
    for (int64_t i = 0; i < MK; ++i) {
        double s = 0.0;
        for (int64_t ch = 0; ch < nc; ++ch) s += part[ch * per + i];
        S[i] = s;
    }
    for (int k = 0; k < K; ++k) {
        double n = 0.0;
        for (int64_t ch = 0; ch < nc; ++ch) n += part[ch * per + MK + k];
        Nk[k] = n;
    }
    double t = 0.0;
    for (int64_t ch = 0; ch < nc; ++ch) t += part[ch * per + MK + K];
    scal[0] = t;
    double n = 0.0;
    for (int k = 0; k < K; ++k) n = vmp_pmm_mac(n, Nk[k], c[k]);
    scal[1] = n;
    double d[VMP_MMM_NT];
    for (int tid = 0; tid < VMP_MMM_NT; ++tid) {
        double a = 0.0;
        for (int64_t e = tid; e < MK; e += VMP_MMM_NT)
            a = vmp_pmm_mac(a, S[e], L[(e % M) * K + e / M]);
        d[tid] = a;
    }
    for (int off = VMP_MMM_NT / 2; off > 0; off >>= 1)
        for (int i = 0; i < off; ++i) d[i] += d[i + off];
    scal[2] = d[0];
}

}  // extern "C"
