// TEST DOUBLE: vmp_chain_input_stats of csrc/vmp_chain_in.hip on the host, built with g++ from the
// very header the kernels include (csrc/vmp_chain_in_dev.h): the same split of the sequences into
// slices, the same chain of fused multiply-adds per element and slice, the same order of the
// slice partials.  One thread plays every lane in turn.
#include <math.h>
#include <stdint.h>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_chain_in_dev.h"

extern "C" {

int32_t chain_in_max_d(void) { return VMP_CHAIN_IN_MAX_D; }
int32_t chain_in_max_k(void) { return VMP_CHAIN_IN_MAX_K; }
int32_t chain_in_tile(int32_t D, int32_t K) { return vmp_chain_in_tile(D, K); }

int64_t chain_in_work_doubles(int64_t ny, int32_t N, int32_t D, int32_t K)
{
    return vmp_chain_in_work_doubles(ny, N, D, K);
}

int64_t chain_in_nslice(int64_t ny, int32_t N, int32_t D, int32_t K)
{
    return vmp_chain_in_nslice(ny, N, D, K);
}

// 0 ok, 1 bad arguments, 2 workspace too small.  Szz may be NULL.
int32_t chain_in_input_stats(int64_t ny, int64_t zrows, int32_t N, int32_t D, int32_t K,
                             const double *x, const double *z, double *Snz, double *Spz,
                             double *Szz, double *work, int64_t work_doubles)
{
    if (ny < 0 || (zrows != 1 && zrows != ny) || N < 2 || D < 1 || K < 1
        || D > VMP_CHAIN_IN_MAX_D || K > VMP_CHAIN_IN_MAX_K)
        return 1;
    const int64_t per = vmp_chain_in_per(ny, N, D, K);
    const int64_t nslice = vmp_chain_in_nslice(ny, N, D, K);
    const int64_t total = vmp_chain_in_total(N, D, K);
    const int64_t ncross = vmp_chain_in_cross(N, D, K);
    if (work_doubles < nslice * total) return 2;
    const int64_t xrow = (int64_t)N * D;
    const int64_t zrow = zrows == 1 && ny != 1 ? 0 : (int64_t)(N - 1) * K;
    for (int64_t s = 0; s < nslice; ++s) {
        const int64_t b0 = s * per;
        const int64_t b1 = ny < b0 + per ? ny : b0 + per;
        double *w = work + s * total;
        for (int t = 0; t < N - 1; ++t)
            for (int k = 0; k < K; ++k) {
                for (int i = 0; i < D; ++i) {
                    double anz = 0.0, apz = 0.0;
                    for (int64_t b = b0; b < b1; ++b) {
                        const double zk = z[b * zrow + t * K + k];
                        anz = vmp_chain_in_step(anz, x[b * xrow + (t + 1) * D + i], zk);
                        apz = vmp_chain_in_step(apz, x[b * xrow + t * D + i], zk);
                    }
                    w[((int64_t)t * D + i) * K + k] = anz;
                    w[ncross + ((int64_t)t * D + i) * K + k] = apz;
                }
                for (int i = 0; i < K; ++i) {
                    double azz = 0.0;
                    for (int64_t b = b0; b < b1; ++b)
                        azz = vmp_chain_in_step(azz, z[b * zrow + t * K + i], z[b * zrow + t * K + k]);
                    w[2 * ncross + ((int64_t)t * K + i) * K + k] = azz;
                }
            }
    }
    const int64_t used = Szz ? total : 2 * ncross;
    for (int64_t e = 0; e < used; ++e) {
        const double v = vmp_chain_in_combine(work, nslice, total, e);
        if (e < ncross) Snz[e] = v;
        else if (e < 2 * ncross) Spz[e - ncross] = v;
        else Szz[e - 2 * ncross] = v;
    }
    return 0;
}

}  // extern "C"
