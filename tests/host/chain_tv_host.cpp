// TEST DOUBLE: vmp_chain_pair_stats of csrc/vmp_chain_tv.hip on the host, built with g++ from the
// very header the kernels include (csrc/vmp_chain_tv_dev.h): the same split of the sequences into
// slices, the same chain of fused multiply-adds per element and slice, the same order of the
// slice partials.  One thread plays every lane in turn.
#include <math.h>
#include <stdint.h>

#define __host__
#define __device__
#include "../../bayespy_amd/csrc/vmp_chain_tv_dev.h"

extern "C" {

int32_t chain_tv_max_d(void) { return VMP_CHAIN_TV_MAX_D; }

int64_t chain_tv_work_doubles(int64_t ny, int32_t N, int32_t D)
{
    return vmp_chain_tv_work_doubles(ny, N, D);
}

int64_t chain_tv_nslice(int64_t ny, int32_t N, int32_t D) { return vmp_chain_tv_nslice(ny, N, D); }

// 0 ok, 1 bad arguments, 2 workspace too small
int32_t chain_tv_pair_stats(int64_t ny, int32_t N, int32_t D, const double *x, double *Sxx,
                            double *Sxp, double *work, int64_t work_doubles)
{
    if (ny < 0 || N < 1 || D < 1 || D > VMP_CHAIN_TV_MAX_D) return 1;
    const int64_t per = vmp_chain_tv_per(ny, N, D);
    const int64_t nslice = vmp_chain_tv_nslice(ny, N, D);
    const int64_t total = vmp_chain_tv_total(N, D);
    if (work_doubles < nslice * total) return 2;
    const int64_t nxx = (int64_t)N * D * D;
    const int64_t row = (int64_t)N * D;
    for (int64_t s = 0; s < nslice; ++s) {
        const int64_t b0 = s * per;
        const int64_t b1 = ny < b0 + per ? ny : b0 + per;
        double *w = work + s * total;
        for (int t = 0; t < N; ++t)
            for (int i = 0; i < D; ++i)
                for (int j = 0; j < D; ++j) {
                    double axx = 0.0, axp = 0.0;
                    for (int64_t b = b0; b < b1; ++b) {
                        const double *xb = x + b * row;
                        axx = vmp_chain_tv_step(axx, xb[t * D + i], xb[t * D + j]);
                        if (t < N - 1)
                            axp = vmp_chain_tv_step(axp, xb[t * D + i], xb[(t + 1) * D + j]);
                    }
                    w[((int64_t)t * D + i) * D + j] = axx;
                    if (t < N - 1) w[nxx + ((int64_t)t * D + i) * D + j] = axp;
                }
    }
    for (int64_t e = 0; e < total; ++e) {
        const double v = vmp_chain_tv_combine(work, nslice, total, e);
        if (e < nxx) Sxx[e] = v;
        else Sxp[e - nxx] = v;
    }
    return 0;
}

}  // extern "C"
