// vmp_ml.hip -- updates of the maximum-likelihood hyperparameter nodes GammaShape and
// Concentration (reference: gamma.py:273-334, dirichlet.py:234-330) and the elementwise inverse
// digamma (misc.invpsi, utils/misc.py:1404-1429).
//
// The concentration update is a fixed-point loop whose length depends on the data: it restarts
// from a = 1 and stops the first time NO element of ANY plate row moved by more than 1e-5 relative
// to its new value.  The whole loop runs in ONE workgroup, one lane per element, and the "any
// element moved" of an iteration is one LDS flag.  No grid-wide barrier, no host round trip: the
// launch is a node of a recorded sweep like any other.  The loop is capped; reaching the cap is
// reported through the status words (the reference would loop on).
#include "vmp_common.h"
#include "vmp_ml_dev.h"

namespace {

constexpr int ML_NT = 256;           // elementwise kernels
constexpr int CONC_NT = 1024;        // the one workgroup of the concentration fixed point

__global__ void __launch_bounds__(ML_NT)
ml_invpsi_kernel(int64_t n, const double *__restrict__ x, double *__restrict__ y)
{
    for (int64_t i = (int64_t)blockIdx.x * ML_NT + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * ML_NT)
        y[i] = vmp_invpsi(x[i]);
}

__global__ void __launch_bounds__(ML_NT)
ml_gamma_shape_kernel(int64_t n, const double *__restrict__ m0, const double *__restrict__ m1,
                      const double *__restrict__ r0, const double *__restrict__ r1,
                      double *__restrict__ a, double *__restrict__ lga)
{
    for (int64_t i = (int64_t)blockIdx.x * ML_NT + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * ML_NT) {
        const double x = vmp_ml_gamma_shape_value(m0[i], m1[i], r0[i], r1[i]);
        a[i] = x;
        lga[i] = vmp_lgamma(x);
    }
}

// One lane per (row, category) element: an iteration reads the old values from one buffer and
// writes the new ones to the other (alpha and work in turn), so the only barrier an iteration needs is
// the one that publishes "some element moved".  status[0]: 1 if some mean_logp is infinite (nothing
// iterated), status[1]: 1 if the loop hit max_iter before converging, status[2]: iterations run.
__global__ void __launch_bounds__(CONC_NT)
ml_concentration_kernel(int64_t rows, int K, const double *__restrict__ m0,
                        const double *__restrict__ m1, const double *__restrict__ r0,
                        const double *__restrict__ r1, int max_iter, double *alpha, double *work,
                        double *__restrict__ z, int32_t *__restrict__ status)
{
    __shared__ int s_inf;
    __shared__ int s_more[3];        // "some element moved" of iteration it lives in s_more[it % 3]
    const int tid = threadIdx.x;
    const int64_t ne = rows * K;
    if (tid == 0) {
        s_inf = 0;
        s_more[0] = s_more[1] = s_more[2] = 0;
    }
    __syncthreads();
    int bad = 0;
    for (int64_t e = tid; e < ne; e += CONC_NT) {
        const int64_t r = e / K;
        if (vmp_ml_isinf(vmp_ml_mean_logp(m0[e], r0[e], m1[r] + r1[r]))) bad = 1;
        alpha[e] = 1.0;
    }
    if (bad) s_inf = 1;
    __syncthreads();
    const bool inf = s_inf != 0;
    int it = 0;
    bool capped = false;
    if (!inf) {
        for (;;) {
            if (it == max_iter) {
                capped = true;
                break;
            }
            const double *cur = (it & 1) ? work : alpha;
            double *nxt = (it & 1) ? alpha : work;
            bool moved = false;
            for (int64_t e = tid; e < ne; e += CONC_NT) {
                const int64_t r = e / K;
                const double an = vmp_ml_concentration_element(cur + r * K, K, m0[e], m1[r], r0[e],
                                                                r1[r]);
                if (vmp_ml_moved(an, cur[e])) moved = true;
                nxt[e] = an;
            }
            const int slot = it % 3;
            if (moved) s_more[slot] = 1;
            // publishes the flag and the new values: the next iteration reads `nxt`, and writes
            // the buffer this one read only after every lane has passed this barrier
            __syncthreads();
            const int more = s_more[slot];
            // the slot of iteration it + 2 was last read before this barrier and is written
            // again only after the next one: clearing it here races with nothing
            if (tid == 0) s_more[(it + 2) % 3] = 0;
            ++it;
            if (!more) break;
        }
    }
    if (it & 1)                      // the last iteration wrote `work`
        for (int64_t e = tid; e < ne; e += CONC_NT) alpha[e] = work[e];
    __syncthreads();
    for (int64_t r = tid; r < rows; r += CONC_NT) z[r] = vmp_ml_concentration_z(alpha + r * K, K);
    if (tid == 0) {
        status[0] = inf ? 1 : 0;
        status[1] = capped ? 1 : 0;
        status[2] = it;
    }
}

unsigned grid_for(int64_t n)
{
    int64_t g = (n + ML_NT - 1) / ML_NT;
    if (g < 1) g = 1;
    if (g > 4096) g = 4096;
    return (unsigned)g;
}

}  // namespace

extern "C" {

int32_t vmp_ml_invpsi(vmp_ctx *ctx, int64_t n, const double *x, double *y)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && n >= 0, VMP_ERR_INVALID, "bad arguments");
    if (n == 0) return VMP_OK;
    VMP_REQUIRE(ctx, x && y, VMP_ERR_INVALID, "null argument");
    hipLaunchKernelGGL(ml_invpsi_kernel, dim3(grid_for(n)), dim3(ML_NT), 0, ctx->stream, n, x, y);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_ml_gamma_shape(vmp_ctx *ctx, int64_t n, const double *m0, const double *m1,
                           const double *r0, const double *r1, double *a, double *lga)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && n >= 0, VMP_ERR_INVALID, "bad arguments");
    if (n == 0) return VMP_OK;
    VMP_REQUIRE(ctx, m0 && m1 && r0 && r1 && a && lga, VMP_ERR_INVALID, "null argument");
    hipLaunchKernelGGL(ml_gamma_shape_kernel, dim3(grid_for(n)), dim3(ML_NT), 0, ctx->stream, n,
                       m0, m1, r0, r1, a, lga);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

int32_t vmp_ml_concentration(vmp_ctx *ctx, int64_t rows, int32_t K, const double *m0,
                             const double *m1, const double *r0, const double *r1, int32_t max_iter,
                             double *alpha, double *work, double *z, int32_t *status)
{
    VMP_FLUSH_SMALL(ctx);
    VMP_REQUIRE(ctx, ctx && rows >= 0 && K >= 1 && max_iter >= 1, VMP_ERR_INVALID,
                "bad arguments");
    VMP_REQUIRE(ctx, status && (rows == 0 || (m0 && m1 && r0 && r1 && alpha && work && z)),
                VMP_ERR_INVALID, "null argument");
    hipLaunchKernelGGL(ml_concentration_kernel, dim3(1), dim3(CONC_NT), 0, ctx->stream, rows, K,
                       m0, m1, r0, r1, max_iter, alpha, work, z, status);
    VMP_HIP_CHECK(ctx, hipGetLastError());
    return VMP_OK;
}

}  // extern "C"
