// TEST PROGRAM: tests/host/dgmm_masked_host.cpp on two shapes, stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_dgmm_masked_host.py; the special functions of
// vmp_common.h come in ahead of it, as for the library).  Exact-size heap buffers, so a read or
// write past any of them is reported.  Shape 1: N = 333, D = 70, K = 5 (neither N nor D a multiple
// of 64 or 32, two chunks, three column blocks), a mask with holes, a row and a column of nothing
// and NaN, 1e300 and -inf at hidden positions.  Shape 2: N = 64, D = 128, K = 64.  Both with and
// without fixed labels, followed by both updates.
#include <stdio.h>

#include "dgmm_masked_host.cpp"

static int run(int64_t N, int D, int K, bool labelled)
{
    std::vector<double> y((size_t)(N * D)), yp((size_t)(N * D)), mu_mom((size_t)D * K * 2),
        tau_mom((size_t)D * K * 2), elog_pi(K);
    std::vector<uint8_t> mask((size_t)(N * D));
    std::vector<int32_t> lab((size_t)N);
    uint32_t s = 4242u + (uint32_t)(N * 7 + D * 5 + K);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    auto uni = [&]() { return (double)(rnd() % 100000) / 100000.0; };
    for (size_t e = 0; e < (size_t)D * K; ++e) {
        const double m = 2.0 * uni() - 1.0, tau = 0.5 + uni();
        mu_mom[2 * e] = m;
        mu_mom[2 * e + 1] = m * m + 0.01;
        tau_mom[2 * e] = tau;
        tau_mom[2 * e + 1] = log(tau) - 0.005;
    }
    for (auto &v : elog_pi) v = -0.1 - 3.0 * uni();
    const double junk[3] = {NAN, 1e300, -INFINITY};
    int64_t observed = 0;
    for (int64_t n = 0; n < N; ++n) {
        lab[n] = (int32_t)(rnd() % (uint32_t)K);
        for (int d = 0; d < D; ++d) {
            const size_t e = (size_t)(n * D + d);
            mask[e] = (rnd() % 10 < 7) && n != 3 && d != 2;
            y[e] = mask[e] ? 4.0 * uni() - 2.0 : junk[rnd() % 3];
            observed += mask[e];
        }
    }
    const int64_t count = dgmmm_pack(N, D, y.data(), mask.data(), yp.data());
    const size_t DK = (size_t)D * K;
    std::vector<double> h(DK), q(DK), g(DK), c(K), S1(DK), S2(DK), M(DK), Nk(K), scal(1),
        r((size_t)(N * K)), par(2 * DK), mom(2 * DK), bound(1);
    dgmmm_tables(D, K, mu_mom.data(), tau_mom.data(), elog_pi.data(), h.data(), q.data(), g.data(),
                 c.data());
    dgmmm_pass(N, D, K, yp.data(), labelled ? lab.data() : nullptr, h.data(), q.data(), g.data(),
               c.data(), S1.data(), S2.data(), M.data(), Nk.data(), scal.data(), r.data());
    double total = 0.0, s12 = 0.0, b = 0.0;
    for (double v : M) total += v;
    for (size_t e = 0; e < DK; ++e) s12 += S1[e] + S2[e];
    std::vector<double> ones(DK, 1.0);
    for (int which = 0; which < 2; ++which) {
        dgmmm_update(D, K, which, ones.data(), ones.data(), S1.data(), S2.data(), M.data(),
                     which == 0 ? tau_mom.data() : mu_mom.data(), par.data(), mom.data(),
                     bound.data());
        b += bound[0];
    }
    printf("N=%ld D=%d K=%d labels=%d: sum M = %.12g of %ld (%ld) observed entries, sum lse = "
           "%.12g, bounds %.12g\n", (long)N, D, K, (int)labelled, total, (long)observed,
           (long)count, scal[0], b);
    // r sums to one over k, so M adds up to the observed entries; nothing hidden reached a sum
    return (count == observed && fabs(total - (double)observed) <= 1e-9 * ((double)observed + 1.0)
            && isfinite(s12) && isfinite(scal[0]) && isfinite(b)) ? 0 : 1;
}

int main()
{
    int bad = 0;
    bad += run(333, 70, 5, false);
    bad += run(333, 70, 5, true);
    bad += run(64, 128, 64, true);
    bad += run(64, 128, 64, false);
    return bad;
}
