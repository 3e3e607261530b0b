// TEST PROGRAM: tests/host/bmm_masked_host.cpp on two shapes, stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_bmm_masked_host.py).  Exact-size heap buffers, so a
// read or write past any of them is reported.  Shape 1: N = 333, D = 70, K = 5 (neither N nor D a
// multiple of 64, two chunks), a mask with holes, a row and a column of nothing and NaN at hidden
// positions.  Shape 2: N = 64, D = 128, K = 64, fixed labels.
#include <stdio.h>

#include "bmm_masked_host.cpp"

static int run(int64_t N, int D, int K, bool labelled)
{
    const int W = vmp_bmm_words(D);
    std::vector<double> x((size_t)(N * D)), elog_p((size_t)D * K * 2), elog_pi(K);
    std::vector<uint8_t> mask((size_t)(N * D));
    std::vector<int32_t> lab((size_t)N);
    uint32_t s = 999u + (uint32_t)(N * 7 + D * 5 + K);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    for (auto &v : elog_p) v = -0.05 - (double)(rnd() % 1000) / 300.0;
    for (auto &v : elog_pi) v = -0.1 - (double)(rnd() % 1000) / 300.0;
    double observed = 0.0;
    for (int64_t n = 0; n < N; ++n) {
        lab[n] = (int32_t)(rnd() % (uint32_t)K);
        for (int d = 0; d < D; ++d) {
            const size_t e = (size_t)(n * D + d);
            mask[e] = (rnd() % 10 < 7) && n != 3 && d != 2;
            x[e] = mask[e] ? (double)(rnd() % 2) : NAN;
            observed += mask[e];
        }
    }
    std::vector<uint64_t> xw((size_t)(N * 2 * W));
    const int flag = bmmm_pack(N, D, 0, x.data(), mask.data(), xw.data());
    std::vector<double> w((size_t)D * K), l0((size_t)D * K), c(K), S((size_t)D * K),
        M((size_t)D * K), Nk(K), counts((size_t)D * K * 2), scal(1), r((size_t)(N * K));
    bmmm_tables(D, K, elog_p.data(), elog_pi.data(), w.data(), l0.data(), c.data());
    bmmm_pass(N, D, K, xw.data(), labelled ? lab.data() : nullptr, w.data(), l0.data(), c.data(),
              S.data(), M.data(), Nk.data(), counts.data(), scal.data(), r.data());
    double total = 0.0;
    for (double v : M) total += v;
    printf("N=%ld D=%d K=%d labels=%d flag=%d: sum M = %.12g of %g observed entries, "
           "sum lse = %.12g\n", (long)N, D, K, (int)labelled, flag, total, observed, scal[0]);
    // r sums to one over k, so M adds up to the observed entries
    return (flag == 0 && fabs(total - observed) <= 1e-9 * (observed + 1.0)) ? 0 : 1;
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
