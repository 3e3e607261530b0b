// TEST PROGRAM: tests/host/cmm_host.cpp on two shapes, stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_cmm_host.py).  Exact-size heap buffers, so a read or
// write past any of them is reported.  Shape 1: N = 333, D = 7, K = 5, M = 5 (neither N nor D a
// multiple of the tile or of the lane groups, two chunks), a mask with holes, a row and a column
// of nothing and NaN / -1 / 1e300 at hidden positions.  Shape 2: N = 64, D = 7, K = 64, M = 32,
// the count table exactly at its cap.
#include <stdio.h>

#include "cmm_host.cpp"

static int run(int64_t N, int D, int K, int M, bool masked, bool labelled)
{
    std::vector<double> x((size_t)(N * D)), elog_p((size_t)M * D * K), elog_pi(K);
    std::vector<uint8_t> mask((size_t)(N * D));
    std::vector<int32_t> lab((size_t)N);
    uint32_t s = 999u + (uint32_t)(N * 7 + D * 5 + K + M);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    for (auto &v : elog_p) v = -0.05 - (double)(rnd() % 1000) / 300.0;
    for (auto &v : elog_pi) v = -0.1 - (double)(rnd() % 1000) / 300.0;
    const double junk[3] = {NAN, -1.0, 1e300};
    double observed = 0.0;
    for (int64_t n = 0; n < N; ++n) {
        lab[n] = (int32_t)(rnd() % (uint32_t)K);
        for (int d = 0; d < D; ++d) {
            const size_t e = (size_t)(n * D + d);
            mask[e] = !masked || ((rnd() % 10 < 7) && n != 3 && d != 2);
            x[e] = mask[e] ? (double)(rnd() % (uint32_t)M) : junk[rnd() % 3];
            observed += mask[e];
        }
    }
    std::vector<uint8_t> xb((size_t)(N * D));
    const int flag = cmm_pack(N, D, M, 0, x.data(), masked ? mask.data() : nullptr, xb.data());
    std::vector<double> L((size_t)M * D * K), c(K), S((size_t)M * D * K), Nk(K), scal(1),
        r((size_t)(N * K));
    cmm_tables(D, K, M, elog_p.data(), elog_pi.data(), L.data(), c.data());
    cmm_pass(N, D, K, M, xb.data(), labelled ? lab.data() : nullptr, L.data(), c.data(), S.data(),
             Nk.data(), scal.data(), r.data());
    double total = 0.0;
    for (double v : S) total += v;
    printf("N=%ld D=%d K=%d M=%d masked=%d labels=%d flag=%d: sum S = %.12g of %g observed "
           "entries, sum lse = %.12g\n", (long)N, D, K, M, (int)masked, (int)labelled, flag, total,
           observed, scal[0]);
    // r sums to one over k, so S adds up to the observed entries
    return (flag == 0 && fabs(total - observed) <= 1e-9 * (observed + 1.0)) ? 0 : 1;
}

int main()
{
    int bad = 0;
    bad += run(333, 7, 5, 5, true, false);
    bad += run(333, 7, 5, 5, true, true);
    bad += run(64, 7, 64, 32, false, false);
    bad += run(64, 7, 64, 32, true, true);
    return bad;
}
