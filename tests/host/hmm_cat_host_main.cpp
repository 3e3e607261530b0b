// TEST PROGRAM: tests/host/hmm_cat_host.cpp on two shapes, stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_hmm_cat_host.py).  Exact-size heap buffers, so a read or
// write past any of them is reported.  Shape 1: one padded lane bucket, several workgroups' worth
// of lane groups, a mask with holes, -1 at masked positions and one out-of-range word at an
// observed position.  Shape 2: K = 64, M = 128 (the LDS maximum of the kernel), T = 2, no mask.
#include <stdio.h>

#include "hmm_cat_host.cpp"

static int run(int64_t B, int T, int M, int K, bool masked, bool labelled)
{
    std::vector<int32_t> y((size_t)(B * T)), lab((size_t)(B * T));
    std::vector<uint8_t> mask((size_t)(B * T));
    std::vector<double> Pt((size_t)M * K), la0(K), lA((size_t)K * K);
    uint32_t s = 12345u + (uint32_t)(B * 7 + T * 5 + M * 3 + K);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    for (auto &v : Pt) v = -0.1 - (double)(rnd() % 1000) / 200.0;
    for (auto &v : la0) v = -0.1 - (double)(rnd() % 1000) / 300.0;
    for (auto &v : lA) v = -0.1 - (double)(rnd() % 1000) / 300.0;
    for (size_t i = 0; i < y.size(); ++i) {
        mask[i] = masked ? (rnd() % 4 != 0) : 1;
        y[i] = mask[i] ? (int32_t)(rnd() % (uint32_t)M) : -1;
        lab[i] = (int32_t)(rnd() % (uint32_t)K);
    }
    if (masked) {
        y[0] = M + 7;                  // out of range at an observed position: counts as masked
        mask[0] = 1;
    }
    std::vector<double> z0sum(K), xisum((size_t)K * K), S((size_t)M * K), scal(2);
    std::vector<double> gamma((size_t)(B * T * K)), z0((size_t)(B * K));
    std::vector<double> zz((size_t)(B * (T - 1) * K * K));
    hmmc_pass(B, T, M, K, y.data(), Pt.data(), la0.data(), lA.data(),
              labelled ? lab.data() : nullptr, masked ? mask.data() : nullptr, z0sum.data(),
              xisum.data(), S.data(), scal.data(), gamma.data(), z0.data(), zz.data());
    double total = 0.0, seen = 0.0;
    for (double v : S) total += v;
    for (size_t i = 0; i < y.size(); ++i)
        if (mask[i] && y[i] >= 0 && y[i] < M) seen += 1.0;
    printf("B=%ld T=%d M=%d K=%d masked=%d labels=%d: sum S = %.12g of %g observed words, "
           "log Z = %.12g\n", (long)B, T, M, K, (int)masked, (int)labelled, total, seen, scal[0]);
    // every chain here has an observed step, so the counts add up to the observed words
    return fabs(total - seen) <= 1e-9 * (seen + 1.0) ? 0 : 1;
}

int main()
{
    int bad = 0;
    bad += run(45, 7, 5, 3, true, false);
    bad += run(45, 7, 5, 3, true, true);
    bad += run(3, 2, 128, 64, false, false);
    return bad;
}
