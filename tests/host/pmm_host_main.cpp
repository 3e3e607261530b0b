// TEST PROGRAM: tests/host/pmm_host.cpp on two shapes, stand-alone, for a build with
// -fsanitize=address,undefined (tests/test_pmm_host.py).  Exact-size heap buffers, so a read or
// write past any of them is reported.  Shape 1: N = 333, D = 131, K = 5 (neither N nor D a multiple
// of the tile or of a column block, two chunks), with a mask with holes, a row and a column of
// nothing and NaN / -1 / 1e300 at hidden positions, and without a mask.  Shape 2: N = 64, D = 7,
// K = 64 with counts up to the cap.
#include <stdio.h>

#include "pmm_host.cpp"

static int run(int64_t N, int D, int K, bool masked, bool labelled, uint32_t top)
{
    std::vector<double> x((size_t)(N * D)), lam_mom((size_t)2 * D * K), elog_pi(K), a0((size_t)D * K),
        b0((size_t)D * K);
    std::vector<uint8_t> mask((size_t)(N * D));
    std::vector<int32_t> lab((size_t)N);
    uint32_t s = 4119u + (uint32_t)(N * 7 + D * 5 + K);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    for (int i = 0; i < D * K; ++i) {
        const double rate = 0.5 + (double)(rnd() % 1000) / 100.0;
        lam_mom[2 * i] = rate;
        lam_mom[2 * i + 1] = log(rate) - 0.01;
        a0[i] = 0.1 + (double)(rnd() % 100) / 50.0;
        b0[i] = 0.1 + (double)(rnd() % 100) / 50.0;
    }
    for (auto &v : elog_pi) v = -0.1 - (double)(rnd() % 1000) / 300.0;
    const double junk[3] = {NAN, -1.0, 1e300};
    double observed = 0.0, total_x = 0.0;
    for (int64_t n = 0; n < N; ++n) {
        lab[n] = (int32_t)(rnd() % (uint32_t)K);
        for (int d = 0; d < D; ++d) {
            const size_t e = (size_t)(n * D + d);
            mask[e] = !masked || ((rnd() % 10 < 7) && n != 3 && d != 2);
            x[e] = mask[e] ? (double)(rnd() % (top + 1)) : junk[rnd() % 3];
            observed += mask[e];
            if (mask[e]) total_x += x[e];
        }
    }
    std::vector<uint16_t> xp((size_t)(N * D));
    int32_t flags[3] = {0, 0, 0};
    int64_t counts[2];
    double lgam;
    pmm_pack(N, D, 0, x.data(), masked ? mask.data() : nullptr, xp.data(), flags, counts, &lgam);
    const int hidden = counts[1] > 0;
    std::vector<double> l((size_t)D * K), lb((size_t)D * K), c(K), lsum(K), S((size_t)D * K),
        M((size_t)D * K), Nk(K), scal(1), r((size_t)(N * K)), par((size_t)2 * D * K),
        mom((size_t)2 * D * K), bound(1);
    pmm_tables(D, K, hidden | VMP_PMM_FORM_CENTRE, lam_mom.data(), elog_pi.data(), l.data(), lb.data(), c.data(),
               lsum.data());
    pmm_pass(N, D, K, hidden, xp.data(), labelled ? lab.data() : nullptr, l.data(), lb.data(),
             c.data(), S.data(), hidden ? M.data() : nullptr, Nk.data(), scal.data(), r.data());
    pmm_update(D, K, hidden, a0.data(), b0.data(), S.data(), hidden ? M.data() : Nk.data(),
               par.data(), mom.data(), bound.data());
    double total = 0.0, cells = 0.0;
    for (double v : S) total += v;
    if (hidden)
        for (double v : M) cells += v;
    const int flag = flags[0] | flags[1] | flags[2];
    printf("N=%ld D=%d K=%d masked=%d labels=%d flag=%d: sum S = %.12g of %.12g, sum M = %.12g of "
           "%g observed entries, lgam = %.12g, sum lse = %.12g, bound = %.12g\n", (long)N, D, K,
           (int)masked, (int)labelled, flag, total, total_x, cells, observed, lgam, scal[0],
           bound[0]);
    // r sums to one over k, so S adds up to the observed counts and M to the observed entries
    bool ok = flag == 0 && counts[0] == (int64_t)observed
        && fabs(total - total_x) <= 1e-9 * (total_x + 1.0) && std::isfinite(bound[0]);
    if (hidden) ok = ok && fabs(cells - observed) <= 1e-9 * (observed + 1.0);
    return ok ? 0 : 1;
}

int main()
{
    int bad = 0;
    bad += run(333, 131, 5, true, false, 12);
    bad += run(333, 131, 5, false, false, 12);
    bad += run(333, 131, 5, true, true, 12);
    bad += run(64, 7, 64, false, false, VMP_PMM_MAX_COUNT);
    return bad;
}
