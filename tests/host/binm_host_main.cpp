// TEST PROGRAM: tests/host/binm_host.cpp (and tests/host/pmm_host.cpp for the one-plane form) on
// three shapes, stand-alone, for a build with -fsanitize=address,undefined
// (tests/test_binm_host.py).  Exact-size heap buffers, so a read or write past any of them is
// reported.  Shape 1: N = 333, D = 131, K = 5 (neither N nor D a multiple of the tile or of a column
// block, two chunks) with trials per entry, a mask with holes, a row and a column of nothing and
// NaN / -1 / 1e300 at hidden positions; the same without a mask and with labels.  Shape 2: N = 64,
// D = 7, K = 64 with trials per column up to the cap: the one-plane form.
#include <stdio.h>

#include "pmm_host.cpp"
#include "binm_host.cpp"

static int run(int64_t N, int D, int K, bool masked, bool labelled, bool per_entry, uint32_t top)
{
    std::vector<double> x((size_t)(N * D)), elog_p((size_t)2 * D * K), elog_pi(K);
    std::vector<int64_t> trials(per_entry ? (size_t)(N * D) : (size_t)D);
    std::vector<uint8_t> mask((size_t)(N * D));
    std::vector<int32_t> lab((size_t)N);
    uint32_t s = 5227u + (uint32_t)(N * 7 + D * 5 + K);
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return s >> 8; };
    for (int i = 0; i < D * K; ++i) {
        const double p = 0.05 + 0.9 * (double)(rnd() % 1000) / 1000.0;
        elog_p[2 * i] = log(p) - 0.01;
        elog_p[2 * i + 1] = log1p(-p) - 0.01;
    }
    for (auto &v : elog_pi) v = -0.1 - (double)(rnd() % 1000) / 300.0;
    for (auto &t : trials) t = (int64_t)(rnd() % (top + 1));
    if (!per_entry) trials[0] = top;
    const double junk[3] = {NAN, -1.0, 1e300};
    double observed = 0.0, total_x = 0.0, total_n = 0.0;
    for (int64_t n = 0; n < N; ++n) {
        lab[n] = (int32_t)(rnd() % (uint32_t)K);
        for (int d = 0; d < D; ++d) {
            const size_t e = (size_t)(n * D + d);
            const int64_t tn = trials[per_entry ? e : (size_t)d];
            mask[e] = !masked || ((rnd() % 10 < 7) && n != 3 && d != 2);
            x[e] = mask[e] ? (double)(rnd() % (uint32_t)(tn + 1)) : junk[rnd() % 3];
            observed += mask[e];
            if (mask[e]) {
                total_x += x[e];
                total_n += (double)tn;
            }
        }
    }
    std::vector<uint16_t> xp((size_t)(N * D)), np((size_t)(N * D));
    int32_t flags[4] = {0, 0, 0, 0};
    int64_t counts[3];
    double lcoef;
    binm_pack(N, D, 0, x.data(), trials.data(), per_entry ? D : 0, 1,
              masked ? mask.data() : nullptr, xp.data(), np.data(), flags, counts, &lcoef);
    const int one_plane = counts[2] == 1 && counts[1] == 0;
    std::vector<double> ncol(D), l1((size_t)D * K), l0((size_t)D * K), c(K), cfold(K),
        S((size_t)D * K), T((size_t)D * K), Nk(K), cnt((size_t)2 * D * K), scal(2),
        r((size_t)(N * K));
    for (int d = 0; d < D; ++d) ncol[d] = (double)trials[(size_t)d];
    binm_tables(D, K, VMP_BINM_FORM_CENTRE, elog_p.data(), elog_pi.data(), ncol.data(), l1.data(),
                l0.data(), c.data(), cfold.data());
    const int32_t *labels = labelled ? lab.data() : nullptr;
    if (one_plane) {
        pmm_pass(N, D, K, 0, xp.data(), labels, l1.data(), l0.data(), cfold.data(), S.data(),
                 nullptr, Nk.data(), scal.data(), r.data());
        binm_const(D, K, ncol.data(), S.data(), Nk.data(), T.data(), cnt.data());
    } else {
        binm_pass(N, D, K, xp.data(), np.data(), labels, l1.data(), l0.data(), c.data(), S.data(),
                  T.data(), Nk.data(), cnt.data(), scal.data(), r.data());
    }
    double total = 0.0, cells = 0.0;
    for (double v : S) total += v;
    for (double v : T) cells += v;
    const int flag = flags[0] | flags[1] | flags[2] | flags[3];
    printf("N=%ld D=%d K=%d masked=%d labels=%d one_plane=%d flag=%d: sum S = %.12g of %.12g, "
           "sum T = %.12g of %.12g, lcoef = %.12g, sum lse = %.12g\n", (long)N, D, K, (int)masked,
           (int)labelled, one_plane, flag, total, total_x, cells, total_n, lcoef, scal[0]);
    // r sums to one over k, so S adds up to the observed counts and T to the observed trials
    const bool ok = flag == 0 && counts[0] == (int64_t)observed && one_plane == (!per_entry && !masked)
        && fabs(total - total_x) <= 1e-9 * (total_x + 1.0)
        && fabs(cells - total_n) <= 1e-9 * (total_n + 1.0) && std::isfinite(lcoef);
    return ok ? 0 : 1;
}

int main()
{
    int bad = 0;
    bad += run(333, 131, 5, true, false, true, 12);
    bad += run(333, 131, 5, false, false, true, 12);
    bad += run(333, 131, 5, true, true, true, 12);
    bad += run(333, 131, 5, true, false, false, 12);
    bad += run(64, 7, 64, false, false, false, VMP_BINM_MAX_TRIALS);
    return bad;
}
