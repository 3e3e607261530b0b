#!/usr/bin/env python
"""
Timed legs of the fused binomial-mixture block (inference/plans/binm.py); one JSON line per shape,
the protocol of tools/bench_pmm.py.

Per shape (N = 1e6, D = 256, K = 32 and N = 1e5, D = 64, K = 32) the plate pass alone through the C
ABI on device-made data, each form next to the Poisson block's pass at the same shape:

  * ``vmp_binm_pass`` two planes (trials per entry, three in ten entries hidden) beside
    ``vmp_pmm_pass`` hidden = 1;
  * ``vmp_binm_pass`` one plane (trials per column, nothing hidden) beside ``vmp_pmm_pass``
    hidden = 0 (the same kernel);

with the fraction of the fp64 matrix peak (4 N D K flops per statistic-product pair: 8 N D K for two
statistics) and the bytes read per entry (2 per plane and read of the planes: above one column block
the planes are read twice).  At the small shape also ms per ``Q.update()`` of the block and of the
generic engine on the same model.

    python tools/bench_binm.py [--steps 10] [--warmup 3] [--out profiles/binm/bench_binm.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_dgmm import timed, FP64_MATRIX_PEAK_TFLOPS, HBM_TBPS                         # noqa: E402


def make_data(N, D, K, seed=0):
    """Counts x (N, D) int32 out of trials n (N, D) int64 near 15 on the device from K probability
    vectors, and the probabilities (K, D)."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    p = torch.rand(K, D, device='cuda', generator=g, dtype=torch.float64) * 0.9 + 0.05
    x = torch.empty(N, D, dtype=torch.int32, device='cuda')
    n = torch.empty(N, D, dtype=torch.int64, device='cuda')
    step = max(1, (1 << 24) // D)
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        z = torch.randint(K, (hi - lo,), device='cuda', generator=g)
        nn = torch.poisson(torch.full((hi - lo, D), 15.0, device='cuda', dtype=torch.float64),
                           generator=g)
        n[lo:hi] = nn.to(torch.int64)
        x[lo:hi] = torch.binomial(nn, p[z], generator=g).to(torch.int32)
    return x, n, p.cpu().numpy()


def leg_passes(N, D, K, steps, warmup):
    import torch
    from scipy.special import digamma
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.binm import BINMKernels
    from bayespy_amd.inference.plans.pmm import PMMKernels
    rt = get_runtime()
    kb, kp = BINMKernels(rt), PMMKernels(rt)
    x, n, p = make_data(N, D, K)
    g = torch.Generator(device='cuda').manual_seed(1)
    mask = (torch.rand(N, D, device='cuda', generator=g) >= 0.3).to(torch.uint8)
    a, b = 60.0 * p.T + 0.5, 60.0 * (1 - p.T) + 0.5
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(rt.device)      # noqa: E731
    elog_p = up(np.stack([digamma(a) - digamma(a + b), digamma(b) - digamma(a + b)],
                         -1).reshape(D * K, 2))
    elog_pi = up(np.full(K, -np.log(K)))
    chunk, wsd = kb.plan(N, D, K)
    ws = rt.empty(int(wsd))
    S, T, Nk, cnt, scal = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K), rt.zeros(D * K, 2), \
        rt.zeros(8)
    l1, l0, c, cf = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K), rt.zeros(K)
    out = dict(N=N, D=D, K=K, chunk_rows=int(chunk))

    def pack(trials, ts_n, ts_d, m):
        xp = torch.zeros(N * D, dtype=torch.int16, device=rt.device)
        np_ = torch.zeros(N * D, dtype=torch.int16, device=rt.device)
        flags = torch.zeros(4, dtype=torch.int32, device=rt.device)
        counts = torch.zeros(3, dtype=torch.int64, device=rt.device)
        lcoef = rt.zeros(1)
        t = timed(lambda: kb.pack(N, D, 3, x, trials, ts_n, ts_d, m, xp, np_, flags, counts, lcoef,
                                  ws), steps, warmup)
        assert not flags.cpu().numpy().any()
        return xp, np_, counts.cpu().numpy(), t

    def rates(ms, stats, planes, block):
        reads = 1 if D <= block else 2
        sec = ms * 1e-3
        tf = 4.0 * stats * N * D * K / sec / 1e12
        by = 2.0 * planes * reads
        return dict(tflops=tf, fraction_of_fp64_matrix_peak=tf / FP64_MATRIX_PEAK_TFLOPS,
                    bytes_per_entry=by, tbps=by * N * D / sec / 1e12,
                    fraction_of_hbm_rate=by * N * D / sec / 1e12 / HBM_TBPS)
    # two planes: trials per entry, hidden entries
    xp, np_, counts, tp = pack(n, D, 1, mask)
    assert counts[1] > 0 and counts[2] == 0
    kb.tables(D, K, 1, elog_p, elog_pi, None, l1, l0, c, None)
    two = timed(lambda: kb.pass_(N, D, K, 0, xp, np_, None, None, l1, l0, c, ws, S, T, Nk, cnt,
                                 scal), steps, warmup)
    out['pack_two_planes'] = tp
    out['binm_two_planes'] = dict(pass_alone=two, **rates(two['median_ms'], 2, 2, 64))
    # the Poisson pass with hidden entries on the same counts
    xq = torch.zeros(N * D, dtype=torch.int16, device=rt.device)
    f3 = torch.zeros(3, dtype=torch.int32, device=rt.device)
    c2 = torch.zeros(2, dtype=torch.int64, device=rt.device)
    kp.pack(N, D, 3, x, mask, xq, f3, c2, rt.zeros(1), ws)
    ph = timed(lambda: kp.pass_(N, D, K, 1, xq, None, l1, l0, c, ws, S, T, Nk, scal), steps, warmup)
    out['pmm_hidden'] = dict(pass_alone=ph, **rates(ph['median_ms'], 2, 1, 64))
    out['two_planes_over_pmm_hidden'] = two['median_ms'] / ph['median_ms']
    # one plane: trials per column, nothing hidden
    ncol_i = torch.full((D,), 40, dtype=torch.int64, device=rt.device)
    xp, np_, counts, _ = pack(ncol_i, 0, 1, None)
    assert counts[1] == 0 and counts[2] == 1
    ncol = ncol_i.to(torch.float64)
    kb.tables(D, K, 1, elog_p, elog_pi, ncol, l1, l0, c, cf)
    one = timed(lambda: kb.pass_(N, D, K, 1, xp, np_, ncol, None, l1, l0, cf, ws, S, T, Nk, cnt,
                                 scal), steps, warmup)
    out['binm_one_plane'] = dict(pass_alone=one, **rates(one['median_ms'], 1, 1, 128))
    pn = timed(lambda: kp.pass_(N, D, K, 0, xp, None, l1, l0, cf, ws, S, T, Nk, scal), steps,
               warmup)
    out['pmm_nothing_hidden'] = dict(pass_alone=pn, **rates(pn['median_ms'], 1, 1, 128))
    out['one_plane_over_pmm'] = one['median_ms'] / pn['median_ms']
    return out


def leg_updates(N, D, K, steps, warmup):
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    x, n, p = make_data(N, D, K)
    x, n = x.cpu().numpy(), n.cpu().numpy()[:, :, None]
    out = dict(leg='update', N=N, D=D, K=K)
    for engine in ('fused', 'generic'):
        R = nodes.Dirichlet(K * [1.0], name='R')
        Z = nodes.Categorical(R, plates=(N, 1), name='Z')
        P = nodes.Beta([0.5, 0.5], plates=(D, K), name='P')
        X = nodes.Mixture(Z, nodes.Binomial, n, P, name='X')
        X.observe(x)
        P.initialize_from_value(np.clip(p.T + 0.02 * np.random.RandomState(1).normal(size=(D, K)),
                                        0.02, 0.98))
        Q = VB(Z, R, X, P, engine=engine)
        out[engine] = timed(lambda: Q.update(verbose=False), steps, warmup)
        out[engine]['plan'] = type(Q.plans[0]).__name__
        out[engine]['L'] = float(Q.L[Q.iter - 1])
        del Q
    out['generic_over_fused'] = out['generic']['median_ms'] / out['fused']['median_ms']
    out['bounds_rel_diff'] = abs(out['fused']['L'] - out['generic']['L']) / abs(out['generic']['L'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default='profiles/binm/bench_binm.json')
    a = ap.parse_args()
    lines = []
    for N, D, K in ((10 ** 6, 256, 32), (10 ** 5, 64, 32)):
        lines.append(json.dumps(leg_passes(N, D, K, a.steps, a.warmup)))
        print(lines[-1], flush=True)
    lines.append(json.dumps(leg_updates(10 ** 5, 64, 32, a.steps, a.warmup)))
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
