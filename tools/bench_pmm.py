#!/usr/bin/env python
"""
Timed legs of the fused Poisson-mixture block (inference/plans/pmm.py); one JSON line each, the
protocol of tools/bench_dgmm.py.

  (i)   ms per ``Q.update()`` of the fused block at N = 1e6, D = 256, K = 32, with the pass kernel's
        share (``vmp_pmm_pass`` timed alone on the same state), its fraction of the fp64 matrix peak
        (4 N D K flops) and of the HBM rate (2 N D bytes per read of x: above one column block of
        128 x is read twice);
  (ii)  the same at N = 1e5, D = 64, K = 32;
  (iii) at N = 1e5, D = 64, K = 32 the fused block against the generic engine on the same model in
        the same session, with the peak allocation and the bound of each;
  (iv)  at N = 1e5, D = 64, K = 32 ``vmp_dgmm_pass`` (the diagonal-Gaussian block on the same counts
        as doubles), the yardstick of the sibling pass.

    python tools/bench_pmm.py [--legs i,ii,iii,iv] [--steps 10] [--warmup 3] [--out profiles/pmm/...json]

Every leg warms up, then times ``steps`` calls one by one between device synchronisations and
reports the median and the extremes.
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
    """Counts (N, D) int32 on the device from K rate vectors near 5, and the rates (K, D)."""
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    rates = 5.0 * torch.exp(0.5 * torch.randn(K, D, device='cuda', generator=g,
                                              dtype=torch.float64))
    x = torch.empty(N, D, dtype=torch.int32, device='cuda')
    step = max(1, (1 << 24) // D)
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        z = torch.randint(K, (hi - lo,), device='cuda', generator=g)
        x[lo:hi] = torch.poisson(rates[z], generator=g).to(torch.int32)
    return x, rates.cpu().numpy()


def build(x, rates, K, engine):
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    N, D = x.shape
    R = nodes.Dirichlet(K * [1.0], name='R')
    Z = nodes.Categorical(R, plates=(N, 1), name='Z')
    lam = nodes.Gamma(1e-2, 1e-2, plates=(D, K), name='lam')
    X = nodes.Mixture(Z, nodes.Poisson, lam, name='X')
    X.observe(x.cpu().numpy())              # the node checks its values on the host
    lam.initialize_from_value(rates.T * np.exp(0.1 * np.random.RandomState(1).normal(size=(D, K))))
    return VB(Z, R, X, lam, engine=engine)


def leg_fused(tag, N, D, K, steps, warmup):
    import torch
    x, rates = make_data(N, D, K)
    torch.cuda.reset_peak_memory_stats()
    Q = build(x, rates, K, 'fused')
    plan = Q.plans[0]
    upd = timed(lambda: Q.update(verbose=False), steps, warmup)
    pas = timed(lambda: plan._run_pass(), steps, warmup)
    reads = 1 if D <= 128 else 2
    sec = pas['median_ms'] * 1e-3
    out = dict(leg=tag, engine='fused', N=N, D=D, K=K, hidden=int(plan.hidden), update=upd,
               pass_alone=pas, pass_share=pas['median_ms'] / upd['median_ms'],
               pass_tflops=4.0 * N * D * K / sec / 1e12,
               pass_tbps=2.0 * reads * N * D / sec / 1e12, x_reads=reads,
               flops_per_byte=4.0 * K / (2.0 * reads), chunk_rows=int(plan.chunk),
               x_bytes=int(x.numel() * 4), ndk_bytes=int(8 * N * D * K),
               peak_alloc_bytes=int(torch.cuda.max_memory_allocated()),
               L=float(Q.L[Q.iter - 1]))
    out['pass_fraction_of_fp64_matrix_peak'] = out['pass_tflops'] / FP64_MATRIX_PEAK_TFLOPS
    out['pass_fraction_of_hbm_rate'] = out['pass_tbps'] / HBM_TBPS
    out['holds_no_ndk_array'] = out['peak_alloc_bytes'] - out['x_bytes'] < out['ndk_bytes']
    return out


def leg_compare(N, D, K, steps, warmup):
    import torch
    x, rates = make_data(N, D, K)
    out = dict(leg='iii', N=N, D=D, K=K, x_bytes=int(x.numel() * 4), ndk_bytes=int(8 * N * D * K))
    for engine in ('fused', 'generic'):
        torch.cuda.reset_peak_memory_stats()
        Q = build(x, rates, K, engine)
        out[engine] = timed(lambda: Q.update(verbose=False), steps, warmup)
        out[engine]['plan'] = type(Q.plans[0]).__name__
        out[engine]['peak_alloc_bytes'] = int(torch.cuda.max_memory_allocated())
        out[engine]['L'] = float(Q.L[Q.iter - 1])
        del Q
    out['generic_over_fused'] = out['generic']['median_ms'] / out['fused']['median_ms']
    out['bounds_rel_diff'] = abs(out['fused']['L'] - out['generic']['L']) / abs(out['generic']['L'])
    out['fused_holds_no_ndk_array'] = \
        out['fused']['peak_alloc_bytes'] - out['x_bytes'] < out['ndk_bytes']
    return out


def leg_dgmm_pass(N, D, K, steps, warmup):
    """``vmp_dgmm_pass`` alone on the same shape: the counts as doubles, zero tables."""
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.dgmm import DGMMKernels
    x, _ = make_data(N, D, K)
    rt = get_runtime()
    k = DGMMKernels(rt)
    y = x.to(torch.float64)
    chunk, wsd = k.plan(N, D, K)
    h, q, c = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
    S1, S2, Nk, scal, ws = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K), rt.zeros(8), rt.empty(wsd)
    pas = timed(lambda: k.pass_(N, D, K, y, None, h, q, c, ws, S1, S2, Nk, scal), steps, warmup)
    return dict(leg='iv', kernel='vmp_dgmm_pass', N=N, D=D, K=K, pass_alone=pas)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='i,ii,iii,iv')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for leg in a.legs.split(','):
        np.random.seed(0)
        if leg == 'i':
            r = leg_fused('i', 10 ** 6, 256, 32, a.steps, a.warmup)
        elif leg == 'ii':
            r = leg_fused('ii', 10 ** 5, 64, 32, a.steps, a.warmup)
        elif leg == 'iii':
            r = leg_compare(10 ** 5, 64, 32, a.steps, a.warmup)
        elif leg == 'iv':
            r = leg_dgmm_pass(10 ** 5, 64, 32, a.steps, a.warmup)
        else:
            raise SystemExit('unknown leg %r' % leg)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
