#!/usr/bin/env python
"""
Timed legs of the fused diagonal-Gaussian-mixture block (inference/plans/dgmm.py); one JSON line
each.

  (i)  ms per ``Q.update()`` of the fused block at N = 1e6, D = 256, K = 32, with the pass kernel's
       share (``vmp_dgmm_pass`` timed alone on the same state), its fraction of the fp64 matrix peak
       (8 N D K flops) and of the HBM rate (16 N D bytes: above D = 64 y is read twice);
  (ii) at N = 1e5, D = 64, K = 32 the fused block against the generic engine on the same model in
       the same session, with the peak allocation of each.

    python tools/bench_dgmm.py [--legs i,ii] [--steps 10] [--warmup 3] [--out profiles/dgmm/...json]

Every leg warms up, then times ``steps`` updates one by one between device synchronisations and
reports the median and the extremes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK_TFLOPS = 78.6          # MI355X, dense fp64 matrix
HBM_TBPS = 8.0                          # MI355X, HBM3E


def make_data(N, D, K, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    centres = 3.0 * torch.randn(K, D, device='cuda', generator=g, dtype=torch.float64)
    y = torch.empty(N, D, dtype=torch.float64, device='cuda')
    step = max(1, (1 << 24) // D)
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        z = torch.randint(K, (hi - lo,), device='cuda', generator=g)
        y[lo:hi] = centres[z] + torch.randn(hi - lo, D, device='cuda', generator=g,
                                            dtype=torch.float64)
    return y, centres.cpu().numpy()


def build(y, centres, K, engine):
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    N, D = y.shape
    alpha = nodes.Dirichlet(K * [1.0], name='alpha')
    Z = nodes.Categorical(alpha, plates=(N, 1), name='Z')
    mu = nodes.GaussianARD(0.0, 1e-3, plates=(D, K), name='mu')
    tau = nodes.Gamma(1e-2, 1e-2, plates=(D, K), name='tau')
    Y = nodes.Mixture(Z, nodes.GaussianARD, mu, tau, name='Y')
    Y.observe(y)
    mu.initialize_from_value(centres.T + 0.5 * np.random.RandomState(1).normal(size=(D, K)))
    return VB(Y, Z, mu, tau, alpha, engine=engine)


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
                steps=steps, warmup=warmup)


def leg_fused(tag, N, D, K, steps, warmup):
    import torch
    y, centres = make_data(N, D, K)
    torch.cuda.reset_peak_memory_stats()
    Q = build(y, centres, K, 'fused')
    plan = Q.plans[0]
    upd = timed(lambda: Q.update(verbose=False), steps, warmup)
    pas = timed(lambda: plan._run_pass(), steps, warmup)
    reads = 1 if D <= 64 else 2
    sec = pas['median_ms'] * 1e-3
    out = dict(leg=tag, engine='fused', N=N, D=D, K=K, update=upd, pass_alone=pas,
               pass_share=pas['median_ms'] / upd['median_ms'],
               pass_tflops=8.0 * N * D * K / sec / 1e12,
               pass_tbps=8.0 * reads * N * D / sec / 1e12, y_reads=reads,
               chunk_rows=int(plan.chunk), y_bytes=int(y.numel() * 8),
               ndk_bytes=int(8 * N * D * K),
               peak_alloc_bytes=int(torch.cuda.max_memory_allocated()))
    out['pass_fraction_of_fp64_matrix_peak'] = out['pass_tflops'] / FP64_MATRIX_PEAK_TFLOPS
    out['pass_fraction_of_hbm_rate'] = out['pass_tbps'] / HBM_TBPS
    out['holds_no_ndk_array'] = out['peak_alloc_bytes'] - out['y_bytes'] < out['ndk_bytes']
    return out


def leg_compare(N, D, K, steps, warmup):
    import torch
    y, centres = make_data(N, D, K)
    out = dict(leg='ii', N=N, D=D, K=K, y_bytes=int(y.numel() * 8), ndk_bytes=int(8 * N * D * K))
    for engine in ('fused', 'generic'):
        torch.cuda.reset_peak_memory_stats()
        Q = build(y, centres, K, engine)
        out[engine] = timed(lambda: Q.update(verbose=False), steps, warmup)
        out[engine]['plan'] = type(Q.plans[0]).__name__
        out[engine]['peak_alloc_bytes'] = int(torch.cuda.max_memory_allocated())
        out[engine]['L'] = float(Q.L[Q.iter - 1])
        del Q
    out['generic_over_fused'] = out['generic']['median_ms'] / out['fused']['median_ms']
    out['fused_holds_no_ndk_array'] = \
        out['fused']['peak_alloc_bytes'] - out['y_bytes'] < out['ndk_bytes']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='i,ii')
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
            r = leg_compare(10 ** 5, 64, 32, a.steps, a.warmup)
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
