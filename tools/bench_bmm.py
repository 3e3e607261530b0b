#!/usr/bin/env python
"""
Timed legs of the fused Bernoulli-mixture block (inference/plans/bmm.py); one JSON line each.

  (i)  ms per ``Q.update()`` of the fused block at N = 1e7, D = 64, K = 32 and at N = 1e6,
       D = 1024, K = 64, with the pass kernel's share (``vmp_bmm_pass`` timed alone on the same
       state) and its fraction of the fp64 matrix peak (4 N D K flops);
  (ii) at N = 1e5, D = 64, K = 32 the fused block against the generic engine (the largest size at
       which the generic engine's (N, D, K) arrays, 1.6 GB each, fit comfortably);
  (m)  the same three legs with 30 % of the entries hidden by a mask of the full shape (m1, m2,
       mii): the masked pass does twice the matrix work (8 N D K flops).

    python tools/bench_bmm.py [--legs i1,i2,ii,m1,m2,mii] [--steps 10] [--warmup 3] [--out profiles/...json]

Every leg warms up, then times ``steps`` updates one by one between device synchronisations and
reports the median and the spread.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP64_MATRIX_PEAK_TFLOPS = 78.6          # MI355X, dense fp64 matrix


def make_data(N, D, K, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    p = torch.rand(K, D, device='cuda', generator=g, dtype=torch.float64)
    x = torch.empty(N, D, dtype=torch.bool, device='cuda')
    step = max(1, (1 << 24) // D)
    for lo in range(0, N, step):                # no (N, D) array of doubles
        hi = min(N, lo + step)
        z = torch.randint(K, (hi - lo,), device='cuda', generator=g)
        x[lo:hi] = torch.rand(hi - lo, D, device='cuda', generator=g, dtype=torch.float32) \
            < p[z].float()
    return x.cpu().numpy()          # observe() checks host arrays; the plan uploads the bits


def make_mask(N, D, hidden, seed=1):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    m = torch.empty(N, D, dtype=torch.bool, device='cuda')
    step = max(1, (1 << 24) // D)
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        m[lo:hi] = torch.rand(hi - lo, D, device='cuda', generator=g) >= hidden
    return m.cpu().numpy()


def build(x, K, engine, mask=None):
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    N, D = x.shape
    R = nodes.Dirichlet(K * [1.0], name='R')
    Z = nodes.Categorical(R, plates=(N, 1), name='Z')
    P = nodes.Beta([0.5, 0.5], plates=(D, K), name='P')
    X = nodes.Mixture(Z, nodes.Bernoulli, P, name='X')
    if mask is None:
        X.observe(x)
    else:
        X.observe(x * mask, mask=mask)
    P.initialize_from_random()
    return VB(Z, R, X, P, engine=engine)


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


def leg_fused(tag, N, D, K, steps, warmup, hidden=0.0):
    import torch
    x = make_data(N, D, K)
    mask = make_mask(N, D, hidden) if hidden else None
    Q = build(x, K, 'fused', mask)
    plan = Q.plans[0]
    upd = timed(lambda: Q.update(verbose=False), steps, warmup)
    pas = timed(lambda: plan._run_pass(), steps, warmup)
    flops = (8.0 if hidden else 4.0) * N * D * K
    out = dict(leg=tag, engine='fused', N=N, D=D, K=K, hidden=hidden, update=upd, pass_alone=pas,
               pass_share=pas['median_ms'] / upd['median_ms'],
               pass_tflops=flops / (pas['median_ms'] * 1e-3) / 1e12,
               chunk_rows=int(plan.chunk), x_bytes=int(plan.xw.numel() * 8),
               peak_alloc_bytes=int(torch.cuda.max_memory_allocated()))
    out['pass_fraction_of_fp64_matrix_peak'] = out['pass_tflops'] / FP64_MATRIX_PEAK_TFLOPS
    return out


def leg_compare(N, D, K, steps, warmup, hidden=0.0):
    x = make_data(N, D, K)
    mask = make_mask(N, D, hidden) if hidden else None
    out = dict(leg='mii' if hidden else 'ii', N=N, D=D, K=K, hidden=hidden)
    for engine in ('fused', 'generic'):
        Q = build(x if engine == 'fused' else x.astype(np.int64), K, engine, mask)
        out[engine] = timed(lambda: Q.update(verbose=False), steps, warmup)
        out[engine]['plan'] = type(Q.plans[0]).__name__
    out['generic_over_fused'] = out['generic']['median_ms'] / out['fused']['median_ms']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='i1,i2,ii')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lines = []
    for leg in a.legs.split(','):
        np.random.seed(0)
        if leg == 'i1':
            r = leg_fused('i1', 10 ** 7, 64, 32, a.steps, a.warmup)
        elif leg == 'i2':
            r = leg_fused('i2', 10 ** 6, 1024, 64, a.steps, a.warmup)
        elif leg == 'ii':
            r = leg_compare(10 ** 5, 64, 32, a.steps, a.warmup)
        elif leg == 'm1':
            r = leg_fused('m1', 10 ** 7, 64, 32, a.steps, a.warmup, hidden=0.3)
        elif leg == 'm2':
            r = leg_fused('m2', 10 ** 6, 1024, 64, a.steps, a.warmup, hidden=0.3)
        elif leg == 'mii':
            r = leg_compare(10 ** 5, 64, 32, a.steps, a.warmup, hidden=0.3)
        else:
            raise SystemExit('unknown leg %r' % leg)
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
