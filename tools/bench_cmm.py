#!/usr/bin/env python
"""
Timed legs of the fused categorical-mixture block (inference/plans/cmm.py); one JSON line each.

  (i)  ms per ``Q.update()`` of the fused block at N = 1e6, D = 32, M = 8, K = 32, with the pass
       kernel's share (``vmp_cmm_pass`` timed alone on the same state) and its rate in table
       lookups (N D K per pass) and count-table updates (as many) per second;
  (ii) at N = 1e5 and the same D, M, K the fused block against the generic engine on the same model
       in the same session, with the peak allocation and the bound of each.

    python tools/bench_cmm.py [--legs i,ii] [--steps 10] [--warmup 3] [--out profiles/cmm/...json]

Every leg warms up, then times ``steps`` updates one by one between device synchronisations and
reports the median and the extremes (the protocol of tools/bench_dgmm.py).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_data(N, D, K, M, seed=0):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    rs = np.random.RandomState(seed)
    p = torch.from_numpy(rs.dirichlet(0.3 * np.ones(M), size=(K, D))).to('cuda')
    x = torch.empty(N, D, dtype=torch.int64, device='cuda')
    step = 1 << 18
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        z = torch.randint(K, (hi - lo,), device='cuda', generator=g)
        x[lo:hi] = torch.multinomial(p[z].reshape(-1, M), 1, generator=g).reshape(hi - lo, D)
    return x, rs.dirichlet(5.0 * np.ones(M), size=(D, K))


def build(x, p0, K, M, engine):
    from bayespy_amd import nodes
    from bayespy_amd.inference import VB
    N, D = x.shape
    R = nodes.Dirichlet(K * [1.0], name='R')
    Z = nodes.Categorical(R, plates=(N, 1), name='Z')
    P = nodes.Dirichlet(M * [0.5], plates=(D, K), name='P')
    X = nodes.Mixture(Z, nodes.Categorical, P, name='X')
    X.observe(x)
    P.initialize_from_value(p0)
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


def leg_fused(N, D, K, M, steps, warmup):
    import torch
    x, p0 = make_data(N, D, K, M)
    torch.cuda.reset_peak_memory_stats()
    Q = build(x, p0, K, M, 'fused')
    plan = Q.plans[0]
    upd = timed(lambda: Q.update(verbose=False), steps, warmup)
    pas = timed(lambda: plan._run_pass(), steps, warmup)
    sec = pas['median_ms'] * 1e-3
    return dict(leg='i', engine='fused', N=N, D=D, K=K, M=M, update=upd, pass_alone=pas,
                pass_share=pas['median_ms'] / upd['median_ms'],
                pass_lookups_per_s=float(N) * D * K / sec,
                pass_count_updates_per_s=float(N) * D * K / sec,
                pass_x_bytes_per_s=float(N) * D / sec,
                chunk_rows=int(plan.chunk), x_bytes=int(x.numel() * 8), packed_bytes=int(N * D),
                ndk_bytes=int(8 * N * D * K),
                peak_alloc_bytes=int(torch.cuda.max_memory_allocated()),
                L=float(Q.L[Q.iter - 1]))


def leg_compare(N, D, K, M, steps, warmup):
    import torch
    x, p0 = make_data(N, D, K, M)
    x = x.cpu().numpy()                 # both engines from the same host array
    out = dict(leg='ii', N=N, D=D, K=K, M=M, x_bytes=int(x.size * 8),
               ndk_bytes=int(8 * N * D * K), ndkm_bytes=int(8 * N * D * K * M))
    for engine in ('fused', 'generic'):
        torch.cuda.reset_peak_memory_stats()
        Q = build(x, p0, K, M, engine)
        out[engine] = timed(lambda: Q.update(verbose=False), steps, warmup)
        out[engine]['plan'] = type(Q.plans[0]).__name__
        out[engine]['peak_alloc_bytes'] = int(torch.cuda.max_memory_allocated())
        out[engine]['L'] = float(Q.L[Q.iter - 1])
        del Q
    out['generic_over_fused'] = out['generic']['median_ms'] / out['fused']['median_ms']
    out['fused_not_slower'] = out['fused']['median_ms'] <= out['generic']['median_ms']
    out['fused_peak_below_one_ndk_array'] = \
        out['fused']['peak_alloc_bytes'] < out['ndk_bytes']
    out['L_relative_difference'] = abs(out['fused']['L'] - out['generic']['L']) \
        / abs(out['generic']['L'])
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
            r = leg_fused(10 ** 6, 32, 32, 8, a.steps, a.warmup)
        elif leg == 'ii':
            r = leg_compare(10 ** 5, 32, 32, 8, a.steps, a.warmup)
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
