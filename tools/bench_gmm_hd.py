#!/usr/bin/env python
"""
Times of the high-dimensional form of the fused Gaussian-mixture block (csrc/vmp_gmm_hd.hip), kernel
by kernel through the C ABI: median (min - max) of --steps calls after --warmup, each call between
two device synchronisations.  The pass is also split into its plate kernels and its reduce by the
library's own events (vmp_ctx_set_timing).  At D <= 32 ``vmp_gmm_pass`` runs on the same data in
the same process.  ``--engines`` adds one Q.update() of the model on 'fused+dims' and on the generic
engine at a size the latter still holds.

    python tools/bench_gmm_hd.py [--shapes 1000000x40x16,1000000x64x64,1000000x32x64] [--engines]
                                 [--out profiles/gmm_hd/bench_gmm_hd.json]

fp64 matrix peak used for the fractions: 78.6 Tflop/s (MI355X); each contraction counts
N K DP^2 multiply-adds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

PEAK = 78.6e12


def timed(rt, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(steps):
        rt.synchronize()
        t0 = time.perf_counter()
        fn()
        rt.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return dict(median_ms=float(np.median(out)), min_ms=min(out), max_ms=max(out))


def bench_shape(N, D, K, steps, warmup):
    import gmm_pass_host as H
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.gmm import GMMKernels
    from bayespy_amd.inference.plans.gmm_hd import HighDimGMMKernels
    rt = get_runtime()
    torch = rt.torch
    g = H.make_inputs(4096, D, K)
    rs = np.random.RandomState(3)
    idx = rs.randint(4096, size=N)
    Y = torch.from_numpy(g['y'][idx] + 0.01 * rs.normal(size=(N, D))).to(rt.device)
    rec = dict(N=N, D=D, K=K)
    forms = [('hd', HighDimGMMKernels(rt))] + ([('block', GMMKernels(rt))] if D <= 32 else [])
    for name, k in forms:
        L = k.layout(D, K)
        st = rt.zeros(int(L.total))
        k.init_state(D, K, g['alpha0'], g['beta0'], g['n0'], g['V0'], st)
        for off, key in ((L.off_mu, 'mu'), (L.off_Cmu, 'Cmu'), (L.off_Lam, 'Lam'),
                         (L.off_logdetLam, 'logdetLam'), (L.off_alpha + L.KP, 'logpi')):
            a = torch.from_numpy(np.ascontiguousarray(g[key]).reshape(-1)).to(rt.device)
            st[int(off):int(off) + a.numel()] = a
        R = rt.empty(N, K)
        ws = rt.empty(int(k.workspace_doubles(D, K)))
        r = {}
        r['prepare_z'] = timed(rt, lambda: k.prepare_z(D, K, False, st), steps, warmup)
        # one-hot R + the second-moment kernel + the reduce: the pass without its responsibility kernel
        lab = torch.from_numpy(rs.randint(K, size=N).astype(np.int64)).to(rt.device)
        r['stats_from_labels'] = timed(
            rt, lambda: k.stats_from_labels(Y, N, D, K, lab, R, st, ws), steps, warmup)
        k.set_timing(True)
        r['pass'] = timed(rt, lambda: k.pass_(Y, N, D, K, R, st, ws), steps, warmup)
        rt.synchronize()
        ev = k.pass_times_ms()[-steps:]
        k.set_timing(False)
        r['pass_plate_kernels_ms'] = float(np.median([a for a, _ in ev]))
        r['pass_reduce_ms'] = float(np.median([b for _, b in ev]))
        DP = int(L.DP) if name == 'hd' else D
        r['pass_fraction_of_fp64_matrix_peak'] = \
            2 * 2.0 * N * K * DP * DP / (1e-3 * r['pass_plate_kernels_ms']) / PEAK
        # the per-cluster kernels run from the statistics the pass just left
        for key, fn in (('update_mu', k.update_mu), ('update_lambda', k.update_lambda),
                        ('update_alpha', k.update_alpha), ('lower_bound', k.lower_bound)):
            r[key] = timed(rt, lambda fn=fn: fn(D, K, st), steps, warmup)
        r['status'] = float(st[int(L.off_scal) + 3].cpu())
        rec[name] = r
    return rec


def bench_engines(N, D, K):
    from bayespy_amd.device import get_runtime
    from bayespy_amd.nodes import Categorical, Dirichlet, Gaussian, GaussianARD, Mixture, Wishart
    from bayespy_amd.inference import VB
    rt = get_runtime()
    torch = rt.torch
    rs = np.random.RandomState(5)
    lab = rs.randint(K, size=N)
    y = 3.0 * rs.normal(size=(K, D))[lab] / np.sqrt(D) + rs.normal(size=(N, D))
    out = dict(N=N, D=D, K=K)
    for engine in ('fused+dims', 'generic'):
        alpha = Dirichlet(np.ones(K), name='alpha')
        z = Categorical(alpha, plates=(N,), name='z')
        mu = GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
        Lam = Wishart(D + 2, np.identity(D), plates=(K,), name='Lambda')
        Y = Mixture(z, Gaussian, mu, Lam, plates=(N,), name='Y')
        z.initialize_from_value(lab)
        Y.observe(y)
        Q = VB(Y, mu, Lam, z, alpha, engine=engine)
        Q.ignore_bound_checks = True
        Q.update(repeat=2, verbose=False)
        torch.cuda.reset_peak_memory_stats()
        ts = []
        for _ in range(5):
            rt.synchronize()
            t0 = time.perf_counter()
            Q.update(verbose=False)
            rt.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        out[engine] = dict(update_median_ms=float(np.median(ts)), update_min_ms=min(ts),
                           update_max_ms=max(ts), bound=float(Q.L[Q.iter - 1]),
                           peak_memory_MiB=torch.cuda.max_memory_allocated() / 2 ** 20)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1000000x40x16,1000000x64x64,1000000x32x64')
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--engines', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    res = dict(what='tools/bench_gmm_hd.py: median (min - max) of %d calls after %d'
                    % (a.steps, a.warmup), shapes=[])
    for s in a.shapes.split(','):
        N, D, K = (int(v) for v in s.split('x'))
        res['shapes'].append(bench_shape(N, D, K, a.steps, a.warmup))
        print(json.dumps(res['shapes'][-1]), flush=True)
    if a.engines:
        res['engines'] = bench_engines(2000, 40, 8)
        print(json.dumps(res['engines']), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
