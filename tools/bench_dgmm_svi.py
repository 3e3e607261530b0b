#!/usr/bin/env python
"""
Time one step of stochastic variational inference on a diagonal-Gaussian mixture: ``Y.observe`` of a
resident device batch, ``Q.update(Z)``, ``Q.gradient_step(mu, tau, alpha)``.

    python tools/bench_dgmm_svi.py [--steps 15] [--warmup 3] [--out profiles/dgmm_svi]

Shape: N_batch = 65536, D = 64, K = 32 (``--small`` adds the golden shape 70, 5, 3).  Legs:
``engine='fused+batches+gaussian'`` (DiagGaussianMixtureSVIPlan), ``engine='generic'`` for the same
model, and ``vmp_dgmm_natural_step`` alone.  After the warm-up every step is timed on its own
between device synchronisations.  Median and min-max, the peak allocated device memory of both
engines (above what was allocated before the model was built) and, for the fused leg, the C-ABI
calls and kernel launches of one step go to one JSON line per leg under ``--out``.  The launches
are counted from the calls with the table ``LAUNCHES`` (read off csrc/vmp_dgmm.hip, vmp_lda.hip and
vmp_dgmm_svi.hip); ``VB.update(Z)`` evaluates the bound after the update, and those launches are
listed apart.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [dict(name='large', NB=65536, D=64, K=32)]
SMALL = dict(name='golden', NB=70, D=5, K=3)
# kernel launches behind an entry point of DGMMKernels: the pass is the pass kernel, the combine, three
# dot products of two launches each and one add
LAUNCHES = dict(tables=1, pass_=9, natural_step=1, dot=2, update=1, dirichlet=1)


def _stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)),
                calls=len(ms))


class _Counting:
    """Proxy of a kernels object that lists the entry points called."""

    def __init__(self, kernels):
        self._k, self.calls = kernels, []

    def __getattr__(self, name):
        fn = getattr(self._k, name)
        if not callable(fn) or name in ('plan', 'natural_step_workspace'):
            return fn

        def go(*a, **kw):
            self.calls.append(name)
            return fn(*a, **kw)
        return go


def _model(engine, NB, D, K, data):
    from bayespy_amd.nodes import GaussianARD, Gamma, Dirichlet, Categorical, Mixture
    from bayespy_amd.inference import VB
    alpha = Dirichlet(np.ones(K), name='class probabilities')
    Z = Categorical(alpha, plates=(NB, 1), plates_multiplier=(20.0, 1), name='classes')
    mu = GaussianARD(0, 0.01, plates=(D, K), name='means')
    tau = Gamma(1.0, 1.0, plates=(D, K), name='precisions')
    Y = Mixture(Z, GaussianARD, mu, tau, name='observations')
    mu.initialize_from_value(3.0 * np.random.RandomState(1).randn(D, K))
    Y.observe(data[0])
    Q = VB(Y, Z, mu, tau, alpha, engine=engine)
    Q.ignore_bound_checks = True
    return Q, Y, Z, mu, tau, alpha


def time_engine(engine, shp, steps, warmup):
    import gc
    import torch
    NB, D, K = shp['NB'], shp['D'], shp['K']
    rs = np.random.RandomState(0)
    data = [torch.from_numpy(3.0 * rs.randn(K, D)[rs.randint(K, size=NB)] + rs.randn(NB, D)).cuda()
            for _ in range(2)]
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()          # the batches, and whatever an earlier leg left
    Q, Y, Z, mu, tau, alpha = _model(engine, NB, D, K, data)
    plan = Q.plans[0]
    counting = None
    ms = []
    for n in range(warmup + steps):
        if n == warmup and engine != 'generic':
            counting = plan._kernels = _Counting(plan.kernels)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Y.observe(data[n % 2])
        Q.update(Z, verbose=False)
        Q.gradient_step(mu, tau, alpha, scale=(n + 1) ** (-0.7))
        torch.cuda.synchronize()
        if n >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    out = _stats(ms)
    out.update(leg=engine, plan=type(plan).__name__,
               peak_allocated_mb=(torch.cuda.max_memory_allocated() - base) / 2 ** 20)
    if counting is not None:
        per = len(counting.calls) // steps
        one = counting.calls[:per]
        # the step proper: the tables and the pass of update(Z), the natural-gradient step; the rest
        # is the bound VB.update evaluates after the update
        first_pass = one.index('pass_')
        step = one[:first_pass + 1] + [c for c in one if c == 'natural_step']
        rest = one[first_pass + 1:]
        rest.remove('natural_step')
        out.update(calls_per_step=step, launches_per_step=sum(LAUNCHES[c] for c in step),
                   calls_of_the_bound=rest, launches_of_the_bound=sum(LAUNCHES[c] for c in rest))
    return out


def time_kernel(shp, steps, warmup):
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.dgmm import DGMMKernels
    D, K = shp['D'], shp['K']
    rt = get_runtime()
    k = DGMMKernels(rt)
    rs = np.random.RandomState(2)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(rt.device)  # noqa: E731
    m0, beta0, a0, b0 = (up(np.full((D, K), v)) for v in (0.0, 0.01, 1.0, 1.0))
    S1, S2, Nk = up(rs.randn(D, K) * 100), up(rs.gamma(2.0, 200.0, size=(D, K))), \
        up(rs.gamma(2.0, 50.0, size=K))
    tabs = [rt.empty(D * K, 2) for _ in range(4)]
    prior_r, alpha_r, elog_r = up(np.ones(K)), rt.empty(K), rt.empty(K)
    ws, bound = rt.empty(k.natural_step_workspace(D, K)), rt.empty(3)
    rt.sync_stream()
    k.natural_step(D, K, 7, m0, beta0, a0, b0, None, None, None, 0, *tabs, prior_r, None, alpha_r,
                   elog_r, 1.0, 1.0, ws, bound)         # the priors
    ms = []
    for n in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        k.natural_step(D, K, 7, m0, beta0, a0, b0, S1, S2, Nk, 0, *tabs, prior_r, Nk, alpha_r,
                       elog_r, 20.0, 0.5, ws, bound)
        torch.cuda.synchronize()
        if n >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    out = _stats(ms)
    out.update(leg='kernel')
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=os.path.join('profiles', 'dgmm_svi'))
    ap.add_argument('--small', action='store_true')
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, 'bench_dgmm_svi.jsonl'), 'w') as f:
        for shp in SHAPES + ([SMALL] if a.small else []):
            for leg in ('fused+batches+gaussian', 'generic', 'kernel'):
                r = time_kernel(shp, a.steps, a.warmup) if leg == 'kernel' \
                    else time_engine(leg, shp, a.steps, a.warmup)
                r.update(shape=shp['name'], NB=shp['NB'], D=shp['D'], K=shp['K'])
                line = json.dumps(r)
                print(line, flush=True)
                f.write(line + '\n')


if __name__ == '__main__':
    main()
