#!/usr/bin/env python
"""
Timed legs of the fused hidden-Markov-model block (inference/plans/hmm.py); one JSON line each.

At B = 2e4 chains, T = 1000 steps, D = 2, K = 8 with learned emissions (the model script of
tests/hmm_models.py, Z from fixed random labels):
  fused    ms per ``Q.update()`` with engine='fused';
  pass     ``vmp_hmm_fused_pass`` alone on the same state, with its bytes per chain step (y read
           twice, the forward state written and read once: 16 D + 16 K) and the exponentials per
           second ((3 K + 2) K per chain step);
  generic  ms per ``Q.update()`` of the same script with engine='generic' (the yardstick: logP and
           zz of shape (B, T-1, K, K), 10 GB each).

  masked   (with --observed and / or --ragged) ``vmp_hmm_fused_pass_masked`` on the same state
           after ``Y.observe(y, mask=m)``: one line per mask -- a fraction of the steps observed at
           random (1.0 is a mask of ones), or sequence lengths uniform in 1 ... T as trailing masks;
           NaN stands at the masked positions.  Without --out these lines (and the unmasked pass
           of the same build before them) go to profiles/hmm_fused/bench_hmm_masked.json.

    python tools/bench_hmm_fused.py [--legs fused,pass,generic] [--B 20000] [--T 1000] [--steps 5]
                                    [--warmup 2] [--out profiles/...json]
    python tools/bench_hmm_fused.py --legs pass --observed 1.0,0.7 --ragged

Every leg warms up, then times ``steps`` calls one by one between device synchronisations and
reports the median and the extremes.
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


def make_data(B, T, D, K, seed=0):
    rs = np.random.RandomState(seed)
    mu = 5.0 * rs.normal(size=(K, D))
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(K, size=B)
    for t in range(1, T):                           # sticky chains
        z[:, t] = np.where(rs.rand(B) < 0.9, z[:, t - 1], rs.randint(K, size=B))
    y = mu[z] + rs.normal(size=(B, T, D))
    return y, mu, rs.randint(K, size=(B, T))


def build(y, mu, z0, engine):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from hmm_models import build_hmm
    m = build_hmm(dict(nodes=nodes), y, mu, None, learned=True)
    m['Z'].initialize_from_value(z0)
    Q = VB(m['Y'], m['mu'], m['Lambda'], m['A'], m['a0'], m['Z'], engine=engine)
    Q.ignore_bound_checks = True
    return Q


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
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)),
                steps=steps, warmup=warmup)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='fused,pass,generic')
    ap.add_argument('--B', type=int, default=20000)
    ap.add_argument('--T', type=int, default=1000)
    ap.add_argument('--D', type=int, default=2)
    ap.add_argument('--K', type=int, default=8)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    ap.add_argument('--observed', default=None,
                    help='comma-separated fractions of observed steps for the masked pass')
    ap.add_argument('--ragged', action='store_true',
                    help='masked pass with sequence lengths uniform in 1 ... T')
    a = ap.parse_args()
    import torch
    B, T, D, K = a.B, a.T, a.D, a.K
    y, mu, z0 = make_data(B, T, D, K)
    shape = dict(B=B, T=T, D=D, K=K)
    lines = []

    def emit(rec):
        rec = dict(shape, **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    legs = a.legs.split(',')
    masks = [('observed %g' % float(f), float(f)) for f in (a.observed or '').split(',') if f]
    if a.ragged:
        masks.append(('ragged', None))
    if masks and 'pass' not in legs:
        legs.append('pass')
    if masks and a.out is None:
        a.out = os.path.join(ROOT, 'profiles', 'hmm_fused', 'bench_hmm_masked.json')
    if 'fused' in legs or 'pass' in legs:
        Q = build(y, mu, z0, 'fused')
        plan = Q.plans[0]
        assert type(plan).__name__ == 'HMMPlan'
        if 'fused' in legs:
            emit(dict(leg='fused', what='Q.update()',
                      **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
            emit(dict(leg='fused_bound', L=float(Q.L[Q.iter - 1])))
        else:
            Q.update(verbose=False)
        if 'pass' in legs:
            r = timed(lambda: plan._run_pass(refresh=False), a.steps, a.warmup)
            steps_total = float(B) * T
            s = 1e-3 * r['ms_median']
            emit(dict(leg='pass', what='vmp_hmm_fused_pass', bytes_per_chain_step=16 * D + 16 * K,
                      GB_per_s=steps_total * (16 * D + 16 * K) / s / 1e9,
                      exp_per_chain_step=(3 * K + 2) * K,
                      Gexp_per_s=steps_total * (3 * K + 2) * K / s / 1e9, **r))
        rs = np.random.RandomState(1)
        for name, frac in masks:
            if frac is None:
                m = np.arange(T)[None, :] < rs.randint(1, T + 1, size=B)[:, None]
            else:
                m = rs.rand(B, T) < frac
            plan.Y.observe(np.where(m[..., None], y, np.nan), mask=m)
            assert plan.Y._plan is plan and plan.has_state()     # the posteriors stay
            plan._materialize()
            assert plan.maskd is not None
            r = timed(lambda: plan._run_pass(refresh=False), a.steps, a.warmup)
            emit(dict(leg='pass_masked', what='vmp_hmm_fused_pass_masked', mask=name,
                      observed_fraction=float(m.mean()),
                      chains_without_observation=int((~m.any(axis=1)).sum()), **r))
        del Q, plan
        torch.cuda.empty_cache()
    if 'generic' in legs:
        try:
            Q = build(y, mu, z0, 'generic')
            emit(dict(leg='generic', what='Q.update()',
                      **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
            emit(dict(leg='generic_bound', L=float(Q.L[Q.iter - 1]),
                      peak_GB=torch.cuda.max_memory_allocated() / 1e9))
        except (RuntimeError, MemoryError) as exc:         # out of memory at this size
            emit(dict(leg='generic', error=str(exc)[:200]))
    if a.out:
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
