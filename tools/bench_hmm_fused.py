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

  cat      (--emissions categorical) the same three legs for the discrete block
           (inference/plans/hmm_cat.py): M = 16 words, learned P, Z from fixed random labels; the
           pass is ``vmp_hmm_fused_pass_categorical`` (8 + 16 K bytes per chain step: the int32 word read
           twice, the forward state written and read once; the <log P> rows come from L2).
           Without --out these lines go to profiles/hmm_fused/bench_hmm_cat.json.

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


def make_words(B, T, M, K, seed=0):
    rs = np.random.RandomState(seed)
    P = rs.dirichlet(0.3 * np.ones(M), size=K)
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(K, size=B)
    for t in range(1, T):                           # sticky chains
        z[:, t] = np.where(rs.rand(B) < 0.9, z[:, t - 1], rs.randint(K, size=B))
    u = rs.rand(B, T)
    y = (u[..., None] > np.cumsum(P, axis=1)[z]).sum(-1).clip(0, M - 1)
    return y, rs.randint(K, size=(B, T))


def build_cat(y, z0, K, M, engine):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    B, T = y.shape
    a0 = N_.Dirichlet(1e-3 * np.ones(K), name='a0')
    A = N_.Dirichlet(1e-3 * np.ones((K, K)), name='A')
    P = N_.Dirichlet(np.ones((K, M)), name='P')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    Y = N_.Mixture(Z, N_.Categorical, P, name='Y')
    Y.observe(y)
    Z.initialize_from_value(z0)
    Q = VB(Y, P, A, a0, Z, engine=engine)
    Q.ignore_bound_checks = True
    return Q


def categorical_legs(a, emit):
    import torch
    B, T, K, M = a.B, a.T, a.K, a.M
    y, z0 = make_words(B, T, M, K)
    legs = a.legs.split(',')
    if 'fused' in legs or 'pass' in legs:
        torch.cuda.reset_peak_memory_stats()
        Q = build_cat(y, z0, K, M, 'fused')
        plan = Q.plans[0]
        assert type(plan).__name__ == 'CategoricalHMMPlan'
        if 'fused' in legs:
            emit(dict(leg='fused', what='Q.update()',
                      **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
            emit(dict(leg='fused_bound', L=float(Q.L[Q.iter - 1]),
                      peak_GB=torch.cuda.max_memory_allocated() / 1e9))
        else:
            Q.update(verbose=False)
        if 'pass' in legs:
            r = timed(lambda: plan._run_pass(refresh=False), a.steps, a.warmup)
            steps_total = float(B) * T
            s = 1e-3 * r['ms_median']
            emit(dict(leg='pass', what='vmp_hmm_fused_pass_categorical',
                      bytes_per_chain_step=8 + 16 * K,
                      GB_per_s=steps_total * (8 + 16 * K) / s / 1e9,
                      exp_per_chain_step=(3 * K + 2) * K,
                      Gexp_per_s=steps_total * (3 * K + 2) * K / s / 1e9, **r))
        del Q, plan
        torch.cuda.empty_cache()
    if 'generic' in legs:
        try:
            torch.cuda.reset_peak_memory_stats()
            Q = build_cat(y, z0, K, M, 'generic')
            emit(dict(leg='generic', what='Q.update()',
                      **timed(lambda: Q.update(verbose=False), a.steps, a.warmup)))
            emit(dict(leg='generic_bound', L=float(Q.L[Q.iter - 1]),
                      peak_GB=torch.cuda.max_memory_allocated() / 1e9))
        except (RuntimeError, MemoryError) as exc:         # out of memory at this size
            emit(dict(leg='generic', error=str(exc)[:200]))


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
    ap.add_argument('--emissions', default='gaussian', choices=('gaussian', 'categorical'))
    ap.add_argument('--M', type=int, default=16, help='words of the categorical legs')
    a = ap.parse_args()
    import torch
    B, T, D, K = a.B, a.T, a.D, a.K
    cat = a.emissions == 'categorical'
    shape = dict(B=B, T=T, M=a.M, K=K, emissions='categorical') if cat else dict(B=B, T=T, D=D, K=K)
    lines = []

    def emit(rec):
        rec = dict(shape, **rec)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    if cat:
        if a.out is None:
            a.out = os.path.join(ROOT, 'profiles', 'hmm_fused', 'bench_hmm_cat.json')
        categorical_legs(a, emit)
        with open(a.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
        return
    y, mu, z0 = make_data(B, T, D, K)

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
