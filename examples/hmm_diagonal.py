#!/usr/bin/env python
"""
A hidden Markov model over feature vectors with one precision per dimension: B sequences of
39-dimensional frames (the usual speech features), K hidden regimes, with a0, A, the state means
and the per-dimension precisions learned from their priors.  ``engine='fused+diagonal'`` adds the
diagonal-Gaussian-emission form of the HMM block (inference/plans/hmm_diag.py, DESIGN.md section
4.15g): the emission table and the statistics are matrix-core products over the whole (b, t)
plate, for up to 1024 dimensions.

    python examples/hmm_diagonal.py [--chains 8] [--steps 200] [--dims 39] [--states 4]
"""
import argparse
import itertools
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def simulate(B, T, D, K, rs):
    """Sticky regimes, each with its own mean and its own noise level per dimension."""
    means, sd = 2.0 * rs.randn(K, D), 0.5 + rs.rand(K, D)
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(K, size=B)
    for t in range(1, T):
        z[:, t] = np.where(rs.rand(B) < 0.95, z[:, t - 1], rs.randint(K, size=B))
    return means[z] + sd[z] * rs.randn(B, T, D), z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=8)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--dims', type=int, default=39)
    ap.add_argument('--states', type=int, default=4)
    ap.add_argument('--sweeps', type=int, default=20)
    a = ap.parse_args()
    from bayespy_amd.nodes import (CategoricalMarkovChain, Dirichlet, Gamma, GaussianARD, Mixture)
    from bayespy_amd.inference import VB
    B, T, D, K = a.chains, a.steps, a.dims, a.states
    rs = np.random.RandomState(1)
    y, z = simulate(B, T, D, K, rs)
    a0 = Dirichlet(np.ones(K), name='a0')
    A = Dirichlet(np.ones((K, K)) + 5 * np.identity(K), name='A')
    # prior means drawn from the data: tells the states apart from the first sweep on
    mu = GaussianARD(y.reshape(-1, D)[rs.choice(B * T, K, replace=False)], 1e-2, shape=(D,),
                     plates=(K,), name='mu')
    tau = Gamma(1e-3, 1e-3, plates=(K, D), name='tau')
    Z = CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    Y = Mixture(Z, GaussianARD, mu, tau, 1, name='Y')
    Y.observe(y)
    Q = VB(Y, Z, mu, tau, A, a0, engine='fused+diagonal')
    print(type(Q.plans[0]).__name__)
    t0 = time.perf_counter()
    Q.update(repeat=a.sweeps, verbose=False)
    print('%d sweeps over %d frames of %d dimensions: %.1f ms, set-up included; bound %.2f -> %.2f'
          % (Q.iter, B * T, D, 1e3 * (time.perf_counter() - t0), Q.L[0], Q.L[Q.iter - 1]))
    est = Q.plans[0].posterior(pairs=False)[0].cpu().numpy().argmax(-1)
    agree = max(np.mean(np.array(perm)[est] == z) for perm in itertools.permutations(range(K))) \
        if K <= 6 else float('nan')
    print('state sequence agreement (best relabelling): %.3f' % agree)


if __name__ == '__main__':
    main()
