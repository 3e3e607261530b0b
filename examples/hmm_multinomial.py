#!/usr/bin/env python
"""
A hidden Markov model whose every time step carries a vector of counts: B sequences of intervals,
each with the counts of M event types among n events, K hidden regimes, with a0, A and P learned
from their Dirichlet priors.  ``engine='fused+counts'`` adds the multinomial-emission form of the
discrete HMM block (inference/plans/hmm_mult.py): the emission table and
the count statistics are two matrix-core products over the whole (b, t) plate.

    python examples/hmm_multinomial.py [--chains 8] [--steps 200] [--types 30] [--states 4]
"""
import argparse
import itertools
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def simulate(B, T, M, K, n, rs):
    """Sticky regimes, each with its own distribution over the event types."""
    P = rs.dirichlet(0.3 * np.ones(M), size=K)
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(K, size=B)
    for t in range(1, T):
        z[:, t] = np.where(rs.rand(B) < 0.95, z[:, t - 1], rs.randint(K, size=B))
    x = np.array([rs.multinomial(n, P[k]) for k in z.reshape(-1)]).reshape(B, T, M)
    return x, z


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=8)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--types', type=int, default=30)
    ap.add_argument('--states', type=int, default=4)
    ap.add_argument('--events', type=int, default=40)
    ap.add_argument('--sweeps', type=int, default=20)
    a = ap.parse_args()
    from bayespy_amd.nodes import CategoricalMarkovChain, Dirichlet, Mixture, Multinomial
    from bayespy_amd.inference import VB
    B, T, M, K, n = a.chains, a.steps, a.types, a.states, a.events
    rs = np.random.RandomState(1)
    x, z = simulate(B, T, M, K, n, rs)
    a0 = Dirichlet(np.ones(K), name='a0')
    A = Dirichlet(np.ones((K, K)) + 5 * np.identity(K), name='A')
    P = Dirichlet(0.5 + rs.gamma(1.0, size=(K, M)), name='P')       # asymmetric: tells states apart
    Z = CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    Y = Mixture(Z, Multinomial, n, P, name='Y')
    Y.observe(x)
    Q = VB(Y, Z, P, A, a0, engine='fused+counts')
    print(type(Q.plans[0]).__name__)
    t0 = time.perf_counter()
    Q.update(repeat=a.sweeps, verbose=False)
    print('%d sweeps over %d count vectors: %.1f ms, set-up included; bound %.2f -> %.2f'
          % (Q.iter, B * T, 1e3 * (time.perf_counter() - t0), Q.L[0], Q.L[Q.iter - 1]))
    est = Q.plans[0].posterior(pairs=False)[0].cpu().numpy().argmax(-1)
    agree = max(np.mean(np.array(perm)[est] == z) for perm in itertools.permutations(range(K))) \
        if K <= 6 else float('nan')
    print('state sequence agreement (best relabelling): %.3f' % agree)


if __name__ == '__main__':
    main()
