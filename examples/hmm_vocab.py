#!/usr/bin/env python
"""
A discrete hidden Markov model over a vocabulary of thousands of words: B sequences of event codes,
K = 16 hidden regimes, M = 5000 codes, with a0, A and P learned from their Dirichlet priors.  The
discrete HMM block stops at 128 words; ``engine='fused+words'`` adds its large-vocabulary form
(inference/plans/hmm_vocab.py), whose count table is a segmented sum over
a word-sorted layout of the observed steps.  Sequences have ragged lengths (a trailing mask).

    python examples/hmm_vocab.py [--chains 256] [--steps 500] [--words 5000] [--states 16]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def simulate(B, T, M, K, rs):
    """Sticky regimes, each with its own sparse distribution over the codes."""
    P = rs.dirichlet(0.05 * np.ones(M), size=K)
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(K, size=B)
    for t in range(1, T):
        z[:, t] = np.where(rs.rand(B) < 0.95, z[:, t - 1], rs.randint(K, size=B))
    u, y = rs.rand(B, T), np.empty((B, T), dtype=np.int64)
    for k in range(K):
        y[z == k] = np.searchsorted(np.cumsum(P[k]), u[z == k]).clip(0, M - 1)
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=256)
    ap.add_argument('--steps', type=int, default=500)
    ap.add_argument('--words', type=int, default=5000)
    ap.add_argument('--states', type=int, default=16)
    ap.add_argument('--sweeps', type=int, default=20)
    a = ap.parse_args()
    from bayespy_amd.nodes import CategoricalMarkovChain, Categorical, Dirichlet, Mixture
    from bayespy_amd.inference import VB
    B, T, M, K = a.chains, a.steps, a.words, a.states
    rs = np.random.RandomState(1)
    y = simulate(B, T, M, K, rs)
    mask = np.arange(T)[None, :] < rs.randint(T // 2, T + 1, size=B)[:, None]
    a0 = Dirichlet(np.ones(K), name='a0')
    A = Dirichlet(np.ones((K, K)) + 5 * np.identity(K), name='A')
    P = Dirichlet(0.5 + rs.gamma(1.0, size=(K, M)), name='P')       # asymmetric: tells states apart
    Z = CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    Y = Mixture(Z, Categorical, P, name='Y')
    Y.observe(np.where(mask, y, -1), mask=mask)     # what stands at a masked step is never used
    Q = VB(Y, Z, P, A, a0, engine='fused+words')
    print(type(Q.plans[0]).__name__)
    t0 = time.perf_counter()
    Q.update(repeat=a.sweeps, verbose=False)
    print('%d sweeps over %d observed codes: %.1f ms, set-up included; bound %.2f -> %.2f'
          % (Q.iter, mask.sum(), 1e3 * (time.perf_counter() - t0), Q.L[0], Q.L[Q.iter - 1]))


if __name__ == '__main__':
    main()
