"""Gaussian hidden Markov model with 16-dimensional observations (cepstral-like feature vectors) and
learned full-covariance emissions on a batch of sequences.  The HMM block stops at D = 8;
``engine='fused+emissions'`` adds its wide-emission form (9 <= D <= 32): the emission table and
the emission statistics run on the fp64 matrix cores, the chain pass keeps the recursion alone, and
no (B, T-1, K, K) array exists.

    python examples/hmm_wide.py [--chains 500] [--steps 200] [--iters 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd.nodes import (Dirichlet, CategoricalMarkovChain, GaussianARD, Wishart, Mixture,  # noqa: E402
                               Gaussian)
from bayespy_amd.inference import VB                                                   # noqa: E402

D, K = 16, 4


def simulate(B, T, rs):
    mu = 3.0 * rs.normal(size=(K, D))
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(K, size=B)
    for t in range(1, T):                           # sticky chains
        z[:, t] = np.where(rs.rand(B) < 0.9, z[:, t - 1], rs.randint(K, size=B))
    return mu[z] + rs.normal(size=(B, T, D)), z, mu


def build(y, z0, engine='fused+emissions'):
    B, T, _ = y.shape
    a0 = Dirichlet(1e-3 * np.ones(K), name='a0')
    A = Dirichlet(1e-3 * np.ones((K, K)), name='A')
    Z = CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    mu = GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
    Lambda = Wishart(D, np.identity(D), plates=(K,), name='Lambda')
    Y = Mixture(Z, Gaussian, mu, Lambda, name='Y')
    Y.observe(y)
    Z.initialize_from_value(z0)
    Q = VB(Y, mu, Lambda, A, a0, Z, engine=engine)
    return Q, dict(a0=a0, A=A, Z=Z, mu=mu, Lambda=Lambda, Y=Y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=500)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    rs = np.random.RandomState(1)
    y, z, mu = simulate(a.chains, a.steps, rs)
    # a crude start: the true state at a third of the steps, a random one elsewhere
    z0 = np.where(rs.rand(*z.shape) < 1.0 / 3, z, rs.randint(K, size=z.shape))
    Q, n = build(y, z0)
    print(type(Q.plans[0]).__name__)
    Q.update(repeat=a.iters)
    m = n['mu'].get_moments()[0]
    print('largest distance of a true state mean to the nearest learned one: %.3f'
          % np.max(np.min(np.linalg.norm(mu[:, None] - m[None], axis=-1), axis=1)))


if __name__ == '__main__':
    main()
