"""Gaussian hidden Markov model (doc/source/examples/hmm.rst, second half) on a batch of chains
with LEARNED emission parameters: a few thousand simulated chains share the initial-state and
transition probabilities, the state means and the state precisions.  With engine='fused' the
chain pass keeps K doubles per step; the generic engine would hold two (B, T-1, K, K) arrays.

    python examples/hmm_batched.py [--chains 4000] [--steps 200] [--iters 20]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd.nodes import (Dirichlet, CategoricalMarkovChain, GaussianARD, Wishart, Mixture,  # noqa: E402
                               Gaussian)
from bayespy_amd.inference import VB                                                   # noqa: E402


def simulate(B, T, rs):
    mu = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 0.0]])
    A = np.array([[0.9, 0.05, 0.05], [0.1, 0.8, 0.1], [0.05, 0.05, 0.9]])
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(3, size=B)
    cum = A.cumsum(axis=1)
    for t in range(1, T):
        z[:, t] = (rs.rand(B)[:, None] > cum[z[:, t - 1]]).sum(axis=1)
    return mu[z] + rs.normal(size=(B, T, 2)), z, mu, A


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=4000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    rs = np.random.RandomState(1)
    B, T, K, D = a.chains, a.steps, 3, 2
    y, z_true, mu_true, A_true = simulate(B, T, rs)

    a0 = Dirichlet(1e-3 * np.ones(K), name='a0')
    A = Dirichlet(1e-3 * np.ones((K, K)), name='A')
    Z = CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    mu = GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
    Lambda = Wishart(D, np.identity(D), plates=(K,), name='Lambda')
    Y = Mixture(Z, Gaussian, mu, Lambda, name='Y')
    Y.observe(y)
    # a crude start: states from the first coordinate's terciles
    cut = np.quantile(y[..., 0], [1 / 3, 2 / 3])
    Z.initialize_from_value((y[..., 0][..., None] > cut).sum(-1))

    Q = VB(Y, mu, Lambda, A, a0, Z, engine='fused')
    Q.update(repeat=a.iters)
    m = mu.get_moments()[0]
    order = np.argsort(m[:, 0])
    print('state means (sorted by the first coordinate):')
    print(np.round(m[order], 3))
    print('transition probabilities:')
    P = np.exp(A.get_moments()[0])[order][:, order]
    print(np.round(P / P.sum(-1, keepdims=True), 3))


if __name__ == '__main__':
    main()
