"""Gaussian hidden Markov model on a batch of sequences of DIFFERENT lengths with learned emission
parameters: the sequences are padded with NaN to the longest one and the padding is masked,
``Y.observe(y, mask=m)``.  A masked step sends no message to the chain and its ``y`` is never
read; with engine='fused' the chain pass reads one byte of the mask per chain and step.

    python examples/hmm_ragged.py [--chains 2000] [--steps 200] [--iters 20]
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
    """(y padded with NaN (B, T, 2), mask (B, T), lengths (B,)): lengths uniform in 1 ... T."""
    mu = np.array([[0.0, 0.0], [3.0, 4.0], [6.0, 0.0]])
    A = np.array([[0.9, 0.05, 0.05], [0.1, 0.8, 0.1], [0.05, 0.05, 0.9]])
    z = np.empty((B, T), dtype=np.int64)
    z[:, 0] = rs.randint(3, size=B)
    cum = A.cumsum(axis=1)
    for t in range(1, T):
        z[:, t] = (rs.rand(B)[:, None] > cum[z[:, t - 1]]).sum(axis=1)
    y = mu[z] + rs.normal(size=(B, T, 2))
    lengths = rs.randint(1, T + 1, size=B)
    mask = np.arange(T)[None, :] < lengths[:, None]
    return np.where(mask[..., None], y, np.nan), mask, lengths


def build(y, mask, K=3, engine='fused'):
    B, T, D = y.shape
    a0 = Dirichlet(1e-3 * np.ones(K), name='a0')
    A = Dirichlet(1e-3 * np.ones((K, K)), name='A')
    Z = CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    mu = GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
    Lambda = Wishart(D, np.identity(D), plates=(K,), name='Lambda')
    Y = Mixture(Z, Gaussian, mu, Lambda, name='Y')
    Y.observe(y, mask=mask)
    # a crude start: states from the first coordinate's terciles (anything at the padding)
    cut = np.quantile(y[..., 0][mask], np.arange(1, K) / K)
    Z.initialize_from_value((np.nan_to_num(y[..., 0])[..., None] > cut).sum(-1))
    Q = VB(Y, mu, Lambda, A, a0, Z, engine=engine)
    return Q, dict(a0=a0, A=A, Z=Z, mu=mu, Lambda=Lambda, Y=Y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--chains', type=int, default=2000)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--iters', type=int, default=20)
    a = ap.parse_args()
    y, mask, lengths = simulate(a.chains, a.steps, np.random.RandomState(1))
    print('%d sequences, lengths %d ... %d, %.0f %% of the padded array observed'
          % (a.chains, lengths.min(), lengths.max(), 100 * mask.mean()))
    Q, n = build(y, mask)
    Q.update(repeat=a.iters)
    m = n['mu'].get_moments()[0]
    order = np.argsort(m[:, 0])
    print('state means (sorted by the first coordinate):')
    print(np.round(m[order], 3))
    print('transition probabilities:')
    P = np.exp(n['A'].get_moments()[0])[order][:, order]
    print(np.round(P / P.sum(-1, keepdims=True), 3))


if __name__ == '__main__':
    main()
