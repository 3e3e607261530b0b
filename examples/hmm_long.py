"""Gaussian hidden Markov model on ONE long sequence (T = 2e5: some hours of 10 Hz sensor data) with
learned full-covariance emissions: the model hmm.rst writes.  The chain passes of the HMM block walk
a sequence step by step on one lane group; ``engine='fused+chains'`` puts the long-chain form in
the block's place, which cuts the sequence into segments and runs the recursion inside all of them
at once.

    python examples/hmm_long.py [--steps 200000] [--iters 10] [--seg-len 0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd.nodes import (Dirichlet, CategoricalMarkovChain, GaussianARD, Wishart, Mixture,  # noqa: E402
                               Gaussian)
from bayespy_amd.inference import VB                                                   # noqa: E402

D, K = 4, 5


def simulate(T, rs):
    mu = 4.0 * rs.normal(size=(K, D))
    stay = rs.rand(T) < 0.98                        # a sticky chain
    jump = rs.randint(K, size=T)
    z = np.empty(T, dtype=np.int64)
    z[0] = jump[0]
    for t in range(1, T):
        z[t] = z[t - 1] if stay[t] else jump[t]
    return mu[z] + rs.normal(size=(T, D)), z, mu


def build(y, z0, engine='fused+chains', seg_len=0):
    T = y.shape[0]
    a0 = Dirichlet(1e-3 * np.ones(K), name='a0')
    A = Dirichlet(1e-3 * np.ones((K, K)), name='A')
    Z = CategoricalMarkovChain(a0, A, states=T, name='Z')
    mu = GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
    Lambda = Wishart(D, np.identity(D), plates=(K,), name='Lambda')
    Y = Mixture(Z, Gaussian, mu, Lambda, name='Y')
    Y.observe(y)
    Z.initialize_from_value(z0)
    Q = VB(Y, mu, Lambda, A, a0, Z, engine=engine)
    if seg_len:
        Q.plans[0].seg_len = seg_len                # transitions of a segment; 0: the library's choice
    return Q, dict(a0=a0, A=A, Z=Z, mu=mu, Lambda=Lambda, Y=Y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=200000)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--seg-len', type=int, default=0)
    a = ap.parse_args()
    rs = np.random.RandomState(1)
    y, z, mu = simulate(a.steps, rs)
    # a crude start: the true state at a third of the steps, a random one elsewhere
    z0 = np.where(rs.rand(*z.shape) < 1.0 / 3, z, rs.randint(K, size=z.shape))
    Q, n = build(y, z0, seg_len=a.seg_len)
    print(type(Q.plans[0]).__name__)
    Q.update(repeat=a.iters)
    print('segment length in use: %d' % Q.plans[0].chains_per_wg)
    m = n['mu'].get_moments()[0]
    print('largest distance of a true state mean to the nearest learned one: %.3f'
          % np.max(np.min(np.linalg.norm(mu[:, None] - m[None], axis=-1), axis=1)))


if __name__ == '__main__':
    main()
