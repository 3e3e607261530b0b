#!/usr/bin/env python
"""
A full-covariance Gaussian mixture over 40-dimensional features: N = 2e5 points from K = 8
clusters.  ``engine='fused+dims'`` adds the high-dimensional form of the Gaussian-mixture block
(inference/plans/gmm_hd.py) for 33 <= D <= 64; the block itself stops at
D = 32 and the generic engine keeps (N, K, D, D) intermediates, 12.8 KB per point and cluster here.

    python examples/gmm_high_dim.py [--points 200000] [--dims 40] [--clusters 8] [--sweeps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', type=int, default=200000)
    ap.add_argument('--dims', type=int, default=40)
    ap.add_argument('--clusters', type=int, default=8)
    ap.add_argument('--sweeps', type=int, default=20)
    a = ap.parse_args()
    from bayespy_amd.nodes import Categorical, Dirichlet, Gaussian, GaussianARD, Mixture, Wishart
    from bayespy_amd.inference import VB
    N, D, K = a.points, a.dims, a.clusters
    rs = np.random.RandomState(1)
    centre = 3.0 * rs.normal(size=(K, D)) / np.sqrt(D)
    mix = rs.normal(size=(K, D, D)) / np.sqrt(D) + np.identity(D)
    lab = rs.randint(K, size=N)
    y = centre[lab] + np.einsum('nde,ne->nd', mix[lab], rs.normal(size=(N, D)))
    alpha = Dirichlet(np.ones(K), name='alpha')
    z = Categorical(alpha, plates=(N,), name='z')
    mu = GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
    Lam = Wishart(D + 2, np.identity(D), plates=(K,), name='Lambda')
    Y = Mixture(z, Gaussian, mu, Lam, plates=(N,), name='Y')
    z.initialize_from_random()
    Y.observe(y)
    Q = VB(Y, mu, Lam, z, alpha, engine='fused+dims')
    print(type(Q.plans[0]).__name__)
    t0 = time.perf_counter()
    for _ in range(a.sweeps):
        Q.update(verbose=False)
        print('sweep %2d  bound %.4f' % (Q.iter, Q.L[Q.iter - 1]))
    print('%d sweeps over %d points, D = %d, K = %d: %.1f ms, set-up included'
          % (Q.iter, N, D, K, 1e3 * (time.perf_counter() - t0)))


if __name__ == '__main__':
    main()
