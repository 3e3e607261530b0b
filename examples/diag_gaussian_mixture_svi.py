#!/usr/bin/env python
"""
Stochastic variational inference for a Gaussian mixture with one precision per dimension on the
fused block: the loop of bayespy/demos/stochastic_inference.py:93-133, the mini-batches drawn from a
host array that need not fit the device.

    python examples/diag_gaussian_mixture_svi.py [--n 200000] [--batch 4096] [--steps 100]

Every step observes a mini-batch, updates the responsibilities -- one pass of the block over the
batch -- and moves the means, the precisions and the class probabilities along their natural
gradients in one launch (``VB.gradient_step``).  ``--missing 0.2`` hides that share of the entries
of every batch (a mask of the full shape: the block for missing observations).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=200000)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--missing', type=float, default=0.0)
    ap.add_argument('--seed', type=int, default=42)
    a = ap.parse_args()
    from bayespy_amd.nodes import GaussianARD, Gamma, Dirichlet, Categorical, Mixture
    from bayespy_amd.inference import VB

    rs = np.random.RandomState(a.seed)
    N, NB, D, K, K_true = a.n, a.batch, 64, 12, 6
    centres = 3.0 * rs.randn(K_true, D)
    data = centres[rs.randint(K_true, size=N)] + rs.randn(N, D)

    def observe(Y):
        rows = data[rs.choice(N, NB)]
        if a.missing > 0:
            Y.observe(rows, mask=rs.rand(NB, D) >= a.missing)
        else:
            Y.observe(rows)

    alpha = Dirichlet(np.ones(K), name='class probabilities')
    Z = Categorical(alpha, plates=(NB, 1), plates_multiplier=(N / NB, 1), name='classes')
    mu = GaussianARD(0, 1e-2, plates=(D, K), name='means')
    tau = Gamma(1.0, 1.0, plates=(D, K), name='precisions')
    Y = Mixture(Z, GaussianARD, mu, tau, name='observations')
    mu.initialize_from_value(3.0 * rs.randn(D, K))

    observe(Y)
    Q = VB(Y, Z, mu, tau, alpha, engine='fused+batches+gaussian')
    Q.ignore_bound_checks = True
    for n in range(a.steps):
        if n:
            observe(Y)
        Q.update(Z, verbose=False)
        Q.gradient_step(mu, tau, alpha, scale=(n + 2) ** (-0.7))
        if n % 20 == 0 or n == a.steps - 1:
            print('step %4d  bound %.6e' % (n, Q.compute_lowerbound()))
    w = alpha.get_moments()[0]
    print('plan: %s; clusters with weight > 1%%: %d (true: %d)'
          % (type(Q.plans[0]).__name__, int(np.sum(np.exp(w) > 0.01)), K_true))


if __name__ == '__main__':
    main()
