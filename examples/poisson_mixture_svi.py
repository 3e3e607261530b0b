#!/usr/bin/env python
"""
Stochastic variational inference for a Poisson mixture (count clustering) on the fused block: the
loop of bayespy/demos/stochastic_inference.py:93-133 on count data, the mini-batches drawn from a
host array.

    python examples/poisson_mixture_svi.py [--n 200000] [--batch 4096] [--steps 100]

Every step observes a mini-batch, updates the responsibilities -- one pack and one pass of the block
over the batch -- and moves the rates and the class probabilities along their natural gradients in
one launch (``VB.gradient_step``).
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
    ap.add_argument('--seed', type=int, default=42)
    a = ap.parse_args()
    from bayespy_amd.nodes import Gamma, Dirichlet, Categorical, Mixture, Poisson
    from bayespy_amd.inference import VB

    rs = np.random.RandomState(a.seed)
    N, NB, D, K, K_true = a.n, a.batch, 32, 12, 6
    rates = rs.gamma(2.0, 4.0, size=(K_true, D))
    data = rs.poisson(rates[rs.randint(K_true, size=N)]).astype(np.int64)

    R = Dirichlet(np.ones(K), name='class probabilities')
    Z = Categorical(R, plates=(NB, 1), plates_multiplier=(N / NB, 1), name='classes')
    lam = Gamma(1.0, 0.1, plates=(D, K), name='rates')
    X = Mixture(Z, Poisson, lam, name='counts')
    lam.initialize_from_value(rs.gamma(2.0, 4.0, size=(D, K)))

    X.observe(data[rs.choice(N, NB)])
    Q = VB(X, Z, lam, R, engine='fused+batches')
    Q.ignore_bound_checks = True
    for n in range(a.steps):
        if n:
            X.observe(data[rs.choice(N, NB)])
        Q.update(Z, verbose=False)
        Q.gradient_step(lam, R, scale=(n + 2) ** (-0.7))
        if n % 20 == 0 or n == a.steps - 1:
            print('step %4d  bound %.6e' % (n, Q.compute_lowerbound()))
    w = R.get_moments()[0]
    print('plan: %s; clusters with weight > 1%%: %d (true: %d)'
          % (type(Q.plans[0]).__name__, int(np.sum(np.exp(w) > 0.01)), K_true))


if __name__ == '__main__':
    main()
