#!/usr/bin/env python
"""
Stochastic variational inference for a Gaussian mixture on the fused block: the loop of
bayespy/demos/stochastic_inference.py:93-133 with the data kept on the host and the mini-batches
streamed to the device.

    python examples/gmm_svi.py [--n 100000] [--batch 4096] [--steps 200]

Every step observes a mini-batch (a device tensor, used in place), updates the responsibilities --
one pass of the block over the batch -- and moves the means and the class probabilities along their
natural gradients in one launch (``VB.gradient_step``).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=100000)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--seed', type=int, default=42)
    a = ap.parse_args()
    from bayespy_amd.nodes import Gaussian, Dirichlet, Categorical, Mixture
    from bayespy_amd.inference import VB
    from bayespy_amd.utils.streaming import HostBatchStream

    rs = np.random.RandomState(a.seed)
    np.random.seed(a.seed)
    N, NB, D, K, K_true = a.n, a.batch, 5, 20, 10
    means = 5.0 * rs.randn(K_true, D)
    data = means[rs.randint(K_true, size=N)] + rs.randn(N, D)

    mu = Gaussian(np.zeros(D), np.identity(D), plates=(K,), name='means')
    alpha = Dirichlet(np.ones(K), name='class probabilities')
    Z = Categorical(alpha, plates=(NB,), plates_multiplier=(N / NB,), name='classes')
    Y = Mixture(Z, Gaussian, mu, np.identity(D), name='observations')
    mu.initialize_from_random()

    Q = VB(Y, Z, mu, alpha, engine='fused')
    Q.ignore_bound_checks = True
    batches = (rs.choice(N, NB) for _ in range(a.steps))
    for n, (y_dev, _) in enumerate(HostBatchStream(data, batches)):
        Y.observe(y_dev)
        Q.update(Z, verbose=False)
        Q.gradient_step(mu, alpha, scale=(n + 1) ** (-0.7))
        if n % 20 == 0 or n == a.steps - 1:
            print('step %4d  bound %.6e' % (n, Q.compute_lowerbound()))
    w = alpha.u[0]
    print('plan: %s; clusters with weight > 1%%: %d (true: %d)'
          % (type(Q.plans[0]).__name__, int(np.sum(np.exp(w) > 0.01)), K_true))


if __name__ == '__main__':
    main()
