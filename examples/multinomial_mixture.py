"""Count-vector clustering: a mixture of multinomials (mixture of unigrams).  N rows of M counts
that add up to the row's total (words of a document, items of a basket, k-mers of a read) and fall
into K groups with their own word probabilities:

    R = Dirichlet(a);  Z = Categorical(R, plates=(N,))
    P = Dirichlet(a0, plates=(K,));  X = Mixture(Z, Multinomial, n, P);  X.observe(x)

``n`` is the number of trials: one number for all rows, or one per row as an (N, 1) array (beside
the cluster axis of ``P``).  ``engine='fused'`` runs it on the fused multinomial-mixture block:
``x`` is kept as 16 bits per count and neither the (N, K) log-density nor the (N, K, M) message to
``P`` is formed.  The clusters found are compared with the ones the data were drawn from.

    python examples/multinomial_mixture.py [rows]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd import nodes                                                          # noqa: E402
from bayespy_amd.inference import VB                                                   # noqa: E402


def run(N=10 ** 5, M=64, K=8, sweeps=20, verbose=True):
    rs = np.random.RandomState(0)
    p = rs.dirichlet(0.5 * np.ones(M), size=K)
    z = rs.randint(K, size=N)
    n = rs.randint(30, 120, size=N)
    x = np.array([rs.multinomial(n[i], p[z[i]]) for i in range(N)], dtype=np.int64)
    R = nodes.Dirichlet(K * [1.0], name='R')
    Z = nodes.Categorical(R, plates=(N,), name='Z')
    P = nodes.Dirichlet(0.5 * np.ones(M), plates=(K,), name='P')
    X = nodes.Mixture(Z, nodes.Multinomial, n[:, None], P, name='X')
    X.observe(x)
    # start from the word frequencies of K rows of the data
    start = x[rs.choice(N, K, replace=False)] + 0.5
    P.initialize_from_value(start / start.sum(axis=1, keepdims=True))

    Q = VB(Z, R, X, P, engine='fused')
    plan = type(Q.plans[0]).__name__
    if verbose:
        print('plan:', plan)
    Q.update(repeat=sweeps, verbose=verbose)

    # rows of one true cluster that share their most probable cluster
    found = Z.get_moments()[0].argmax(axis=-1)
    acc = float(np.mean([np.bincount(found[z == k], minlength=K).max() / max(np.sum(z == k), 1)
                         for k in range(K)]))
    if verbose:
        print('rows of a true cluster that were put together: %.1f %%' % (100 * acc))
    return dict(plan=plan, L=np.array(Q.L[:Q.iter]), accuracy=acc)


if __name__ == '__main__':
    run(N=int(sys.argv[1]) if len(sys.argv) > 1 else 10 ** 5)
