"""Count clustering: a mixture of Poisson columns.  N rows of D counts (events per hour, words per
document, reads per gene) that fall into K groups with their own rates:

    R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
    lam = Gamma(a0, b0, plates=(D, K));  X = Mixture(Z, Poisson, lam);  X.observe(x)

``engine='fused'`` runs it on the fused Poisson-mixture block: ``x`` is kept as 16 bits per count
and neither the (N, D, K) log-density nor the (N, D, K) messages to ``lam`` are formed.  With
``missing=True`` three in ten counts are held back (``X.observe(x, mask=m)`` with a mask of the full
shape).  The clusters found are compared with the ones the data were drawn from.

    python examples/poisson_mixture.py [rows] [missing]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd import nodes                                                          # noqa: E402
from bayespy_amd.inference import VB                                                   # noqa: E402


def run(N=10 ** 5, D=64, K=8, sweeps=20, missing=False, hidden=0.3, verbose=True):
    rs = np.random.RandomState(0)
    rates = rs.gamma(2.0, 3.0, size=(K, D))
    z = rs.randint(K, size=N)
    x = rs.poisson(rates[z]).astype(np.int64)
    R = nodes.Dirichlet(K * [1.0], name='R')
    Z = nodes.Categorical(R, plates=(N, 1), name='Z')
    lam = nodes.Gamma(1e-2, 1e-2, plates=(D, K), name='lam')
    X = nodes.Mixture(Z, nodes.Poisson, lam, name='X')
    if missing:
        mask = rs.random_sample((N, D)) >= hidden
        # what stands at a hidden position is never read by the block; observe() itself checks
        # every value, so the holes are filled with zeros
        X.observe(np.where(mask, x, 0), mask=mask)
    else:
        X.observe(x)
    # start from the rates of K rows of the data
    lam.initialize_from_value(x[rs.choice(N, K, replace=False)].T + 0.5)

    Q = VB(Z, R, X, lam, engine='fused')
    plan = type(Q.plans[0]).__name__
    if verbose:
        print('plan:', plan)
    Q.update(repeat=sweeps, verbose=verbose)

    # rows of one true cluster that share their most probable cluster
    found = Z.get_moments()[0][:, 0, :].argmax(axis=-1)
    acc = float(np.mean([np.bincount(found[z == k], minlength=K).max() / max(np.sum(z == k), 1)
                         for k in range(K)]))
    if verbose:
        print('rows of a true cluster that were put together: %.1f %%' % (100 * acc))
    return dict(plan=plan, L=np.array(Q.L[:Q.iter]), accuracy=acc)


if __name__ == '__main__':
    run(N=int(sys.argv[1]) if len(sys.argv) > 1 else 10 ** 5,
        missing=len(sys.argv) > 2 and sys.argv[2] == 'missing')
