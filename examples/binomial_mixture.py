"""Successes out of trials: a mixture of binomial columns.  N rows of D counts x_nd out of n_nd
trials (methylated reads of the reads that cover a site, clicks of impressions, correct items of
the items attempted) that fall into K groups with their own success probabilities:

    R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
    P = Beta(a0, plates=(D, K));  X = Mixture(Z, Binomial, n, P);  X.observe(x)

``n`` is a constant with a singleton cluster axis: here one number of trials per entry, (N, D, 1).
``engine='fused'`` runs it on the fused binomial-mixture block: counts and trials are kept as 16
bits each and neither the (N, D, K) log-density nor the (N, D, K, 2) messages to ``P`` are formed.
With ``missing=True`` three in ten entries are held back (``X.observe(x, mask=m)`` with a mask of
the full shape).  The clusters found are compared with the ones the data were drawn from.

    python examples/binomial_mixture.py [rows] [missing]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd import nodes                                                          # noqa: E402
from bayespy_amd.inference import VB                                                   # noqa: E402


def run(N=10 ** 5, D=64, K=8, sweeps=20, missing=False, hidden=0.3, verbose=True):
    rs = np.random.RandomState(0)
    p = rs.beta(1.0, 1.0, size=(K, D))
    z = rs.randint(K, size=N)
    n = rs.poisson(15.0, size=(N, D, 1))            # the exposure of every entry; zeros occur
    x = rs.binomial(n[..., 0], p[z]).astype(np.int64)
    R = nodes.Dirichlet(K * [1.0], name='R')
    Z = nodes.Categorical(R, plates=(N, 1), name='Z')
    P = nodes.Beta([0.5, 0.5], plates=(D, K), name='P')
    X = nodes.Mixture(Z, nodes.Binomial, n, P, name='X')
    if missing:
        mask = rs.random_sample((N, D)) >= hidden
        # what stands at a hidden position is never read by the block; observe() itself checks
        # every value, so the holes are filled with zeros
        X.observe(np.where(mask, x, 0), mask=mask)
    else:
        X.observe(x)
    # start from the success rates of K rows of the data
    rows = rs.choice(N, K, replace=False)
    P.initialize_from_value(((x[rows] + 0.5) / (n[rows, :, 0] + 1.0)).T)

    Q = VB(Z, R, X, P, engine='fused')
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
