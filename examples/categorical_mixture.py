"""Latent class model: a mixture of categorical columns.  A survey of D multiple-choice items with M
answers each, filled in by N people who fall into K classes:

    R = Dirichlet(a);  Z = Categorical(R, plates=(N, 1))
    P = Dirichlet(conc, plates=(D, K));  X = Mixture(Z, Categorical, P);  X.observe(x)

``engine='fused'`` runs it on the fused categorical-mixture block: ``x`` is kept as one byte per
answer and neither the (N, D, K) log-density nor the (N, D, K, M) message to ``P`` is formed.  With
``missing=True`` three in ten answers are held back (``X.observe(x, mask=m)`` with a mask of the
full shape), predicted from the posterior and compared with what was hidden.

    python examples/categorical_mixture.py [rows] [missing]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd import nodes                                                          # noqa: E402
from bayespy_amd.inference import VB                                                   # noqa: E402


def run(N=10 ** 6, D=32, K=8, M=8, sweeps=20, missing=False, hidden=0.3, verbose=True):
    rs = np.random.RandomState(0)
    p_true = rs.dirichlet(0.2 * np.ones(M), size=(K, D))
    z = rs.randint(K, size=N)
    cum = np.cumsum(p_true, axis=-1)
    x = np.empty((N, D), dtype=np.int64)
    for lo in range(0, N, 1 << 16):                     # (rows, D, M) only for a block of rows
        u = rs.random_sample((min(N, lo + (1 << 16)) - lo, D, 1))
        x[lo:lo + len(u)] = (u > cum[z[lo:lo + len(u)]]).sum(axis=-1).clip(0, M - 1)
    R = nodes.Dirichlet(K * [1.0], name='R')
    Z = nodes.Categorical(R, plates=(N, 1), name='Z')
    P = nodes.Dirichlet(M * [0.5], plates=(D, K), name='P')
    X = nodes.Mixture(Z, nodes.Categorical, P, name='X')
    if missing:
        mask = rs.random_sample((N, D)) >= hidden
        # what stands at a hidden position is never read by the block; observe() itself checks
        # every value, so the holes are filled with zeros
        X.observe(np.where(mask, x, 0), mask=mask)
    else:
        mask = np.ones((N, D), dtype=bool)
        X.observe(x)
    P.initialize_from_value(rs.dirichlet(5.0 * np.ones(M), size=(D, K)))

    Q = VB(Z, R, X, P, engine='fused')
    plan = type(Q.plans[0]).__name__
    if verbose:
        print('plan:', plan)
    Q.update(repeat=sweeps, verbose=verbose)

    # the most probable answer under sum_k r_nk p_dk[m], with p from the <log> moments of P
    p = np.exp(P.get_moments()[0])
    p /= p.sum(axis=-1, keepdims=True)
    guess = np.einsum('nk,dkm->ndm', Z.get_moments()[0][:, 0, :], p).argmax(axis=-1)
    where = ~mask if missing else mask
    acc = float(np.mean(guess[where] == x[where]))
    if verbose:
        print('%s answers predicted correctly: %.1f %%'
              % ('hidden' if missing else 'observed', 100 * acc))
    return dict(plan=plan, L=np.array(Q.L[:Q.iter]), accuracy=acc)


if __name__ == '__main__':
    run(N=int(sys.argv[1]) if len(sys.argv) > 1 else 10 ** 5,
        missing=len(sys.argv) > 2 and sys.argv[2] == 'missing')
