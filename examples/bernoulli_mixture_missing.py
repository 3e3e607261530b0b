"""Bernoulli mixture (doc/source/examples/bmm.rst) on a table with holes: a survey of D yes / no
items answered by N people, of which three in ten answers are missing.  ``X.observe(x, mask=m)``
with a mask of the full shape (N, D) keeps the model on the fused block (``engine='fused'``): the
observations and the mask are two bit planes, N D / 4 bytes, and no (N, D, K) array is formed.
The hidden answers are then predicted from the posterior and compared with what was held back.

    python examples/bernoulli_mixture_missing.py [rows]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd import nodes                                                          # noqa: E402
from bayespy_amd.inference import VB                                                   # noqa: E402


def run(N=10 ** 6, D=64, K=8, sweeps=20, hidden=0.3, verbose=True):
    rs = np.random.RandomState(0)
    p_true = rs.beta(0.3, 0.3, size=(K, D))
    x = rs.random_sample((N, D)) < p_true[rs.randint(K, size=N)]
    mask = rs.random_sample((N, D)) >= hidden
    # what stands at a hidden position is never read by the block; observe() itself checks every
    # value, so the holes are filled with zeros
    R = nodes.Dirichlet(K * [1.0], name='R')
    Z = nodes.Categorical(R, plates=(N, 1), name='Z')
    P = nodes.Beta([0.5, 0.5], plates=(D, K), name='P')
    X = nodes.Mixture(Z, nodes.Bernoulli, P, name='X')
    X.observe(x & mask, mask=mask)
    P.initialize_from_value(rs.beta(2.0, 2.0, size=(D, K)))

    Q = VB(Z, R, X, P, engine='fused')
    plan = type(Q.plans[0]).__name__
    if verbose:
        print('plan:', plan)
    Q.update(repeat=sweeps, verbose=verbose)

    # E[x_nd] = sum_k r_nk p_dk with p from the <log> moments of P
    e = P.get_moments()[0]
    p = np.exp(e[..., 0]) / (np.exp(e[..., 0]) + np.exp(e[..., 1]))
    guess = Z.get_moments()[0][:, 0, :] @ p.T > 0.5
    acc = float(np.mean(guess[~mask] == x[~mask]))
    if verbose:
        print('rows with no answer at all:', int(np.sum(~Z.mask)))
        print('hidden answers predicted correctly: %.1f %%' % (100 * acc))
    return dict(plan=plan, L=np.array(Q.L[:Q.iter]), held_out_accuracy=acc)


if __name__ == '__main__':
    run(N=int(sys.argv[1]) if len(sys.argv) > 1 else 10 ** 6)
