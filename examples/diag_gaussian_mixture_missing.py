#!/usr/bin/env python
"""
Gaussian mixture with one precision per dimension and missing observations on the fused block

    alpha = Dirichlet(a);  Z = Categorical(alpha, plates=(N, 1))
    mu = GaussianARD(0, 1e-3, plates=(D, K));  tau = Gamma(1e-2, 1e-2, plates=(D, K))
    Y = Mixture(Z, GaussianARD, mu, tau);  Y.observe(y, mask=m)           m (N, D), 30 % hidden

``VB(..., engine='fused')`` runs it on ``MaskedDiagGaussianMixturePlan``: one pass over the rows
per update of ``Z`` leaves N_k, the counts sum r m, sum r y and sum r y^2 over the observed
entries; nothing of size (N, D, K) exists and the mask is not kept beside y.  The hidden entries of
``y`` are NaN here: they reach nothing.

    python examples/diag_gaussian_mixture_missing.py [N] [D] [K]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(N=2000, D=70, K=4, sweeps=10, seed=0, hidden=0.3, verbose=True):
    from bayespy_amd.nodes import Categorical, Dirichlet, GaussianARD, Gamma, Mixture
    from bayespy_amd.inference import VB
    rs = np.random.RandomState(seed)
    centres = 2.0 * rs.normal(size=(K, D))
    scales = rs.gamma(4.0, 0.25, size=(K, D))
    z = rs.randint(K, size=N)
    y = centres[z] + scales[z] * rs.normal(size=(N, D))
    mask = rs.rand(N, D) >= hidden
    y = np.where(mask, y, np.nan)

    alpha = Dirichlet(K * [1.0], name='alpha')
    Z = Categorical(alpha, plates=(N, 1), name='Z')
    mu = GaussianARD(0.0, 1e-3, plates=(D, K), name='mu')
    tau = Gamma(1e-2, 1e-2, plates=(D, K), name='tau')
    Y = Mixture(Z, GaussianARD, mu, tau, name='Y')
    Y.observe(y, mask=mask)
    # break the symmetry: K rows of the data (hidden entries at the mean of their column) as the
    # first means, each the row farthest from the rows chosen before it
    filled = np.where(mask, y, np.nanmean(y, axis=0))
    rows = [int(rs.randint(N))]
    for _ in range(K - 1):
        dist = np.min([((filled - filled[i]) ** 2).sum(axis=1) for i in rows], axis=0)
        rows.append(int(dist.argmax()))
    mu.initialize_from_value(filled[rows].T)
    Q = VB(Y, Z, mu, tau, alpha, engine='fused')
    Q.update(repeat=sweeps, verbose=verbose)            # stops early once the bound stands still
    r = Z.get_moments()[0][:, 0, :]
    found = r.argmax(axis=1)
    # a found cluster counts for the true class most of its rows come from
    hits = sum(np.bincount(z[found == k], minlength=K).max() for k in range(K) if np.any(found == k))
    return dict(plan=type(Q.plans[0]).__name__, L=np.array(Q.L[:Q.iter]), accuracy=hits / N,
                means=mu.get_moments()[0], precisions=tau.get_moments()[0])


if __name__ == '__main__':
    args = [int(a) for a in sys.argv[1:4]]
    out = run(*args)
    print('plan %s, bound %.6g, accuracy %.3f' % (out['plan'], out['L'][-1], out['accuracy']))
