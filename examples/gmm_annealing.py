#!/usr/bin/env python
"""Deterministic annealing of a Gaussian mixture -- bayespy/demos/annealing.py of the reference on
the fused Gaussian-mixture block of ``bayespy_amd``.

Two well-separated clusters that hold 30 % and 70 % of the data, a prior on the weights that says
so, and the labels the wrong way round at the start, which drives the means towards the optimum
with the clusters swapped.  The script prints the means and the lower bound of plain VB-EM and of
the schedule 0.01, x 1.2 up to 1 (``VB.set_annealing``): at small coefficients the two clusters
merge, near 0.2 they split again.  Both runs stay on the fused block (``GMMPlan``); nothing goes
through the generic engine.  On this model BOTH RUNS REACH THE SAME BOUND: unlike the reference's
demo it learns its weights and precisions, the schedule splits the merged clusters the swapped way
round by itself, and ends in the optimum plain VB-EM stays in.  The script shows how a schedule is
driven on the fused block, not an escape from a poor optimum."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayespy_amd.nodes import (Dirichlet, Categorical, Gaussian, GaussianARD, Wishart,   # noqa: E402
                               Mixture)
from bayespy_amd.inference import VB                                                     # noqa: E402

N, MAXITER = 500, 100
rs = np.random.RandomState(42)
z = (rs.rand(N) < 0.7).astype(int)
y = np.array([4.0, -4.0])[z][:, None] + 0.5 * rs.randn(N, 1)


def model():
    alpha = Dirichlet(N * np.array([0.3, 0.7]), name='alpha')
    Z = Categorical(alpha, plates=(N,), name='z')
    mu = GaussianARD(0, 1e-2, shape=(1,), plates=(2,), name='mu')
    Lambda = Wishart(4 * N, 4 * N * np.identity(1), plates=(2,), name='Lambda')
    Y = Mixture(Z, Gaussian, mu, Lambda, name='Y')
    # the inferior optimum: the clusters swapped
    Z.initialize_from_value(1 - z)
    Y.observe(y)
    return VB(Y, mu, Lambda, Z, alpha), mu


Q, mu = model()
print('engine:', type(Q.plans[0]).__name__)
Q.update(repeat=MAXITER, verbose=False)
print('VB-EM           means %s  lower bound %.4f' % (mu.u[0].ravel(), Q.compute_lowerbound()))

Q, mu = model()
beta = 0.01
while beta < 1.0:
    beta = min(beta * 1.2, 1.0)
    Q.set_annealing(beta)
    Q.update(repeat=MAXITER, tol=1e-4, verbose=False)
print('annealed VB-EM  means %s  lower bound %.4f' % (mu.u[0].ravel(), Q.compute_lowerbound()))
print('true means [ 4. -4.] with weights [0.3 0.7]')
