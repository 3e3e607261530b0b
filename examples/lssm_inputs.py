#!/usr/bin/env python
"""A driven linear state-space model, x_t = A x_{t-1} + B u_t + noise, over a batch of sequences: a
damped oscillator pushed by a known control signal.  ``GaussianMarkovChain(..., inputs=u)`` takes
the controls as its fifth parent; the dynamics node then holds [A | B] row by row, so the input gain
B is learned together with A.  The states are observed directly (C = I), which keeps A and B
identifiable, and the sequences share [A | B] and nu, so the generic engine takes the input cross
terms of the messages from one pass over the means (vmp_chain_input_stats)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bayespy_amd.nodes import GaussianARD, Gamma, GaussianMarkovChain       # noqa: E402
from bayespy_amd.inference import VB                                          # noqa: E402

np.random.seed(5)
Bs, T, D, K = 200, 100, 2, 1
w, r = 0.3, 0.97
a_true = r * np.array([[np.cos(w), -np.sin(w)], [np.sin(w), np.cos(w)]])
b_true = np.array([[0.0], [0.8]])
u = np.sign(np.sin(0.11 * np.arange(T - 1)[None, :, None] + np.random.rand(Bs, 1, 1) * 6.0))
x = np.zeros((Bs, T, D))
x[:, 0] = np.random.randn(Bs, D)
for t in range(1, T):
    x[:, t] = x[:, t - 1] @ a_true.T + u[:, t - 1] @ b_true.T + 0.1 * np.random.randn(Bs, D)
y = x + 0.2 * np.random.randn(Bs, T, D)

alpha = Gamma(1e-5, 1e-5, plates=(D + K,), name='alpha')
AB = GaussianARD(0, alpha, shape=(D + K,), plates=(D,), name='AB')
AB.initialize_from_value(np.concatenate([np.identity(D), np.zeros((D, K))], axis=-1))
nu = Gamma(1e-3, 1e-3, plates=(D,), name='nu')
X = GaussianMarkovChain(np.zeros(D), 1e-3 * np.identity(D), AB, nu, n=T, inputs=u, plates=(Bs,),
                        name='X')
tau = Gamma(1e-5, 1e-5, name='tau')
Y = GaussianARD(X.as_gaussian(), tau, name='Y')
Y.observe(y)

Q = VB(X, AB, alpha, nu, tau, Y)
print('engine:', type(Q.plans[0]).__name__)
Q.update(repeat=50, tol=1e-7)
m = np.array(AB.u[0])
print('A: true\n%s\nestimated\n%s' % (np.round(a_true, 3), np.round(m[:, :D], 3)))
print('B: true %s, estimated %s' % (b_true.ravel(), np.round(m[:, D:].ravel(), 3)))
print('noise sd: true 0.2, estimated %.3f' % (1.0 / np.sqrt(float(np.array(tau.u[0])))))
