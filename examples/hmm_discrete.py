#!/usr/bin/env python
"""
The discrete hidden Markov model of doc/source/examples/hmm.rst (first half) on the fused block
with categorical emissions (inference/plans/hmm_cat.py), then a batch of ragged sequences over a
learned emission table.

    python examples/hmm_discrete.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def weather():
    """hmm.rst: rainy / sunny days seen through walk / shop / clean.  a0, A and P are known, so Y
    and Z are the whole model and one update gives the exact posterior."""
    from bayespy_amd.nodes import CategoricalMarkovChain, Categorical, Mixture
    from bayespy_amd.inference import VB
    rs = np.random.RandomState(1)
    N = 100
    a0 = [0.6, 0.4]                     # p(rainy) = 0.6, p(sunny) = 0.4
    A = [[0.7, 0.3],                    # p(rainy -> rainy) = 0.7, p(rainy -> sunny) = 0.3
         [0.4, 0.6]]                    # p(sunny -> rainy) = 0.4, p(sunny -> sunny) = 0.6
    P = [[0.1, 0.4, 0.5],
         [0.6, 0.3, 0.1]]
    weather = np.empty(N, dtype=int)
    s = rs.choice(2, p=a0)
    for n in range(N):
        weather[n] = s
        s = rs.choice(2, p=A[s])
    activity = np.array([rs.choice(3, p=P[w]) for w in weather])

    Z = CategoricalMarkovChain(a0, A, states=N)
    Y = Mixture(Z, Categorical, P)
    Y.observe(activity)
    Q = VB(Y, Z, engine='fused')
    Q.update()
    p_rainy = Y.parents[0].get_moments()[0][:, 0]
    print('log p(activity) = %.6f' % Q.L[0])
    print('days whose likelier weather is the true one: %d of %d'
          % (np.sum((p_rainy > 0.5) == (weather == 0)), N))


def ragged_batch():
    """B sequences of different lengths, padded to T and masked past their ends (any integer may
    stand there: -1 here); the transition and emission tables are learned."""
    from bayespy_amd.nodes import Dirichlet, CategoricalMarkovChain, Categorical, Mixture
    from bayespy_amd.inference import VB
    rs = np.random.RandomState(2)
    B, T, K, M = 200, 60, 3, 8
    A_true = 0.1 * np.ones((K, K)) + 0.7 * np.identity(K)
    P_true = rs.dirichlet(0.3 * np.ones(M), size=K)
    lengths = rs.randint(5, T + 1, size=B)
    y = np.full((B, T), -1)
    for b in range(B):
        s = rs.randint(K)
        for t in range(lengths[b]):
            y[b, t] = rs.choice(M, p=P_true[s])
            s = rs.choice(K, p=A_true[s])
    mask = np.arange(T)[None, :] < lengths[:, None]

    a0 = Dirichlet(np.ones(K), name='a0')
    A = Dirichlet(np.ones((K, K)), name='A')
    P = Dirichlet(np.ones((K, M)), name='P')
    Z = CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    Y = Mixture(Z, Categorical, P, name='Y')
    Y.observe(y, mask=mask)
    # random labels make the K emission rows alike and leave VB on that plateau; labels that
    # depend on the word break the symmetry
    Z.initialize_from_value(np.where(mask, y, 0) % K)
    Q = VB(Y, P, A, a0, Z, engine='fused')
    Q.update(repeat=200, tol=1e-9, verbose=False)
    print("%d sweeps, lower bound %.2f" % (Q.iter, Q.L[Q.iter - 1]))
    P_hat = np.exp(P.get_moments()[0])
    P_hat /= P_hat.sum(-1, keepdims=True)
    err = [min(np.abs(P_hat[k] - P_true[j]).max() for k in range(K)) for j in range(K)]
    print('largest distance of a true emission row from its closest learned row:',
          np.round(err, 3))


if __name__ == '__main__':
    weather()
    ragged_batch()
