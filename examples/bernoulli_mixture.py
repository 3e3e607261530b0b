"""Bernoulli mixture (doc/source/examples/bmm.rst) at a size the reference cannot hold: ten
million rows of 64 binary observations, 32 clusters.  The reference forms (N, D, K) arrays of
doubles (164 GB each here); the fused block keeps the observations as 80 MB of bits and one pass
leaves the statistics S_dk and N_k.  Opt-in: ``engine='fused'``.

    python examples/bernoulli_mixture.py [rows]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bayespy_amd import nodes                                                          # noqa: E402
from bayespy_amd.inference import VB                                                   # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10 ** 7
D, K = 64, 32

# artificial data drawn from the model itself, in pieces (no (N, D) array of doubles on the host)
rs = np.random.RandomState(0)
p_true = rs.beta(0.3, 0.3, size=(K, D))
x = np.empty((N, D), dtype=bool)
for lo in range(0, N, 1 << 18):
    hi = min(N, lo + (1 << 18))
    z = rs.randint(K, size=hi - lo)
    x[lo:hi] = rs.random_sample((hi - lo, D)) < p_true[z]

R = nodes.Dirichlet(K * [1e-5], name='R')
Z = nodes.Categorical(R, plates=(N, 1), name='Z')
P = nodes.Beta([0.5, 0.5], plates=(D, K), name='P')
X = nodes.Mixture(Z, nodes.Bernoulli, P, name='X')
X.observe(x)
P.initialize_from_random()

Q = VB(Z, R, X, P, engine='fused')
print('plan:', type(Q.plans[0]).__name__)
Q.update(repeat=30)
weights = np.exp(R.get_moments()[0])
print('clusters with more than 1% of the rows:', int(np.sum(weights / weights.sum() > 0.01)))
