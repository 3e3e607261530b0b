"""TEST INFRASTRUCTURE: the script of tests/hmm_mult_models.py (``run_cases``) with 65 states, for
the reference (tools/make_golden_hmm_states.py -> tests/golden/hmm_states.npz) and for
engine='fused+states'.  The inputs hold valid counts at every masked step."""
import numpy as np

import hmm_cat_models as base
import hmm_mult_models as mult

#       plates  T   K  M  learned roles      Z from labels
CASES = dict(s=((2,), 6, 65, 5, ('a0', 'A', 'P'), False))   # a batch, n per step, a hole in the mask


def make_inputs(rs):
    (plates, T, K, M, _, _), g = CASES['s'], {}
    a0 = rs.dirichlet(np.ones(K))
    A = rs.dirichlet(np.ones(K), size=K) * 0.4 + 0.6 * np.identity(K)
    P = rs.dirichlet(0.5 * np.ones(M), size=K) * 0.9 + 0.1 / M
    n = rs.randint(1, 30, size=plates + (T, 1))
    z = base._sample(rs, plates, T, a0, A, np.identity(K))
    g['s_y'] = np.array([[rs.multinomial(int(n[b, t, 0]), P[z[b, t]]) for t in range(T)]
                         for b in range(plates[0])])
    g['s_n'] = n
    g['s_a0_prior'] = 0.5 + rs.gamma(1.0, size=K)
    g['s_A_prior'] = 0.5 + rs.gamma(1.0, size=(K, K))
    g['s_P_prior'] = 0.5 + rs.gamma(1.0, size=(K, M))
    g['s_mask'] = np.ones(plates + (T,), dtype=bool)
    g['s_mask'][0, 2:4] = False
    return g


def run_cases(mods, g, **kw):
    keep = mult.CASES
    mult.CASES = CASES
    try:
        return mult.run_cases(mods, g, **kw)
    finally:
        mult.CASES = keep
