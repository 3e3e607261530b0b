"""TEST INFRASTRUCTURE: the discrete hidden-Markov-model scripts of tests/hmm_cat_models.py
(``build``, ``run_cases``: the same statements) at vocabularies above 128 words, which run on the
reference (tools/make_golden_hmm_vocab.py -> tests/golden/hmm_vocab.npz) and on this framework
through engine='fused+words' (tests/test_hmm_vocab_gpu.py, tests/test_hmm_vocab_host.py)."""
import numpy as np

import hmm_cat_models as base

#       plates  T   K  M    learned roles      Z from labels
CASES = dict(
    w=((), 60, 3, 131, ('a0', 'A', 'P'), False),        # one chain, everything from the prior
    x=((5,), 12, 2, 300, ('a0', 'A', 'P'), True),       # a batch: ragged tails, a hole, fixed labels
)


def _on_cases(fn, *args, **kw):
    keep, base.CASES = base.CASES, CASES
    try:
        return fn(*args, **kw)
    finally:
        base.CASES = keep


def make_inputs(rs):
    g = {}
    for tag, (plates, T, K, M, learned, labels) in CASES.items():
        a0 = rs.dirichlet(np.ones(K))
        A = rs.dirichlet(np.ones(K), size=K) * 0.4 + 0.6 * np.identity(K)
        P = rs.dirichlet(0.5 * np.ones(M), size=K) * 0.9 + 0.1 / M
        g[tag + '_y'] = base._sample(rs, plates, T, a0, A, P)
        g[tag + '_a0_prior'] = 0.5 + rs.gamma(1.0, size=K)
        g[tag + '_A_prior'] = 0.5 + rs.gamma(1.0, size=(K, K))
        g[tag + '_P_prior'] = 0.5 + rs.gamma(1.0, size=(K, M))
        g[tag + '_z0'] = rs.randint(K, size=plates + (T,))
    m = base.trailing((12, 9, 12, 4, 1), 12)
    m[0, 5:7] = False
    g['x_mask'] = m
    g['x_y'] = np.where(m, g['x_y'], 0)     # the reference checks the words whatever the mask says
    return g


def build(mods, g, tag, **kw):
    return _on_cases(base.build, mods, g, tag, **kw)


def run_cases(mods, g, **kw):
    return _on_cases(base.run_cases, mods, g, **kw)
