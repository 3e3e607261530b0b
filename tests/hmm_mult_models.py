"""TEST INFRASTRUCTURE: the scripts of tests/hmm_cat_models.py (``run_cases``) with multinomial
emissions, for the reference (tools/make_golden_hmm_mult.py -> tests/golden/hmm_mult.npz) and for
engine='fused+counts'.  The reference checks the counts whatever the mask says, so the inputs
hold valid counts at every masked step."""
import numpy as np

import hmm_cat_models as base

#       plates  T   K  M  learned roles      Z from labels
CASES = dict(
    m=((), 40, 3, 7, ('a0', 'A', 'P'), False),          # one chain, scalar n, all from the prior
    n=((4,), 10, 2, 5, ('a0', 'A', 'P'), True),         # a batch: n per step, ragged tails, a hole
)


def make_inputs(rs):
    g = {}
    for tag, (plates, T, K, M, learned, labels) in CASES.items():
        a0 = rs.dirichlet(np.ones(K))
        A = rs.dirichlet(np.ones(K), size=K) * 0.4 + 0.6 * np.identity(K)
        P = rs.dirichlet(0.5 * np.ones(M), size=K) * 0.9 + 0.1 / M
        n = np.array(20) if tag == 'm' else rs.randint(1, 30, size=plates + (T, 1))
        z = base._sample(rs, plates, T, a0, A, np.identity(K))
        x = np.empty(plates + (T, M), dtype=np.int64)
        for idx in np.ndindex(*plates + (T,)):
            x[idx] = rs.multinomial(int(np.broadcast_to(n, plates + (T, 1))[idx + (0,)]), P[z[idx]])
        g[tag + '_y'], g[tag + '_n'] = x, n
        g[tag + '_a0_prior'] = 0.5 + rs.gamma(1.0, size=K)
        g[tag + '_A_prior'] = 0.5 + rs.gamma(1.0, size=(K, K))
        g[tag + '_P_prior'] = 0.5 + rs.gamma(1.0, size=(K, M))
        g[tag + '_z0'] = rs.randint(K, size=plates + (T,))
    m = base.trailing((10, 7, 10, 1), 10)
    m[0, 4:6] = False
    g['n_mask'] = m
    return g


def build(mods, g, tag, observe=True, fill=None, wrap=lambda m: m):
    N_ = mods['nodes']
    plates, T, K, M, learned, _ = CASES[tag]
    a0, A, P = (N_.Dirichlet(g['%s_%s_prior' % (tag, nm)], name=nm) for nm in ('a0', 'A', 'P'))
    Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=plates, name='Z')
    Y = N_.Mixture(Z, N_.Multinomial, g[tag + '_n'], P, name='Y')
    m = dict(a0=a0, A=A, P=P, Z=Z, Y=Y)

    def obs(key='y'):
        y = g['%s_%s' % (tag, key)]
        if tag + '_mask' in g:
            mask = g[tag + '_mask']
            Y.observe(y if fill is None else np.where(mask[..., None], y, fill), mask=wrap(mask))
        else:
            Y.observe(y)
    m['observe'] = obs
    if observe:
        obs()
    return m


def run_cases(mods, g, **kw):
    keep = base.CASES, base.build
    base.CASES, base.build = CASES, build
    try:
        return base.run_cases(mods, g, **kw)
    finally:
        base.CASES, base.build = keep
