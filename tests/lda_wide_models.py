"""Latent-Dirichlet-allocation models with more than 64 topics (doc/source/examples/lda.rst), shared
statement for statement by the fixture generator tools/make_golden_lda_wide.py, which runs them on
the reference, and the tests, which run them on this package.  ``mods`` is that of
tests/lda_models.py plus ``params``: a function (Q, model) -> (alpha of p_topic (D, K), alpha of
p_word (K, V)), the Dirichlet parameters as each side keeps them."""
import numpy as np

from lda_models import build_lda

D, N, V, SWEEPS = 7, 400, 30, 5
# tag -> topics
WIDE_CASES = {'k70': 70, 'k130': 130}
EMPTY_DOC, EMPTY_WORDS = 3, (0, 17)


def make_wide_inputs(rs):
    """Inputs and initial moments; document 3 and the words 0 and 17 have no token."""
    g = {}
    docs = rs.choice([d for d in range(D) if d != EMPTY_DOC], size=N)
    words = rs.choice([w for w in range(V) if w not in EMPTY_WORDS], size=N)
    g['docs'], g['words'] = docs.astype(np.int64), words.astype(np.int64)
    for tag, K in WIDE_CASES.items():
        g[tag + '_theta0'] = rs.dirichlet(np.ones(K), size=D)
        g[tag + '_beta0'] = rs.dirichlet(np.ones(V), size=K)
    return g


def run_wide_case(mods, g, tag, sweeps=SWEEPS, after_sweep=None):
    """{key: array}: after every sweep the bound, every per-node term and both Dirichlet
    parameter tables.  ``after_sweep(Q, it)`` runs between the sweeps."""
    K = WIDE_CASES[tag]
    m = build_lda(mods, g['docs'], g['words'], D, V, K)
    m['p_topic'].initialize_from_value(g[tag + '_theta0'])
    m['p_word'].initialize_from_value(g[tag + '_beta0'])
    Q = mods['VB'](m['words'], m['topics'], m['p_word'], m['p_topic'], **mods.get('vb_kwargs', {}))
    if 'after_vb' in mods:
        mods['after_vb'](Q)
    Q.ignore_bound_checks = True
    at, ab = [], []
    for it in range(sweeps):
        Q.update(repeat=1, verbose=False)
        a, b = mods['params'](Q, m)
        at.append(np.array(a, dtype=np.float64))
        ab.append(np.array(b, dtype=np.float64))
        if after_sweep is not None:
            after_sweep(Q, it)
    out = {tag + '_plan': Q, tag + '_model': m, tag + '_L': np.array(Q.L[:sweeps]),
           tag + '_alpha_topic': np.array(at), tag + '_alpha_word': np.array(ab)}
    for nm in ('words', 'topics', 'p_word', 'p_topic'):
        out['%s_l_%s' % (tag, nm)] = np.array(Q.l[m[nm]][:sweeps])
    return out


def plan_params(Q, m):
    """The parameters as the fused plan keeps them (p_word transposed)."""
    plan = Q.plans[0]
    return plan.alpha_theta.cpu().numpy(), plan.alpha_beta_t.cpu().numpy().T
