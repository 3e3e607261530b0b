"""TEST INFRASTRUCTURE: the Gaussian hidden-Markov-model script of doc/source/examples/hmm.rst at
D = 12, K = 3 with two ragged chains (lengths as a trailing mask, NaN at every masked ``y``), in
form (a) -- constant mu and Lambda -- and form (b) -- GaussianARD / Wishart nodes.  It runs,
statement for statement, on the reference (tools/make_golden_hmm_wide.py ->
tests/golden/hmm_wide.npz) and on this framework (tests/test_hmm_wide_gpu.py).  ``mods`` as in
tests/hmm_models.py."""
import numpy as np

from hmm_models import _data, build_hmm, trailing

N_ITER = 4
FORMS = (('a', False), ('b', True))


def make_inputs(rs):
    g = {}
    _data(g, rs, 'a', (2,), 40, 12, 3, True)
    _data(g, rs, 'b', (2,), 40, 12, 3, False)
    for tag, _ in FORMS:
        g[tag + '_mask'] = trailing((40, 27), 40)
        g[tag + '_y'] = np.where(g[tag + '_mask'][..., None], g[tag + '_y'], np.nan)
    return g


def run_cases(mods, g, n_iter=N_ITER):
    """Per form: <tag>_L, <tag>_Z_u0 / _Z_u1, <tag>_A_u0, <tag>_a0_u0 (form (b): <tag>_mu_u0,
    <tag>_Lambda_u0) and the engine itself as <tag>_plan."""
    out = {}
    for tag, learned in FORMS:
        m = build_hmm(mods, g[tag + '_y'], g[tag + '_mu'], g[tag + '_Lambda'], observe=False,
                      learned=learned)
        m['Y'].observe(g[tag + '_y'], mask=g[tag + '_mask'])
        m['Z'].initialize_from_value(g[tag + '_z0'])
        more = (m['mu'], m['Lambda']) if learned else ()
        Q = mods['VB'](m['Y'], m['Z'], m['A'], m['a0'], *more, **mods.get('vb_kwargs', {}))
        Q.ignore_bound_checks = True
        Q.update(*more, m['A'], m['a0'], m['Z'], repeat=n_iter, verbose=False)
        out[tag + '_L'] = np.array(Q.L[:n_iter])
        u = m['Z'].get_moments()
        out[tag + '_Z_u0'], out[tag + '_Z_u1'] = np.array(u[0]), np.array(u[1])
        out[tag + '_A_u0'] = np.array(m['A'].get_moments()[0])
        out[tag + '_a0_u0'] = np.array(m['a0'].get_moments()[0])
        if learned:
            out[tag + '_mu_u0'] = np.array(m['mu'].get_moments()[0])
            out[tag + '_Lambda_u0'] = np.array(m['Lambda'].get_moments()[0])
        out[tag + '_plan'] = Q
    return out
