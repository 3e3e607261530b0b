"""TEST INFRASTRUCTURE: the Bernoulli-mixture model scripts (doc/source/examples/bmm.rst) that run,
statement for statement, on the reference (tools/make_golden_bmm.py -> tests/golden/bmm_fused.npz)
and on this framework (tests/test_bmm_host.py, tests/test_bmm_gpu.py).

``mods``: dict(nodes=<module with Dirichlet, Categorical, Beta, Mixture, Bernoulli>, VB=<class>,
vb_kwargs=<dict, optional>, after_vb=<callable(Q), optional>)."""
import numpy as np

N_ITER = 4


def make_bmm_inputs(rs):
    g = {}

    def data(tag, N, D, K):
        p = rs.beta(0.4, 0.4, size=(K, D))
        z = rs.randint(K, size=N)
        g[tag + '_x'] = (rs.rand(N, D) < p[z]).astype(np.int64)
        g[tag + '_p0'] = rs.beta(0.5, 0.5, size=(D, K)).clip(1e-3, 1 - 1e-3)
        g[tag + '_z0'] = rs.randint(K, size=(N, 1))
    data('a', 300, 70, 3)           # (a) and (b) share it
    data('c', 50, 5, 1)             # K = 1
    data('d', 60, 1, 3)             # D = 1
    data('e', 40, 9, 2)             # rows of zeros and rows of ones
    g['e_x'][:6] = 0
    g['e_x'][6:11] = 1
    g['a_alpha'] = np.array([0.5, 1.0, 2.0])
    return g


def build_bmm(mods, x, K, beta=(0.5, 0.5), alpha=None, observe=True, engine_kwargs=None):
    N_ = mods['nodes']
    N, D = np.shape(x)
    R = N_.Dirichlet(K * [1e-5] if alpha is None else alpha, name='R')
    Z = N_.Categorical(R, plates=(N, 1), name='Z')
    P = N_.Beta(list(beta), plates=(D, K), name='P')
    X = N_.Mixture(Z, N_.Bernoulli, P, name='X')
    if observe:
        X.observe(x)
    return dict(R=R, Z=Z, P=P, X=X)


CASES = ('a', 'b', 'c', 'd', 'e')


def run_bmm_cases(mods, g, only=None, n_iter=N_ITER):
    """Per case: <tag>_L, <tag>_<node>_Lterm for R, Z, P, X and <tag>_<node>_u0 for R, P, Z; the
    engine itself as <tag>_plan."""
    out = {}
    for tag in CASES:
        if only is not None and tag not in only:
            continue
        src = 'a' if tag == 'b' else tag
        x = g[src + '_x']
        K = g[src + '_p0'].shape[1]
        if tag in ('a', 'b'):
            m = build_bmm(mods, x, K, beta=(2.0, 0.5), alpha=g['a_alpha'])
        else:
            m = build_bmm(mods, x, K)
        R, Z, P, X = m['R'], m['Z'], m['P'], m['X']
        m['P'].initialize_from_value(g[src + '_p0'])
        if tag == 'b':
            Z.initialize_from_value(g['a_z0'])
        Q = mods['VB'](Z, R, X, P, **mods.get('vb_kwargs', {}))
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        Q.ignore_bound_checks = True
        if tag == 'b':
            Q.update(P, Z, R, repeat=n_iter, verbose=False)
        else:
            Q.update(repeat=n_iter, verbose=False)
        out[tag + '_L'] = np.array(Q.L[:n_iter])
        for nm in ('R', 'Z', 'P', 'X'):
            out['%s_%s_Lterm' % (tag, nm)] = np.array(Q.l[m[nm]][:n_iter])
        for nm in ('R', 'P', 'Z'):
            out['%s_%s_u0' % (tag, nm)] = np.array(m[nm].get_moments()[0])
        out[tag + '_plan'] = Q
    return out
