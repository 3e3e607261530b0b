"""TEST INFRASTRUCTURE: the categorical-mixture (latent class) model scripts that run, statement for
statement, on the reference (tools/make_golden_cmm.py -> tests/golden/cmm.npz) and on this
framework (tests/test_cmm_host.py, tests/test_cmm_gpu.py).

``mods``: dict(nodes=<module with Dirichlet, Categorical, Mixture>, VB=<class>,
vb_kwargs=<dict, optional>, after_vb=<callable(Q), optional>).  ``P`` is initialised from a value in
every case, as in tests/bmm_models.py."""
import numpy as np

N_ITER = 4
CASES = ('a', 'b', 'c', 'd', 'e', 'f', 'g')
# case -> the case whose data it runs on
SOURCE = dict(a='a', b='a', c='c', d='d', e='e', f='a', g='a')


def make_cmm_inputs(rs):
    g = {}

    def data(tag, N, D, K, M):
        p = rs.dirichlet(0.4 * np.ones(M), size=(K, D))
        z = rs.randint(K, size=N)
        u = rs.rand(N, D, 1)
        g[tag + '_x'] = (u > np.cumsum(p[z], axis=-1)).sum(axis=-1).clip(0, M - 1).astype(np.int64)
        p0 = rs.dirichlet(np.ones(M), size=(D, K)).clip(1e-3, None)
        g[tag + '_p0'] = p0 / p0.sum(axis=-1, keepdims=True)
        g[tag + '_z0'] = rs.randint(K, size=(N, 1))
    data('a', 300, 7, 3, 5)         # (a), (b), (f) and (g) share it
    data('c', 50, 5, 1, 4)          # K = 1
    data('d', 60, 1, 3, 3)          # D = 1
    data('e', 40, 6, 2, 2)          # M = 2, category 1 never observed in column 0
    g['e_x'][:, 0] = 0
    g['a_alpha'] = np.array([0.5, 1.0, 2.0])
    g['a_conc'] = np.array([0.3, 0.5, 1.0, 1.5, 2.0])
    m = rs.rand(300, 7) < 0.7       # (f): about 70 % ones, a row and a column of nothing
    m[4], m[:, 2], m[11] = False, False, True
    m[11, 2] = False
    g['f_mask'] = m
    g['g_mask'] = np.ones((300, 7), dtype=bool)
    return g


def build_cmm(mods, x, K, M, conc=None, alpha=None, mask=None, observe=True):
    """The hidden entries of ``x`` are set to zero before ``observe``, which checks every value,
    hidden ones included, in the reference as here."""
    N_ = mods['nodes']
    N, D = np.shape(x)
    R = N_.Dirichlet(K * [1e-2] if alpha is None else alpha, name='R')
    Z = N_.Categorical(R, plates=(N, 1), name='Z')
    P = N_.Dirichlet(M * [0.5] if conc is None else conc, plates=(D, K), name='P')
    X = N_.Mixture(Z, N_.Categorical, P, name='X')
    if observe:
        if mask is None:
            X.observe(x)
        else:
            X.observe(np.where(mask, x, 0).astype(np.int64), mask=mask)
    return dict(R=R, Z=Z, P=P, X=X)


def run_cmm_cases(mods, g, only=None, n_iter=N_ITER):
    """Per case: <tag>_L, <tag>_<node>_Lterm for R, Z, P, X, <tag>_<node>_u0 for R, P, Z,
    <tag>_Z_mask and <tag>_P_mask; the engine itself as <tag>_plan."""
    out = {}
    for tag in CASES:
        if only is not None and tag not in only:
            continue
        src = SOURCE[tag]
        x, p0 = g[src + '_x'], g[src + '_p0']
        K, M = p0.shape[1], p0.shape[2]
        mask = g[tag + '_mask'] if tag + '_mask' in g else None
        if src == 'a':
            m = build_cmm(mods, x, K, M, conc=g['a_conc'], alpha=g['a_alpha'], mask=mask)
        else:
            m = build_cmm(mods, x, K, M, mask=mask)
        R, Z, P, X = m['R'], m['Z'], m['P'], m['X']
        P.initialize_from_value(p0)
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
        out[tag + '_Z_mask'] = np.array(Z.mask)
        out[tag + '_P_mask'] = np.array(P.mask)
        out[tag + '_plan'] = Q
    return out
