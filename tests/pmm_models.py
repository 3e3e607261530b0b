"""TEST INFRASTRUCTURE: the Poisson-mixture (count clustering) model scripts that run, statement for
statement, on the reference (tools/make_golden_pmm.py -> tests/golden/pmm.npz) and on this framework
(tests/test_pmm_host.py, tests/test_pmm_gpu.py).

``mods``: dict(nodes=<module with Dirichlet, Categorical, Gamma, Poisson, Mixture>, VB=<class>,
vb_kwargs=<dict, optional>, after_vb=<callable(Q), optional>).  ``lam`` is initialised from a value
in every case, as ``P`` is in tests/cmm_models.py."""
import numpy as np

N_ITER = 4
CASES = ('a', 'b', 'c', 'd', 'e', 'f', 'g')
# case -> the case whose data it runs on
SOURCE = dict(a='a', b='a', c='c', d='d', e='e', f='a', g='a')


def make_pmm_inputs(rs):
    g = {}

    def data(tag, N, D, K, scale):
        rates = rs.gamma(2.0, scale, size=(K, D))
        z = rs.randint(K, size=N)
        g[tag + '_x'] = rs.poisson(rates[z]).astype(np.int64)
        g[tag + '_lam0'] = rs.gamma(4.0, scale / 2.0, size=(D, K))
        g[tag + '_z0'] = rs.randint(K, size=(N, 1))
    data('a', 300, 7, 3, 4.0)       # (a), (b), (f) and (g) share it
    data('c', 50, 5, 1, 4.0)        # K = 1
    data('d', 60, 1, 3, 6.0)        # D = 1
    data('e', 40, 6, 2, 1500.0)     # rates near 3000: lgamma(x + 1) and the 16-bit range matter
    g['e_x'][:, 0] = 0              # a column of all zeros
    g['a_alpha'] = np.array([0.5, 1.0, 2.0])
    g['a_a0'] = rs.gamma(2.0, 0.5, size=(7, 3)) + 0.1
    g['a_b0'] = rs.gamma(2.0, 0.2, size=(7, 3)) + 0.05
    m = rs.rand(300, 7) < 0.7       # (f): about 70 % ones, a row and a column of nothing
    m[4], m[:, 2], m[11] = False, False, True
    m[11, 2] = False
    g['f_mask'] = m
    g['g_mask'] = np.ones((300, 7), dtype=bool)
    return g


def build_pmm(mods, x, K, a0=None, b0=None, alpha=None, mask=None, observe=True):
    """The hidden entries of ``x`` are set to zero before ``observe``, which checks every value,
    hidden ones included, in the reference as here."""
    N_ = mods['nodes']
    N, D = np.shape(x)
    R = N_.Dirichlet(K * [1e-2] if alpha is None else alpha, name='R')
    Z = N_.Categorical(R, plates=(N, 1), name='Z')
    lam = N_.Gamma(1e-2 if a0 is None else a0, 1e-3 if b0 is None else b0, plates=(D, K),
                   name='lam')
    X = N_.Mixture(Z, N_.Poisson, lam, name='X')
    if observe:
        if mask is None:
            X.observe(x)
        else:
            X.observe(np.where(mask, x, 0).astype(np.int64), mask=mask)
    return dict(R=R, Z=Z, lam=lam, X=X)


def run_pmm_cases(mods, g, only=None, n_iter=N_ITER):
    """Per case: <tag>_L, <tag>_<node>_Lterm for R, Z, lam, X, <tag>_R_u0, <tag>_lam_u0,
    <tag>_lam_u1, <tag>_Z_u0, <tag>_Z_mask and <tag>_lam_mask; the engine itself as <tag>_plan."""
    out = {}
    for tag in CASES:
        if only is not None and tag not in only:
            continue
        src = SOURCE[tag]
        x, lam0 = g[src + '_x'], g[src + '_lam0']
        K = lam0.shape[1]
        mask = g[tag + '_mask'] if tag + '_mask' in g else None
        if src == 'a':
            m = build_pmm(mods, x, K, a0=g['a_a0'], b0=g['a_b0'], alpha=g['a_alpha'], mask=mask)
        else:
            m = build_pmm(mods, x, K, mask=mask)
        R, Z, lam, X = m['R'], m['Z'], m['lam'], m['X']
        lam.initialize_from_value(lam0)
        if tag == 'b':
            Z.initialize_from_value(g['a_z0'])
        Q = mods['VB'](Z, R, X, lam, **mods.get('vb_kwargs', {}))
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        Q.ignore_bound_checks = True
        if tag == 'b':
            Q.update(lam, Z, R, repeat=n_iter, verbose=False)
        else:
            Q.update(repeat=n_iter, verbose=False)
        out[tag + '_L'] = np.array(Q.L[:n_iter])
        for nm in ('R', 'Z', 'lam', 'X'):
            out['%s_%s_Lterm' % (tag, nm)] = np.array(Q.l[m[nm]][:n_iter])
        out[tag + '_R_u0'] = np.array(R.get_moments()[0])
        out[tag + '_lam_u0'] = np.array(lam.get_moments()[0])
        out[tag + '_lam_u1'] = np.array(lam.get_moments()[1])
        out[tag + '_Z_u0'] = np.array(Z.get_moments()[0])
        out[tag + '_Z_mask'] = np.array(Z.mask)
        out[tag + '_lam_mask'] = np.array(lam.mask)
        out[tag + '_plan'] = Q
    return out
