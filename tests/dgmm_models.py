"""TEST INFRASTRUCTURE: the diagonal-Gaussian-mixture model scripts

    alpha = Dirichlet(a);  Z = Categorical(alpha, plates=(N, 1))
    mu = GaussianARD(m0, beta0, plates=(D, K));  tau = Gamma(a0, b0, plates=(D, K))
    Y = Mixture(Z, GaussianARD, mu, tau);  Y.observe(y)

that run, statement for statement, on the reference (tools/make_golden_dgmm.py ->
tests/golden/dgmm.npz) and on this framework (tests/test_dgmm_host.py, tests/test_dgmm_gpu.py).

``mods``: dict(nodes=<module with Dirichlet, Categorical, GaussianARD, Gamma, Mixture>, VB=<class>,
vb_kwargs=<dict, optional>, after_vb=<callable(Q), optional>).

Cases: (a) N = 120, D = 6, K = 4 from fixed labels and ``mu`` from parameters, 6 sweeps in the
order Z, mu, tau, alpha; (b) array priors (D, K) with m0 != 0, ``mu.initialize_from_value``, Z from
its prior; (c) N = D = K = 1; (d) ``observe`` after ``VB(...)`` and a re-observe with other data;
(e) ``tau`` (from parameters, as ``alpha``) updated before ``mu``; (f) from fixed labels in the
order mu, tau, alpha, Z, where the labels decide the first statistics."""
import numpy as np

N_ITER = 6
CASES = ('a', 'b', 'c', 'd', 'e', 'f')
ORDER = dict(a='Z mu tau alpha', b='Z mu tau alpha', c='Z mu tau alpha', d='Z mu tau alpha',
             e='Z tau mu alpha', f='mu tau alpha Z')
NODES = ('alpha', 'Z', 'mu', 'tau', 'Y')


def _data(rs, N, D, K, spread=3.0):
    centres = spread * rs.normal(size=(K, D))
    z = rs.randint(K, size=N)
    return centres[z] + rs.gamma(4.0, 0.25, size=(K, D))[z] * rs.normal(size=(N, D)), z, centres


def make_inputs(rs):
    g = {}
    g['a_y'], g['a_z0'], cen = _data(rs, 120, 6, 4)
    g['a_mu0'] = cen.T + rs.normal(size=(6, 4))
    # (b) array priors
    N, D, K = 90, 5, 3
    g['b_y'], _, cen = _data(rs, N, D, K)
    g['b_m0'] = rs.normal(size=(D, K))
    g['b_beta0'] = rs.gamma(2.0, 0.05, size=(D, K))
    g['b_a0'] = rs.gamma(2.0, 0.5, size=(D, K))
    g['b_b0'] = rs.gamma(2.0, 0.5, size=(D, K))
    g['b_alpha'] = rs.gamma(2.0, 1.0, size=K)
    g['b_mu0'] = cen.T + 0.5 * rs.normal(size=(D, K))
    # (c) one of everything
    g['c_y'] = rs.normal(size=(1, 1))
    # (d) two data sets of one shape
    g['d_y'], _, cen = _data(rs, 70, 3, 3)
    g['d_y2'] = _data(rs, 70, 3, 3)[0]
    g['d_mu0'] = cen.T + 0.5 * rs.normal(size=(3, 3))
    # (e) tau before mu, tau and alpha from parameters
    g['e_y'], _, cen = _data(rs, 65, 17, 2)
    g['e_mu0'] = cen.T + 0.5 * rs.normal(size=(17, 2))
    g['e_tau_a'] = rs.gamma(4.0, 1.0, size=(17, 2))
    g['e_tau_b'] = rs.gamma(4.0, 1.0, size=(17, 2))
    g['e_alpha'] = rs.gamma(3.0, 1.0, size=2)
    # (f) the labels decide
    g['f_y'], z, _ = _data(rs, 70, 3, 3)
    g['f_z0'] = np.where(rs.rand(70) < 0.8, z, rs.randint(3, size=70))
    return g


def build_dgmm(mods, N, D, K, y=None, m0=0.0, beta0=1e-3, a0=1e-2, b0=1e-2, alpha=None):
    N_ = mods['nodes']
    al = N_.Dirichlet(K * [0.5] if alpha is None else alpha, name='alpha')
    Z = N_.Categorical(al, plates=(N, 1), name='Z')
    mu = N_.GaussianARD(m0, beta0, plates=(D, K), name='mu')
    tau = N_.Gamma(a0, b0, plates=(D, K), name='tau')
    Y = N_.Mixture(Z, N_.GaussianARD, mu, tau, name='Y')
    if y is not None:
        Y.observe(y)
    return dict(alpha=al, Z=Z, mu=mu, tau=tau, Y=Y)


def run_cases(mods, g, only=None, n_iter=N_ITER):
    """Per case: <tag>_L, <tag>_<node>_Lterm for the five nodes, <tag>_alpha_u0, <tag>_Z_u0,
    <tag>_mu_u0 / _u1, <tag>_tau_u0 / _u1; the engine itself as <tag>_plan."""
    out = {}
    for tag in CASES:
        if only is not None and tag not in only:
            continue
        y = g[tag + '_y']
        N, D = y.shape
        if tag == 'b':
            K = g['b_m0'].shape[1]
            m = build_dgmm(mods, N, D, K, y, m0=g['b_m0'], beta0=g['b_beta0'], a0=g['b_a0'],
                           b0=g['b_b0'], alpha=g['b_alpha'])
        elif tag == 'c':
            K = 1
            m = build_dgmm(mods, N, D, K, y)
        else:
            K = {'a': 4, 'd': 3, 'e': 2, 'f': 3}[tag]
            m = build_dgmm(mods, N, D, K, None if tag == 'd' else y)
        if tag in ('a', 'f'):
            m['Z'].initialize_from_value(g[tag + '_z0'][:, None])
        if tag == 'a':
            m['mu'].initialize_from_parameters(g['a_mu0'], 1.0)
        if tag in ('b', 'd', 'e'):
            m['mu'].initialize_from_value(g[tag + '_mu0'])
        if tag == 'e':
            m['tau'].initialize_from_parameters(g['e_tau_a'], g['e_tau_b'])
            m['alpha'].initialize_from_parameters(g['e_alpha'])
        Q = mods['VB'](m['Y'], m['Z'], m['mu'], m['tau'], m['alpha'], **mods.get('vb_kwargs', {}))
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        Q.ignore_bound_checks = True
        order = [m[nm] for nm in ORDER[tag].split()]
        if tag == 'd':
            m['Y'].observe(y)
            Q.update(*order, repeat=n_iter // 2, verbose=False)
            m['Y'].observe(g['d_y2'])
            Q.update(*order, repeat=n_iter - n_iter // 2, verbose=False)
        else:
            Q.update(*order, repeat=n_iter, verbose=False)
        out[tag + '_L'] = np.array(Q.L[:n_iter])
        for nm in NODES:
            out['%s_%s_Lterm' % (tag, nm)] = np.array(Q.l[m[nm]][:n_iter])
        out[tag + '_alpha_u0'] = np.array(m['alpha'].get_moments()[0])
        out[tag + '_Z_u0'] = np.array(m['Z'].get_moments()[0])
        for nm in ('mu', 'tau'):
            u = m[nm].get_moments()
            out['%s_%s_u0' % (tag, nm)] = np.array(u[0])
            out['%s_%s_u1' % (tag, nm)] = np.array(u[1])
        out[tag + '_plan'] = Q
    return out
