"""TEST INFRASTRUCTURE: the diagonal-Gaussian-mixture model scripts with missing observations

    alpha = Dirichlet(a);  Z = Categorical(alpha, plates=(N, 1))
    mu = GaussianARD(m0, beta0, plates=(D, K));  tau = Gamma(a0, b0, plates=(D, K))
    Y = Mixture(Z, GaussianARD, mu, tau);  Y.observe(y, mask=m)

that run, statement for statement, on the reference (tools/make_golden_dgmm_masked.py ->
tests/golden/dgmm_masked.npz) and on this framework (tests/test_dgmm_masked_host.py,
tests/test_dgmm_masked_gpu.py).

``mods``: dict(nodes=<module with Dirichlet, Categorical, GaussianARD, Gamma, Mixture>, VB=<class>,
vb_kwargs=<dict, optional>, after_vb=<callable(Q), optional>).

Cases (six sweeps each; the hidden entries of every stored y are NaN and are set to zero before
``observe``): (a) data, labels and ``mu`` parameters of case a of tests/golden/dgmm.npz under a 70 %
mask, order Z mu tau alpha; (b) the array priors of its case b, the mask with a row of nothing, a
column of nothing and a row observed everywhere else; (c) N = D = K = 1, observed; (d) case a's data
under a mask of ones; (e) ``observe`` after ``VB(...)``, three sweeps, a re-observe of other data
under another mask, three more; (f) fixed labels that decide the first statistics (order mu tau
alpha Z) with a row of nothing; (g) N = 90, D = 65, K = 2: a second column block at any width."""
import numpy as np

N_ITER = 6
CASES = ('a', 'b', 'c', 'd', 'e', 'f', 'g')
ORDER = dict(a='Z mu tau alpha', b='Z mu tau alpha', c='Z mu tau alpha', d='Z mu tau alpha',
             e='Z mu tau alpha', f='mu tau alpha Z', g='Z mu tau alpha')
NODES = ('alpha', 'Z', 'mu', 'tau', 'Y')
PER_CASE = 1 + 5 + 6 + 2


def make_masked_inputs(rs, plain):
    """``plain``: the in_* arrays of tests/golden/dgmm.npz."""
    g = {}

    def hide(tag, y, m):
        g[tag + '_mask'] = m
        g[tag + '_y'] = np.where(m, y, np.nan)

    ya = plain['a_y']
    g['a_z0'], g['a_mu0'] = plain['a_z0'], plain['a_mu0']
    hide('a', ya, rs.rand(*ya.shape) < 0.7)
    for k in ('b_m0', 'b_beta0', 'b_a0', 'b_b0', 'b_alpha', 'b_mu0'):
        g[k] = plain[k]
    yb = plain['b_y']
    m = rs.rand(*yb.shape) < 0.7
    m[11] = True
    m[4], m[:, 3] = False, False
    hide('b', yb, m)
    hide('c', plain['c_y'], np.ones((1, 1), dtype=bool))
    hide('d', ya, np.ones(ya.shape, dtype=bool))
    g['e_mu0'] = plain['d_mu0']
    hide('e', plain['d_y'], rs.rand(*plain['d_y'].shape) < 0.7)
    m2 = rs.rand(*plain['d_y2'].shape) < 0.6
    g['e_mask2'] = m2
    g['e_y2'] = np.where(m2, plain['d_y2'], np.nan)
    g['f_z0'] = plain['f_z0']
    m = rs.rand(*plain['f_y'].shape) < 0.7
    m[6] = False
    hide('f', plain['f_y'], m)
    N, D, K = 90, 65, 2
    centres = 1.5 * rs.normal(size=(K, D))
    y = centres[rs.randint(K, size=N)] + rs.normal(size=(N, D))
    m = rs.rand(N, D) < 0.7
    m[12, 64] = False
    hide('g', y, m)
    g['g_mu0'] = centres.T + 0.5 * rs.normal(size=(D, K))
    return g


def build_dgmm_masked(mods, N, D, K, y=None, mask=None, m0=0.0, beta0=1e-3, a0=1e-2, b0=1e-2,
                      alpha=None):
    N_ = mods['nodes']
    al = N_.Dirichlet(K * [0.5] if alpha is None else alpha, name='alpha')
    Z = N_.Categorical(al, plates=(N, 1), name='Z')
    mu = N_.GaussianARD(m0, beta0, plates=(D, K), name='mu')
    tau = N_.Gamma(a0, b0, plates=(D, K), name='tau')
    Y = N_.Mixture(Z, N_.GaussianARD, mu, tau, name='Y')
    if y is not None:
        Y.observe(np.where(mask, y, 0.0), mask=mask)
    return dict(alpha=al, Z=Z, mu=mu, tau=tau, Y=Y)


def run_masked_cases(mods, g, only=None, n_iter=N_ITER):
    """Per case: <tag>_L, <tag>_<node>_Lterm for the five nodes, <tag>_alpha_u0, <tag>_Z_u0,
    <tag>_mu_u0 / _u1, <tag>_tau_u0 / _u1, <tag>_Z_mask, <tag>_mu_mask; the engine itself as
    <tag>_plan."""
    out = {}
    for tag in CASES:
        if only is not None and tag not in only:
            continue
        y, mask = g[tag + '_y'], g[tag + '_mask']
        N, D = y.shape
        if tag == 'b':
            K = g['b_m0'].shape[1]
            m = build_dgmm_masked(mods, N, D, K, y, mask, m0=g['b_m0'], beta0=g['b_beta0'],
                                  a0=g['b_a0'], b0=g['b_b0'], alpha=g['b_alpha'])
        else:
            K = {'a': 4, 'c': 1, 'd': 4, 'e': 3, 'f': 3, 'g': 2}[tag]
            m = build_dgmm_masked(mods, N, D, K, None if tag == 'e' else y, mask)
        if tag in ('a', 'd', 'f'):
            m['Z'].initialize_from_value(g[('a' if tag == 'd' else tag) + '_z0'][:, None])
        if tag in ('a', 'd'):
            m['mu'].initialize_from_parameters(g['a_mu0'], 1.0)
        if tag in ('b', 'e', 'g'):
            m['mu'].initialize_from_value(g[tag + '_mu0'])
        Q = mods['VB'](m['Y'], m['Z'], m['mu'], m['tau'], m['alpha'], **mods.get('vb_kwargs', {}))
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        Q.ignore_bound_checks = True
        order = [m[nm] for nm in ORDER[tag].split()]
        if tag == 'e':
            m['Y'].observe(np.where(mask, y, 0.0), mask=mask)
            if 'after_vb' in mods:
                mods['after_vb'](Q)
            Q.update(*order, repeat=n_iter // 2, verbose=False)
            m['Y'].observe(np.where(g['e_mask2'], g['e_y2'], 0.0), mask=g['e_mask2'])
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
        out[tag + '_Z_mask'] = np.array(m['Z'].mask)
        out[tag + '_mu_mask'] = np.array(m['mu'].mask)
        out[tag + '_plan'] = Q
    return out
