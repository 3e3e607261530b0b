"""Model scripts of the Gaussian mixture under stochastic variational inference
(bayespy/demos/stochastic_inference.py:93-133), shared by tools/make_golden_gmm_svi.py -- which runs
them on the live reference -- and the tests, which run them on this package:
``mods = dict(nodes=<module with the node classes>, VB=<class>, vb_kwargs=..., after_vb=...)``.

Every case is a dict of inputs (``make_inputs``) and gives a dict of recorded arrays (``run_case``):
after every step the bound, the per-node bound terms (Y, z, mu, alpha, then Lambda where it is a
node) and the moments of the global nodes; at the end ``Z.u[0]`` of the last mini-batch."""
import numpy as np

CASES = ('demo', 'wishart_d3', 'wishart_d9', 'wishart_d17', 'updates', 'const_kdd')


def _spd(rs, D, cond):
    """A symmetric matrix with eigenvalues between 1 and ``cond``."""
    q, _ = np.linalg.qr(rs.normal(size=(D, D)))
    e = np.exp(rs.uniform(0.0, np.log(cond), size=D))
    a = (q * e) @ q.T
    return 0.5 * (a + a.T)


def _mixture_data(rs, N, D, K_true, spread):
    means = spread * rs.normal(size=(K_true, D))
    z = rs.randint(K_true, size=N)
    return means[z] + rs.normal(size=(N, D))


def make_inputs(rs):
    g = {}

    def case(tag, N, NB, D, K, steps, K_true, spread=4.0):
        # float32 values (exact in float64): half the size in the fixture
        g[tag + '_data'] = _mixture_data(rs, N, D, K_true, spread).astype(np.float32)
        g[tag + '_batches'] = np.stack([rs.choice(N, NB) for _ in range(steps)])
        g[tag + '_mu0'] = spread * rs.normal(size=(K, D))
        g[tag + '_dims'] = np.array([N, NB, D, K])
    case('demo', 600, 50, 2, 4, 8, 3)
    case('wishart_d3', 400, 40, 3, 5, 6, 4)
    case('wishart_d9', 120, 40, 9, 3, 3, 3)
    case('wishart_d17', 100, 50, 17, 2, 3, 2)
    case('updates', 360, 30, 2, 3, 5, 3)
    case('const_kdd', 300, 30, 3, 3, 4, 3)
    g['const_kdd_Lambda'] = np.stack([_spd(rs, 3, 20.0) for _ in range(3)])
    return g


def build(mods, g, tag):
    """The nodes of case ``tag``: dict(Y, Z, mu, alpha[, Lambda]) -- nothing observed yet."""
    N_ = mods['nodes']
    N, NB, D, K = (int(v) for v in g[tag + '_dims'])
    alpha = N_.Dirichlet(np.ones(K), name='class probabilities')
    Z = N_.Categorical(alpha, plates=(NB,), plates_multiplier=(N / NB,), name='classes')
    m = dict(alpha=alpha, Z=Z)
    if tag == 'demo':
        # the demo as written: Gaussian(0, I) means, the precision fixed to the identity
        mu = N_.Gaussian(np.zeros(D), np.identity(D), plates=(K,), name='means')
        Lam = np.identity(D)
    elif tag == 'const_kdd':
        mu = N_.Gaussian(np.zeros(D), 0.01 * np.identity(D), plates=(K,), name='means')
        Lam = g[tag + '_Lambda']
    else:
        mu = N_.GaussianARD(0, 0.01, shape=(D,), plates=(K,), name='means')
        Lam = N_.Wishart(D + 1.0, np.identity(D), plates=(K,), name='precisions')
        m['Lambda'] = Lam
    m['mu'] = mu
    m['Y'] = N_.Mixture(Z, N_.Gaussian, mu, Lam, name='observations')
    mu.initialize_from_value(g[tag + '_mu0'])
    return m


def run_case(mods, g, tag, observe=None, on_step=None):
    """Run the mini-batch loop of case ``tag``; ``observe(Y, rows, n)`` may replace ``Y.observe``
    (device tensors), ``on_step(Q, m, n)`` runs after every step."""
    m = build(mods, g, tag)
    Y, Z, mu, alpha = m['Y'], m['Z'], m['mu'], m['alpha']
    Lam = m.get('Lambda')
    glob = [mu, alpha] + ([Lam] if Lam is not None else [])
    Q = mods['VB'](Y, Z, *glob, **mods.get('vb_kwargs', {}))
    Q.ignore_bound_checks = True
    if 'after_vb' in mods:
        mods['after_vb'](Q)
    data, batches = g[tag + '_data'].astype(np.float64), g[tag + '_batches']
    out = {k: [] for k in ('L', 'terms', 'mu_u0', 'mu_u1', 'alpha_u0', 'Lambda_u0', 'Lambda_u1')}
    for n in range(len(batches)):
        rows = data[batches[n], :]
        if observe is None:
            Y.observe(rows)
        else:
            observe(Y, rows, n)
        Q.update(Z, verbose=False)
        if tag == 'demo':
            Q.gradient_step(mu, alpha, scale=(n + 1) ** (-0.7))
        elif tag == 'updates':
            # a step per global node (each sees what the one before it left), then all three at once
            if n % 2 == 0:
                Q.update(mu, verbose=False)
                Q.update(Lam, verbose=False)
                Q.update(alpha, verbose=False)
            else:
                Q.gradient_step(mu, Lam, alpha, scale=1.0)
        elif tag == 'const_kdd':
            Q.gradient_step(mu, alpha, scale=(n + 2) ** (-0.6))
        else:
            Q.gradient_step(mu, Lam, alpha, scale=(n + 1) ** (-0.7))
        out['L'].append(float(Q.compute_lowerbound()))
        out['terms'].append([float(x.lower_bound_contribution()) for x in [Y, Z] + glob])
        out['mu_u0'].append(np.array(mu.u[0]))
        out['mu_u1'].append(np.array(mu.u[1]))
        out['alpha_u0'].append(np.array(alpha.u[0]))
        if Lam is not None:
            out['Lambda_u0'].append(np.array(Lam.u[0]))
            out['Lambda_u1'].append(np.array(Lam.u[1]))
        if on_step is not None:
            on_step(Q, m, n)
    res = {tag + '_' + k: np.array(v) for k, v in out.items() if len(v)}
    res[tag + '_Z_u0_last'] = np.array(Z.u[0])
    res[tag + '_plan'] = Q
    return res


def check_case(res, g, tag):
    """The recorded trace of the reference against a run: bound rtol 1e-9, per-node terms rtol 1e-9 /
    atol 1e-9, moments rtol 1e-7 / atol 1e-10 (the tolerances of the generic engine's test of the
    same kind of trace)."""
    np.testing.assert_allclose(res[tag + '_L'], g[tag + '_L'], rtol=1e-9)
    np.testing.assert_allclose(res[tag + '_terms'], g[tag + '_terms'], rtol=1e-9, atol=1e-9)
    for k in ('mu_u0', 'mu_u1', 'alpha_u0', 'Lambda_u0', 'Lambda_u1', 'Z_u0_last'):
        if tag + '_' + k in g:
            np.testing.assert_allclose(res[tag + '_' + k], g[tag + '_' + k], rtol=1e-7, atol=1e-10,
                                       err_msg=tag + '_' + k)
