"""Models with the maximum-likelihood nodes GammaShape / Concentration, shared (statement for
statement) by the fixture generator tools/make_golden_ml.py, which runs them on the reference, and
the tests, which run them on this package.

The sweeps are driven node by node (``node.update()`` in the order of the VB call, then the sum of
the nodes' bound terms): the reference's VB cannot add up the bound of a Concentration node with
plates (its ``lower_bound_contribution`` is an array over the plates, dirichlet.py:323-327)."""
import numpy as np


def make_ml_inputs(rs):
    g = {}
    # 1. the gamma-shape demo (demos/gamma_shape.py)
    g['gs_tau'] = rs.gamma(10.0, 1.0 / 20.0, size=1000)
    # 2. GammaShape with plates and its own m0 / m1
    g['gp_tau'] = rs.gamma([2.0, 5.0, 0.7], 1.0 / np.array([1.0, 3.0, 0.5]), size=(40, 3))
    g['gp_m0'], g['gp_m1'] = np.array([0.3, -0.2, 0.1]), 2.0
    # 3. / 4. Concentration(4) -> Dirichlet(plates=(30, 1)) -> Categorical(plates=(30, 200))
    p = rs.dirichlet([2.0, 0.5, 1.0, 4.0], size=30)
    c = (p[:, None, :].cumsum(-1) > rs.rand(30, 200, 1)).argmax(-1)
    g['cc_z'] = c
    g['cc_reg0'], g['cc_reg1'] = np.log(np.array([0.1, 0.2, 0.3, 0.4])), 3.0
    # 5. Concentration(K, plates=(3, 1, 1)) over Dirichlet plates (3, G, 1): rows converge at different
    #    iterations
    K, G, M = 5, 12, 80
    alphas = np.array([[0.3] * K, [5.0] * K, [1.0, 2.0, 3.0, 4.0, 5.0]])
    pp = np.stack([rs.dirichlet(alphas[i], size=G) for i in range(3)])          # (3, G, K)
    u = rs.rand(3, G, M, 1)
    g['cp_z'] = (pp[:, :, None, :].cumsum(-1) > u).argmax(-1)                   # (3, G, M)
    # 6. BetaConcentration -> Beta -> Bernoulli
    q = rs.beta(2.0, 5.0, size=25)
    g['bc_x'] = (rs.rand(25, 60) < q[:, None]).astype(np.int64)
    # 7. Gaussian mixture whose assignment Dirichlet has a Concentration parent
    N, D, K = 2000, 3, 4
    mus = rs.normal(0, 4, size=(K, D))
    lab = rs.randint(K, size=N)
    g['gm_y'] = mus[lab] + rs.normal(size=(N, D))
    g['gm_lab0'] = rs.randint(K, size=N)
    return g


def _sweeps(tag, out, nodes, n, track):
    Ls = []
    for _ in range(n):
        for nd in nodes:
            nd.update()
        Ls.append(float(sum(np.sum(nd.lower_bound_contribution()) for nd in nodes)))
    out[tag + '_L'] = np.array(Ls)
    for nm, nd in track.items():
        out['%s_%s_u' % (tag, nm)] = [np.array(v) for v in nd.get_moments()]


def run_ml_cases(nodes_mod, vb_cls, g, only=None):
    N_ = nodes_mod
    out = {}

    def want(tag):
        return only is None or tag in only

    if want('gs'):
        a = N_.GammaShape(name='a')
        b = N_.Gamma(1e-5, 1e-5, name='b')
        tau = N_.Gamma(a, b, plates=(1000,), name='tau')
        tau.observe(g['gs_tau'])
        _sweeps('gs', out, [tau, a, b], 200, dict(a=a, b=b))

    if want('gp'):
        a = N_.GammaShape(m0=g['gp_m0'], m1=float(g['gp_m1']), plates=(3,), name='a')
        b = N_.Gamma(1.0, 1.0, plates=(3,), name='b')
        tau = N_.Gamma(a, b, plates=(40, 3), name='tau')
        tau.observe(g['gp_tau'])
        _sweeps('gp', out, [tau, a, b], 20, dict(a=a, b=b))

    for tag, reg in (('cc', True), ('cn', False), ('cu', 'user')):
        if not want(tag):
            continue
        if reg == 'user':
            reg = [g['cc_reg0'], float(g['cc_reg1'])]
        c = N_.Concentration(4, regularization=reg, name='c')
        p = N_.Dirichlet(c, plates=(30, 1), name='p')
        z = N_.Categorical(p, plates=(30, 200), name='z')
        z.observe(g['cc_z'])
        _sweeps(tag, out, [z, p, c], 10, dict(c=c, p=p))

    if want('cp'):
        K = 5
        c = N_.Concentration(K, plates=(3, 1, 1), name='c')
        p = N_.Dirichlet(c, plates=(3, 12, 1), name='p')
        z = N_.Categorical(p, plates=(3, 12, 80), name='z')
        z.observe(g['cp_z'])
        _sweeps('cp', out, [z, p, c], 8, dict(c=c, p=p))

    if want('bc'):
        c = N_.BetaConcentration(name='c')
        p = N_.Beta(c, plates=(25, 1), name='p')
        x = N_.Bernoulli(p, plates=(25, 60), name='x')
        x.observe(g['bc_x'])
        _sweeps('bc', out, [x, p, c], 10, dict(c=c, p=p))

    if want('gm'):
        y = g['gm_y']
        N, D = y.shape
        K = 4
        c = N_.Concentration(K, name='c')
        alpha = N_.Dirichlet(c, name='alpha')
        z = N_.Categorical(alpha, plates=(N,), name='z')
        mu = N_.GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
        Lam = N_.Wishart(D, 0.01 * np.identity(D), plates=(K,), name='Lambda')
        Y = N_.Mixture(z, N_.Gaussian, mu, Lam, plates=(N,), name='Y')
        z.initialize_from_value(g['gm_lab0'])
        Y.observe(y)
        vb_cls(Y, mu, Lam, z, alpha, c)        # compiles the model (the warning names the reason)
        _sweeps('gm', out, [Y, mu, Lam, z, alpha, c], 6, dict(c=c, alpha=alpha, mu=mu))
    return out
