"""TEST INFRASTRUCTURE: deterministic annealing (VB.set_annealing) on the two Gaussian-mixture
blocks.  The full-covariance model

    alpha = Dirichlet(a);  z = Categorical(alpha, plates=(N,))
    mu = GaussianARD(0, beta0, shape=(D,), plates=(K,));  Lambda = Wishart(n0, V0, plates=(K,))
    Y = Mixture(z, Gaussian, mu, Lambda);  Y.observe(y)

scripts that run, statement for statement, on the reference (tools/make_golden_anneal.py ->
tests/golden/anneal.npz) and on this framework (tests/test_anneal_gpu.py).

``mods``: dict(nodes=<module with Dirichlet, Categorical, GaussianARD, Gaussian, Wishart,
Mixture>, VB=<class>, vb_kwargs=<dict, optional>).

Cases (the smallest shapes at which the kernels can still go wrong):
  one    N = 300, D = 2, K = 3 (K padded to 16): coefficient 0.5 set before the first update, ``z``
         from ``initialize_from_value``, 5 iterations
  two    the same shape, ``z`` from its prior (and a Dirichlet prior that is not symmetric, so
         that the clusters differ at all): the schedule 0.3, x 1.5 up to 1.0, 3 iterations each;
         then the bound once more after ``set_annealing(0.5)`` with NO update -- the temperature
         of a bound term is the node's at the request
  three  N = 200, D = 17, K = 33 (the wide pass, the clusters split over a wavefront pair): 0.5,
         ``z`` from a value, 3 iterations
The Wishart degrees n0 keep min(coefficient) * n0 > D - 1, so every stored value is finite.

The diagonal model (tests/dgmm_models.py ``build_dgmm``: Z (N, 1), mu and tau with plates (D, K)):
  four   N = 300, D = 5, K = 3: the smallest diagonal case; 0.5, ``Z`` from a value, the order
         mu, tau, alpha, Z, 5 iterations
  five   N = 300, D = 70, K = 17 (D above the 64-column block): ``Z`` from its prior, ``mu`` from a
         value, the order Z, mu, tau, alpha, the schedule of case two and its bound at 0.5 after"""
import numpy as np

CASES = ('one', 'two', 'three')
DIAG_CASES = ('four', 'five')
DIAG_SHAPES = dict(four=(300, 5, 3), five=(300, 70, 17))
DIAG_NODES = ('Y', 'Z', 'alpha', 'mu', 'tau')
SHAPES = dict(one=(300, 2, 3), two=(300, 2, 3), three=(200, 17, 33))
N0 = dict(one=5.0, two=5.0, three=40.0)
MIN_ANNEALING = dict(one=0.5, two=0.3, three=0.5)
NODES = ('Y', 'z', 'alpha', 'mu', 'Lambda')


def schedule(start=0.3, factor=1.5):
    out, b = [], start
    while b < 1.0:
        out.append(b)
        b *= factor
    return out + [1.0]


def make_inputs(rs):
    g = {}
    for tag in CASES:
        N, D, K = SHAPES[tag]
        centres = 4.0 * rs.normal(size=(K, D))
        lab = rs.randint(K, size=N)
        g[tag + '_y'] = centres[lab] + rs.normal(size=(N, D))
        g[tag + '_z0'] = np.where(rs.rand(N) < 0.6, lab, rs.randint(K, size=N))
    g['two_alpha'] = np.array([0.5, 1.5, 3.0])
    for tag in DIAG_CASES:
        N, D, K = DIAG_SHAPES[tag]
        centres = 3.0 * rs.normal(size=(K, D)) / np.sqrt(D) * 2.0
        lab = rs.randint(K, size=N)
        g[tag + '_y'] = centres[lab] + rs.gamma(4.0, 0.25, size=(K, D))[lab] * rs.normal(size=(N, D))
        g[tag + '_z0'] = np.where(rs.rand(N) < 0.6, lab, rs.randint(K, size=N))
        g[tag + '_mu0'] = centres.T + 0.5 * rs.normal(size=(D, K))
    return g


def build(mods, y, K, n0, alpha=None, z0=None):
    N_ = mods['nodes']
    N, D = y.shape
    al = N_.Dirichlet(1e-1 * np.ones(K) if alpha is None else alpha, name='alpha')
    z = N_.Categorical(al, plates=(N,), name='z')
    mu = N_.GaussianARD(0, 1e-2, shape=(D,), plates=(K,), name='mu')
    Lam = N_.Wishart(n0, 0.5 * n0 * np.identity(D), plates=(K,), name='Lambda')
    Y = N_.Mixture(z, N_.Gaussian, mu, Lam, plates=(N,), name='Y')
    if z0 is not None:
        z.initialize_from_value(z0)
    Y.observe(y)
    Q = mods['VB'](Y, mu, Lam, z, al, **mods.get('vb_kwargs', {}))
    Q.ignore_bound_checks = True
    return Q, dict(Y=Y, z=z, alpha=al, mu=mu, Lambda=Lam)


def run_cases(mods, g, only=None):
    """Per case: <tag>_L (the bound after every iteration), <tag>_<node>_Lterm, the final moments
    <tag>_z_u0, _alpha_u0, _mu_u0, _mu_u1, _Lambda_u0, _Lambda_u1; case two also
    two_after_L / two_after_<node>_Lterm (the bound at 0.5 of the q left by the schedule); the
    engine itself as <tag>_plan."""
    out = {}
    for tag in CASES:
        if only is not None and tag not in only:
            continue
        y = g[tag + '_y']
        K = SHAPES[tag][2]
        assert MIN_ANNEALING[tag] * N0[tag] > y.shape[1] - 1
        Q, m = build(mods, y, K, N0[tag], alpha=g['two_alpha'] if tag == 'two' else None,
                     z0=None if tag == 'two' else g[tag + '_z0'])
        if tag == 'two':
            for b in schedule():
                Q.set_annealing(b)
                Q.update(repeat=3, verbose=False)
        else:
            Q.set_annealing(0.5)
            Q.update(repeat=5 if tag == 'one' else 3, verbose=False)
        n = Q.iter
        out[tag + '_L'] = np.array(Q.L[:n])
        for nm in NODES:
            out['%s_%s_Lterm' % (tag, nm)] = np.array(Q.l[m[nm]][:n])
        if tag == 'two':
            Q.set_annealing(0.5)
            out['two_after_L'] = np.array(Q.compute_lowerbound())
            for nm in NODES:
                out['two_after_%s_Lterm' % nm] = np.array(m[nm].lower_bound_contribution())
        out[tag + '_z_u0'] = np.array(m['z'].get_moments()[0])
        out[tag + '_alpha_u0'] = np.array(m['alpha'].get_moments()[0])
        for nm in ('mu', 'Lambda'):
            u = m[nm].get_moments()
            out['%s_%s_u0' % (tag, nm)] = np.array(u[0])
            out['%s_%s_u1' % (tag, nm)] = np.array(u[1])
        out[tag + '_plan'] = Q
    return out


def run_diag_cases(mods, g, only=None):
    """Per case: <tag>_L, <tag>_<node>_Lterm, the final moments <tag>_Z_u0, _alpha_u0, _mu_u0 / _u1,
    _tau_u0 / _u1; case five also five_after_L / five_after_<node>_Lterm; the engine as
    <tag>_plan."""
    from dgmm_models import build_dgmm
    out = {}
    for tag in DIAG_CASES:
        if only is not None and tag not in only:
            continue
        N, D, K = DIAG_SHAPES[tag]
        m = build_dgmm(mods, N, D, K, g[tag + '_y'], beta0=1e-2, a0=0.5, b0=0.5)
        if tag == 'four':
            m['Z'].initialize_from_value(g['four_z0'][:, None])
            order = 'mu tau alpha Z'
        else:
            m['mu'].initialize_from_value(g['five_mu0'])
            order = 'Z mu tau alpha'
        Q = mods['VB'](m['Y'], m['Z'], m['mu'], m['tau'], m['alpha'], **mods.get('vb_kwargs', {}))
        Q.ignore_bound_checks = True
        order = [m[nm] for nm in order.split()]
        if tag == 'five':
            for b in schedule():
                Q.set_annealing(b)
                Q.update(*order, repeat=3, verbose=False)
        else:
            Q.set_annealing(0.5)
            Q.update(*order, repeat=5, verbose=False)
        n = Q.iter
        out[tag + '_L'] = np.array(Q.L[:n])
        for nm in DIAG_NODES:
            out['%s_%s_Lterm' % (tag, nm)] = np.array(Q.l[m[nm]][:n])
        if tag == 'five':
            Q.set_annealing(0.5)
            out['five_after_L'] = np.array(Q.compute_lowerbound())
            for nm in DIAG_NODES:
                out['five_after_%s_Lterm' % nm] = np.array(m[nm].lower_bound_contribution())
        out[tag + '_alpha_u0'] = np.array(m['alpha'].get_moments()[0])
        out[tag + '_Z_u0'] = np.array(m['Z'].get_moments()[0])
        for nm in ('mu', 'tau'):
            u = m[nm].get_moments()
            out['%s_%s_u0' % (tag, nm)] = np.array(u[0])
            out['%s_%s_u1' % (tag, nm)] = np.array(u[1])
        out[tag + '_plan'] = Q
    return out
