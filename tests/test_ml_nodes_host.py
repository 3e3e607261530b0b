"""CPU: the maximum-likelihood nodes GammaShape / Concentration (gamma.py:273-334,
dirichlet.py:234-330) -- constructors and argument checks, the C ABI declarations, the device
arithmetic (csrc/vmp_ml_dev.h, vmp_invpsi) built for the host against NumPy restatements of the
reference, the fused matchers declining, and the generic engine's host logic against the
live-reference fixtures (tests/golden/ml_nodes.npz) through the NumPy double of the entry points."""
import os
import warnings

import numpy as np
import pytest

import ml_host
from ml_host import concentration_fixed_point, host_concentration, host_invpsi, invpsi


# -- nodes ---------------------------------------------------------------------------------------
def test_exports_and_aliases():
    import bayespy_amd.nodes as N
    for name in ('GammaShape', 'Concentration', 'DirichletConcentration', 'BetaConcentration'):
        assert name in N.__all__ and hasattr(N, name)
    assert N.DirichletConcentration is N.Concentration
    c = N.BetaConcentration(name='c')
    assert isinstance(c, N.Concentration) and c.dims == ((2,), ()) and c.name == 'c'


def test_constructors_plates_and_regularization():
    import bayespy_amd.nodes as N
    a = N.GammaShape(plates=(3,), name='a')
    assert a.plates == (3,) and a.dims == ((), ())
    tau = N.Gamma(a, 1.0, plates=(5, 3))
    assert tau.plates == (5, 3)
    c = N.Concentration(4, plates=(2, 1))
    assert c.plates == (2, 1) and c.dims == ((4,), ())
    np.testing.assert_allclose(c.regularization[0], np.log(1 / 4))
    assert c.regularization[1] == 1
    assert list(N.Concentration(3, regularization=None).regularization) == [0, 0]
    assert list(N.Concentration(3, regularization=False).regularization) == [0, 0]
    p = N.Dirichlet(c, plates=(2, 7))
    assert p.plates == (2, 7) and p.dims == ((4,),)
    b = N.Beta(N.BetaConcentration(), plates=(6,))
    assert b.plates == (6,) and b.dims == ((2,),)
    with pytest.raises(ValueError, match='broadcast'):
        N.Dirichlet(c, plates=(3, 7))


def test_argument_errors_match_the_reference():
    import bayespy_amd.nodes as N
    c = N.Concentration(3)
    with pytest.raises(ValueError, match='Regularization must 2-tuple'):
        c.regularization = [0, 0, 0]
    with pytest.raises(ValueError, match='Wrong shape'):
        c.regularization = [np.zeros(4), 0]
    with pytest.raises(ValueError, match='Wrong shape'):
        N.Concentration(3, regularization=[0, np.ones(2)])
    with pytest.raises(ValueError, match='non-negative'):
        c.initialize_from_value([1.0, -1.0, 2.0])
    with pytest.raises(ValueError, match='Shape parameter must be positive'):
        N.GammaShape().initialize_from_value(0.0)
    with pytest.raises(NotImplementedError):
        N.GammaShape().observe(1.0)
    with pytest.raises(NotImplementedError):
        N.Concentration(2).random()


def test_new_symbols_are_declared_and_bound():
    from bayespy_amd import _lib
    declared = _lib.header_symbols()
    for name in ('vmp_ml_invpsi', 'vmp_ml_gamma_shape', 'vmp_ml_concentration'):
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)


# -- device arithmetic built for the host ----------------------------------------------------------
def test_invpsi_matches_the_reference_recipe():
    x = np.concatenate([np.linspace(-30, 12, 2001), [-2.22, -2.2200001, 0.0, np.nan]])
    y = host_invpsi(x)
    r = invpsi(x)
    ok = ~np.isnan(r)
    np.testing.assert_allclose(y[ok], r[ok], rtol=1e-13, atol=1e-300)
    assert np.isnan(y[-1])
    from scipy import special
    np.testing.assert_allclose(special.psi(y[ok & (x > -20)]), x[ok & (x > -20)], rtol=1e-9,
                               atol=1e-9)


@pytest.mark.parametrize('rows', [1, 7, 300])
def test_fixed_point_matches_the_reference_with_its_iteration_count(rows):
    rs = np.random.RandomState(rows)
    K = 4
    logp = np.log(rs.dirichlet(rs.gamma(2.0, 1.0, size=K), size=(rows, 20))).sum(axis=1)
    m1 = np.full(rows, 20.0)
    r0, r1 = np.full((rows, K), np.log(1 / K)), np.ones(rows)
    a, z, st = host_concentration(logp, m1, r0, r1)
    ar, it, capped = concentration_fixed_point(logp, m1, r0, r1)
    assert not capped and st[0] == 0 and st[1] == 0
    assert st[2] == it                       # the global stopping rule: same iteration
    np.testing.assert_allclose(a, ar, rtol=1e-12)
    from scipy import special
    np.testing.assert_allclose(z, special.gammaln(a.sum(-1)) - special.gammaln(a).sum(-1),
                               rtol=1e-12, atol=1e-12)


def test_rows_converge_at_different_iterations_and_stop_together():
    K = 3
    m0 = np.array([[-3.0, -3.1, -2.9], [-30.0, -1.0, -8.0]])
    one = concentration_fixed_point(m0[:1], np.ones(1), np.zeros((1, K)), np.ones(1))[1]
    both = concentration_fixed_point(m0, np.ones(2), np.zeros((2, K)), np.ones(2))[1]
    assert one != both
    _, _, st = host_concentration(m0, np.ones(2), np.zeros((2, K)), np.ones(2))
    assert st[2] == both


def test_fixed_point_nan_inf_and_cap():
    K = 3
    # NaN compares false: a row of NaN never keeps the loop going
    m0 = np.array([[np.nan, -1.0, -2.0]])
    a, _, st = host_concentration(m0, np.ones(1), np.zeros((1, K)), np.ones(1))
    ar, it, _ = concentration_fixed_point(m0, np.ones(1), np.zeros((1, K)), np.ones(1))
    assert st[2] == it and np.isnan(a[0, 0]) and np.isnan(ar[0, 0])
    # infinite mean_logp: the reference raises; the kernel reports and does not iterate
    m0 = np.array([[-np.inf, -1.0, -2.0]])
    with pytest.raises(ValueError, match='infs'):
        concentration_fixed_point(m0, np.ones(1), np.zeros((1, K)), np.ones(1))
    _, _, st = host_concentration(m0, np.ones(1), np.zeros((1, K)), np.ones(1))
    assert list(st) == [1, 0, 0]
    # the cap
    m0 = np.array([[-3.0, -3.1, -2.9]])
    _, _, st = host_concentration(m0, np.ones(1), np.zeros((1, K)), np.ones(1), max_iter=2)
    assert list(st) == [0, 1, 2]


# -- fused matchers ------------------------------------------------------------------------------
def test_fused_matchers_decline_node_valued_hyperparameters():
    import bayespy_amd.nodes as N
    from bayespy_amd.inference.plans.gmm import GMMPlan
    from bayespy_amd.inference.plans.pca import PCAPlan
    from bayespy_amd.inference.plans.masked_pca import MaskedPCAPlan
    from bayespy_amd.inference.plans.lssm import LSSMPlan
    # Gaussian mixture with a learnt assignment concentration
    c = N.Concentration(3, name='c')
    alpha = N.Dirichlet(c, name='alpha')
    z = N.Categorical(alpha, plates=(50,), name='z')
    mu = N.GaussianARD(0, 1e-3, shape=(2,), plates=(3,), name='mu')
    Lam = N.Wishart(2, np.identity(2), plates=(3,), name='Lambda')
    Y = N.Mixture(z, N.Gaussian, mu, Lam, plates=(50,), name='Y')
    Y.observe(np.zeros((50, 2)))
    why = []
    assert GMMPlan.match([Y, mu, Lam, z, alpha, c], why) is None
    assert any('concentration of the assignment prior is a node' in w for w in why)
    # PCA (and its missing-data block) with a learnt shape of the noise precision
    a = N.GammaShape(name='a')
    tau = N.Gamma(a, 1e-2, name='tau')
    al = N.Gamma(1e-2, 1e-2, plates=(2,), name='al')
    W = N.GaussianARD(0, al, shape=(2,), plates=(4, 1), name='W')
    X = N.GaussianARD(0, 1, shape=(2,), plates=(1, 9), name='X')
    F = N.SumMultiply('i,i', W, X, name='F')
    Yp = N.GaussianARD(F, tau, name='Y')
    Yp.observe(np.zeros((4, 9)))
    nodes = [Yp, F, W, X, tau, al, a]
    why = []
    assert PCAPlan.match(nodes, why) is None
    assert any('precision is not a Gamma node with constant parameters' in w for w in why)
    Yp.observe(np.zeros((4, 9)), mask=np.ones((4, 9), dtype=bool) & (np.arange(9) > 0))
    why = []
    assert MaskedPCAPlan.match(nodes, why) is None
    assert any('constant parameters' in w for w in why)
    # state-space model with a learnt shape of the noise precision
    from bayespy_amd.nodes import GaussianMarkovChain
    D, T = 2, 6
    A = N.GaussianARD(0, N.Gamma(1e-5, 1e-5, plates=(D,)), shape=(D,), plates=(D,), name='A')
    Xc = GaussianMarkovChain(np.zeros(D), np.identity(D), A, np.ones(D), n=T, name='X')
    C = N.GaussianARD(0, N.Gamma(1e-5, 1e-5, plates=(D,)), shape=(D,), plates=(3, 1), name='C')
    Fs = N.SumMultiply('i,i', C, Xc, name='F')
    a2 = N.GammaShape(name='a2')
    tau2 = N.Gamma(a2, 1e-5, name='tau')
    Ys = N.GaussianARD(Fs, tau2, name='Y')
    Ys.observe(np.zeros((3, T)))
    why = []
    assert LSSMPlan.match([Ys, Fs, C, Xc, A, tau2, a2], why) is None
    assert any('node-valued hyperparameter' in w for w in why)


def test_sharded_models_with_ml_nodes_are_refused():
    import bayespy_amd.nodes as N
    from bayespy_amd.inference.plans.generic import GenericPlan
    ml_host.install()
    try:
        c = N.Concentration(3, name='c')
        p = N.Dirichlet(c, plates=(4,), name='p')
        p.shard(0)
        with pytest.raises(NotImplementedError, match='sharded'):
            GenericPlan([p, c])
    finally:
        from host_generic import uninstall
        uninstall()


# -- the generic engine on the host against the live-reference fixtures -----------------------------
@pytest.mark.parametrize('tag', ['gs', 'gp', 'cc', 'cn', 'cu', 'cp', 'bc'])
def test_models_through_the_host_double_match_reference(golden_dir, tag):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    from ml_models import run_ml_cases
    f = np.load(os.path.join(golden_dir, 'ml_nodes.npz'))
    g = {k[3:]: f[k] for k in f.files if k.startswith('in_')}
    rt = ml_host.install()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = run_ml_cases(N_, VB, g, only=[tag])
    finally:
        from host_generic import uninstall
        uninstall()
    assert rt.lib.calls.get('vmp_ml_gamma_shape', 0) + rt.lib.calls.get('vmp_ml_concentration', 0)
    np.testing.assert_allclose(res[tag + '_L'], f[tag + '_L'], rtol=1e-9)
    for k, v in res.items():
        if isinstance(v, list):
            for i, vi in enumerate(v):
                np.testing.assert_allclose(vi, f['%s_%d' % (k, i)], rtol=1e-7, atol=1e-12)


def _concentration_model():
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    rs = np.random.RandomState(7)
    c = N_.Concentration(3, name='c')
    p = N_.Dirichlet(c, plates=(5, 1), name='p')
    z = N_.Categorical(p, plates=(5, 40), name='z')
    z.observe(rs.randint(3, size=(5, 40)))
    a = N_.GammaShape(name='a')
    tau = N_.Gamma(a, 2.0, plates=(30,), name='tau')
    tau.observe(rs.gamma(3.0, 0.5, size=30))
    Q = VB(z, p, c, tau, a)
    Q.ignore_bound_checks = True
    return Q, c, a


def test_distribution_operations_on_ml_nodes_raise_not_implemented():
    ml_host.install()
    try:
        Q, c, a = _concentration_model()
        Q.update(repeat=2, verbose=False)
        for node in (c, a):
            with pytest.raises(NotImplementedError, match='gradient step'):
                Q.gradient_step(node)
            with pytest.raises(NotImplementedError, match='maximum-likelihood'):
                node.get_parameters()
            with pytest.raises(NotImplementedError, match='maximum-likelihood'):
                node.set_parameters([np.ones(node.dims[0])])
            with pytest.raises(NotImplementedError, match='maximum-likelihood'):
                node.get_riemannian_gradient()
            with pytest.raises(NotImplementedError, match='maximum-likelihood'):
                node.logpdf(np.ones(node.dims[0]))
            with pytest.raises(NotImplementedError, match='maximum-likelihood'):
                node.random()
            with pytest.raises(NotImplementedError, match='maximum-likelihood'):
                node.initialize_from_random()
    finally:
        from host_generic import uninstall
        uninstall()


def test_new_regularization_keeps_the_estimate():
    """As in the reference, setting the regularization leaves u as it is; the bound term and the
    next update read the new value."""
    ml_host.install()
    try:
        Q, c, _ = _concentration_model()
        Q.update(repeat=2, verbose=False)
        u = [np.array(v) for v in c.u]
        reg = [np.log(np.array([0.2, 0.3, 0.5])), 4.0]
        c.regularization = reg
        for x, y in zip(c.u, u):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_allclose(c.lower_bound_contribution(),
                                   np.sum(u[0] * reg[0]) + u[1] * reg[1], rtol=1e-12)
        Q.update(repeat=1, verbose=False)
        assert not np.array_equal(c.u[0], u[0])
    finally:
        from host_generic import uninstall
        uninstall()


def test_state_space_reason_only_for_state_space_models():
    import bayespy_amd.nodes as N
    from bayespy_amd.inference.plans.lssm import LSSMPlan
    b = N.Gamma(1e-2, 1e-2, name='b')
    tau = N.Gamma(2.0, b, name='tau')
    W = N.GaussianARD(0, 1, shape=(2,), plates=(4, 1), name='W')
    X = N.GaussianARD(0, 1, shape=(2,), plates=(1, 9), name='X')
    Y = N.GaussianARD(N.SumMultiply('i,i', W, X), tau, name='Y')
    Y.observe(np.zeros((4, 9)))
    why = []
    assert LSSMPlan.match([Y, W, X, tau, b], why) is None
    assert not why
