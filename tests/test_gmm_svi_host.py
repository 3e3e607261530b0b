"""CPU: the fused Gaussian-mixture block under stochastic variational inference (GMMSVIPlan) on the
kernel double tests/gmm_svi_host.py -- matcher and registration, decline reasons, the traces of the
live reference (tests/golden/gmm_svi.npz, tests/golden/svi_gmm.npz), re-observation, the multiplier's
setter, checkpoints, the C ABI."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gmm_svi_models as M          # noqa: E402
import gmm_svi_host                 # noqa: E402


def _mods():
    import bayespy_amd.nodes
    from bayespy_amd.inference import VB
    return dict(nodes=bayespy_amd.nodes, VB=VB, vb_kwargs=dict(engine='fused'),
                after_vb=gmm_svi_host.attach)


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(GOLDEN, 'gmm_svi.npz')))


def _old_trace_model(g, **vb):
    from bayespy_amd.nodes import GaussianARD, Gaussian, Dirichlet, Categorical, Mixture
    from bayespy_amd.inference import VB
    N, NB = int(g['N']), int(g['NB'])
    K, D = g['mu0'].shape
    mu = GaussianARD(0, 0.001, shape=(D,), plates=(K,), name='means')
    alpha = Dirichlet(np.ones(K), name='class probabilities')
    Z = Categorical(alpha, plates=(NB,), plates_multiplier=(N / NB,), name='classes')
    Y = Mixture(Z, Gaussian, mu, np.identity(D), name='observations')
    mu.initialize_from_value(g['mu0'])
    Q = VB(Y, Z, mu, alpha, **vb)
    Q.ignore_bound_checks = True
    return Q, Y, Z, mu, alpha


@pytest.mark.parametrize('tag', M.CASES)
def test_matcher_accepts_fixture_cases_and_block_declines(golden, tag):
    from bayespy_amd.inference.plans import GMMPlan, GMMSVIPlan
    import bayespy_amd.nodes
    m = M.build(dict(nodes=bayespy_amd.nodes), golden, tag)
    nodes = list(m.values())
    assert GMMPlan.match(nodes) is None
    roles = GMMSVIPlan.match(nodes)
    assert roles is not None and roles['Y'] is m['Y'] and roles['z'] is m['Z']
    assert ('Lambda' in roles) == ('Lambda' in m)


def test_matcher_accepts_the_generic_engines_trace_model():
    from bayespy_amd.inference.plans import GMMPlan, GMMSVIPlan
    from bayespy_amd.inference.plans.generic import GenericPlan
    g = np.load(os.path.join(GOLDEN, 'svi_gmm.npz'))
    Q, Y, Z, mu, alpha = _old_trace_model(g)
    # without engine='fused' the model runs on the generic engine as before
    assert isinstance(Q.plans[0], GenericPlan)
    assert GMMPlan.match([Y, Z, mu, alpha]) is None
    assert GMMSVIPlan.match([Y, Z, mu, alpha]) is not None
    Q2, *_ = _old_trace_model(g, engine='fused')
    assert type(Q2.plans[0]).__name__ == 'GMMSVIPlan'


def test_plain_mixture_stays_on_the_block_and_lists_are_pinned():
    from bayespy_amd.nodes import GaussianARD, Gaussian, Wishart, Dirichlet, Categorical, Mixture
    from bayespy_amd.inference import VB
    from bayespy_amd.inference import plans as P
    N, D, K = 20, 2, 3
    alpha = Dirichlet(np.ones(K), name='alpha')
    z = Categorical(alpha, plates=(N,), name='z')
    mu = GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
    Lam = Wishart(D, np.identity(D), plates=(K,), name='Lambda')
    Y = Mixture(z, Gaussian, mu, Lam, name='Y')
    Q = VB(Y, mu, Lam, z, alpha, engine='fused')
    assert type(Q.plans[0]).__name__ == 'GMMPlan'
    names = lambda ts: [t.__name__ for t in ts]          # noqa: E731
    assert names(P.PLAN_TYPES) == ['PCAPlan', 'MaskedPCAPlan', 'GMMPlan', 'LSSMPlan',
                                   'MaskedLSSMPlan', 'LDAPlan']
    assert names(P.OPT_IN_TYPES) == ['BernoulliMixturePlan', 'HMMPlan']
    assert {k.__name__: names(v) for k, v in P.OPT_IN_EMISSIONS.items()} == \
        {'HMMPlan': ['CategoricalHMMPlan']}
    assert names(P.opt_in_types()) == ['BernoulliMixturePlan', 'HMMPlan', 'CategoricalHMMPlan']
    assert {k.__name__: v.__name__ for k, v in P.OPT_IN_FORMS.items()} == {'LDAPlan': 'LDASVIPlan'}
    assert {k.__name__: names(v) for k, v in P.OPT_IN_AFTER.items()} == {'GMMPlan': ['GMMSVIPlan']}


def _declined(build):
    from bayespy_amd.inference.plans import GMMSVIPlan
    why = []
    assert GMMSVIPlan.match(build(), why) is None
    return why


def _model(D=2, K=3, N=10, m=5.0, mean=None, prec=None, lam=None, mu_mult=None, shard=False,
           mask=None):
    from bayespy_amd.nodes import Gaussian, Dirichlet, Categorical, Mixture
    alpha = Dirichlet(np.ones(K), name='alpha')
    z = Categorical(alpha, plates=(N,), plates_multiplier=(m,), name='z')
    mu = Gaussian(np.zeros(D) if mean is None else mean, np.identity(D) if prec is None else prec,
                  plates=(K,), plates_multiplier=mu_mult, name='mu')
    Y = Mixture(z, Gaussian, mu, np.identity(D) if lam is None else lam, name='Y')
    if shard:
        z.shard(-1)
    if mask is not None:
        Y.observe(np.zeros((N, D)), mask=mask)
    return [Y, z, mu, alpha]


@pytest.mark.parametrize('kwargs, words', [
    (dict(prec=np.diag([1.0, 2.0])), 'not a scalar multiple of the identity'),
    (dict(mean=np.array([0.0, 1.0])), 'prior mean of the means is not zero'),
    (dict(mu_mult=(2.0,), m=1.0), 'a global node (mu, Lambda or alpha) carries a plates_multiplier'),
    (dict(shard=True), 'sharded'),
    (dict(mask=np.arange(10) % 2 == 0), 'missing values'),
    (dict(lam=np.array([[1.0, 2.0], [2.0, 1.0]])), 'not symmetric positive definite'),
])
def test_decline_reasons(kwargs, words):
    why = _declined(lambda: _model(**kwargs))
    assert len(why) == 1 and words in why[0], why


@pytest.mark.parametrize('tag', M.CASES)
def test_fixture_traces(golden, tag):
    res = M.run_case(_mods(), golden, tag)
    assert type(res[tag + '_plan'].plans[0]).__name__ == 'GMMSVIPlan'
    M.check_case(res, golden, tag)


def test_generic_engines_trace_on_the_block():
    g = np.load(os.path.join(GOLDEN, 'svi_gmm.npz'))
    Q, Y, Z, mu, alpha = _old_trace_model(g, engine='fused')
    gmm_svi_host.attach(Q)
    data, batches = g['data'], g['batches']
    for n in range(len(batches)):
        Y.observe(data[batches[n], :])
        Q.update(Z, verbose=False)
        Q.gradient_step(mu, alpha, scale=(n + 1) ** (-0.7))
        np.testing.assert_allclose(Q.compute_lowerbound(), g['L'][n], rtol=1e-9)
        np.testing.assert_allclose(mu.u[0], g['mu_u0'][n], rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(alpha.u[0], g['alpha_u0'][n], rtol=1e-7)
    np.testing.assert_allclose(Z.u[0], g['Z_u0_last'], rtol=1e-7, atol=1e-12)
    terms = [Y.lower_bound_contribution(), Z.lower_bound_contribution(),
             mu.lower_bound_contribution(), alpha.lower_bound_contribution()]
    np.testing.assert_allclose(terms, g['L_terms_last'], rtol=1e-9, atol=1e-9)


def test_reobservation_keeps_the_state(golden):
    seen = []

    def on_step(Q, m, n):
        p = Q.plans[0]
        seen.append((id(p.state), id(p.phi_mu), p.kernels.calls.count('init_state')))
    with warnings.catch_warnings():
        warnings.simplefilter('error')          # no 'state discarded' warning either
        res = M.run_case(_mods(), golden, 'wishart_d3', on_step=on_step)
    assert len(set(seen)) == 1 and seen[0][2] == 1
    calls = res['wishart_d3_plan'].plans[0].kernels.calls
    assert calls.count('natural_init') == 1 and calls.count('natural_step:7') == 6


def test_one_array_filled_again_keeps_the_state(golden):
    """The loop that keeps ONE batch array and fills it in place: the same object is observed at
    every step.  The state stays (one init_state, the same state tensor) and the trace is the
    reference's."""
    buf, seen = {}, []

    def observe(Y, rows, n):
        if 'a' not in buf:
            buf['a'] = np.empty_like(rows)
        buf['a'][:] = rows
        Y.observe(buf['a'])

    def on_step(Q, m, n):
        p = Q.plans[0]
        seen.append((id(p.state), id(p.phi_mu), p.kernels.calls.count('init_state'),
                     p.kernels.calls.count('natural_init')))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = M.run_case(_mods(), golden, 'wishart_d3', observe=observe, on_step=on_step)
    assert len(set(seen)) == 1 and seen[0][2:] == (1, 1)
    M.check_case(res, golden, 'wishart_d3')


def test_unchanged_multiplier_written_again_changes_nothing(golden):
    def on_step(Q, m, n):
        p = Q.plans[0]
        state, version = p.state, p._version
        m['Z'].plates_multiplier = tuple(m['Z'].plates_multiplier)
        m['Y'].plates_multiplier = None              # Y keeps inheriting the factor of Z
        assert p._ready and p.state is state and p._version <= version + 1
        assert p.kernels.calls.count('init_state') == 1
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = M.run_case(_mods(), golden, 'demo', on_step=on_step)
    M.check_case(res, golden, 'demo')


def test_random_initialisation_is_the_generic_engines_draw(golden):
    """mu.initialize_from_random(): a draw from the prior with the host generator, formed as
    GenericPlan._sample forms it; a point mass (Cov = 0, bound -inf) until the first step."""
    import torch
    from bayespy_amd.inference.plans.generic import GenericPlan
    m_ = _mods()
    m = M.build(m_, golden, 'const_kdd')             # Gaussian(0, 0.01 I) means
    K, D = golden['const_kdd_mu0'].shape
    m['mu'].initialize_from_random()
    Q = m_['VB'](m['Y'], m['Z'], m['mu'], m['alpha'], engine='fused')
    Q.ignore_bound_checks = True
    gmm_svi_host.attach(Q)
    m['Y'].observe(golden['const_kdd_data'].astype(np.float64)[golden['const_kdd_batches'][0]])
    np.random.seed(77)
    Q.update(m['Z'], verbose=False)
    np.random.seed(77)
    prior = [torch.zeros(K, D, dtype=torch.float64),
             torch.from_numpy(np.broadcast_to(np.identity(D) / 0.01, (K, D, D)).copy())]
    want = GenericPlan._sample(None, m['mu'], None, prior)
    got = m['mu'].u
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], want[:, :, None] * want[:, None, :])
    assert np.abs(want).max() > 1.0                  # a draw of spread 10, not the prior mean
    assert Q.compute_lowerbound() == -np.inf
    assert m['mu'].lower_bound_contribution() == -np.inf
    Q.gradient_step(m['mu'], m['alpha'], scale=0.5)
    assert np.isfinite(Q.compute_lowerbound())


def test_point_mass_until_the_first_step(golden):
    m_ = _mods()
    m = M.build(m_, golden, 'demo')
    Q = m_['VB'](m['Y'], m['Z'], m['mu'], m['alpha'], engine='fused')
    Q.ignore_bound_checks = True
    gmm_svi_host.attach(Q)
    data = golden['demo_data'].astype(np.float64)
    m['Y'].observe(data[golden['demo_batches'][0]])
    Q.update(m['Z'], verbose=False)
    np.testing.assert_array_equal(m['mu'].u[0], golden['demo_mu0'])
    np.testing.assert_array_equal(
        m['mu'].u[1], golden['demo_mu0'][:, :, None] * golden['demo_mu0'][:, None, :])
    assert Q.compute_lowerbound() == -np.inf
    Q.gradient_step(m['mu'], scale=0.5)
    assert np.isfinite(Q.compute_lowerbound())


def test_changed_multiplier_is_honoured(golden):
    m_ = _mods()
    g = golden
    runs = []
    for change in (False, True):
        m = M.build(m_, g, 'wishart_d3')
        Q = m_['VB'](m['Y'], m['Z'], m['mu'], m['alpha'], m['Lambda'], engine='fused')
        Q.ignore_bound_checks = True
        gmm_svi_host.attach(Q)
        data = g['wishart_d3_data'].astype(np.float64)
        m['Y'].observe(data[g['wishart_d3_batches'][0]])
        Q.update(m['Z'], verbose=False)
        state = Q.plans[0].state
        if change:
            m['Z'].plates_multiplier = (3.0,)
            assert Q.plans[0].state is state and Q.plans[0]._ready
        Q.gradient_step(m['mu'], m['Lambda'], m['alpha'], scale=1.0)
        runs.append((m['alpha'].u[0].copy(), Q.plans[0]._blk(Q.plans[0].layout.off_alpha, (5,)),
                     Q.plans[0].statistics()[0], Q.compute_lowerbound()))
    (_, a10, R, L10), (_, a3, _, L3) = runs
    np.testing.assert_allclose(a10, 1.0 + 10.0 * R, rtol=1e-14)
    np.testing.assert_allclose(a3, 1.0 + 3.0 * R, rtol=1e-14)
    assert L10 != L3


def test_gradient_step_of_z_raises(golden):
    m_ = _mods()
    m = M.build(m_, golden, 'demo')
    Q = m_['VB'](m['Y'], m['Z'], m['mu'], m['alpha'], engine='fused')
    gmm_svi_host.attach(Q)
    m['Y'].observe(golden['demo_data'][golden['demo_batches'][0]].astype(np.float64))
    with pytest.raises(NotImplementedError, match='keeps no natural parameters'):
        Q.gradient_step(m['Z'], scale=0.5)


def test_checkpoint_round_trip_and_kinds(golden, tmp_path):
    tag = 'wishart_d3'
    fn = str(tmp_path / 'svi.bin')
    data, batches = golden[tag + '_data'].astype(np.float64), golden[tag + '_batches']

    def start():
        m_ = _mods()
        m = M.build(m_, golden, tag)
        Q = m_['VB'](m['Y'], m['Z'], m['mu'], m['alpha'], m['Lambda'], engine='fused')
        Q.ignore_bound_checks = True
        gmm_svi_host.attach(Q)
        return Q, m

    def steps(Q, m, which):
        out = []
        for n in which:
            m['Y'].observe(data[batches[n]])
            Q.update(m['Z'], verbose=False)
            Q.gradient_step(m['mu'], m['Lambda'], m['alpha'], scale=(n + 1) ** (-0.7))
            out.append((Q.compute_lowerbound(), m['mu'].u[0], m['Lambda'].u[0], m['alpha'].u[0]))
        return out
    Q, m = start()
    steps(Q, m, range(3))
    Q.save(filename=fn)
    want = steps(Q, m, range(3, 5))
    Q2, m2 = start()
    m2['Y'].observe(data[batches[2]])
    Q2.load(filename=fn)
    got = steps(Q2, m2, range(3, 5))
    for a, b in zip(want, got):
        assert a[0] == b[0]
        for x, y in zip(a[1:], b[1:]):
            np.testing.assert_array_equal(x, y)
    # a checkpoint of the other form of the block is refused, both ways
    from test_gmm_plan_host import _build
    gg = np.load(os.path.join(GOLDEN, 'gmm_n400_d3_k4.npz'))
    Qp = _build(gg['y'], gg['lab0'], 4)
    with pytest.raises(ValueError, match="kind 'gmm_svi'"):
        Qp.plans[0].load_state(_reader(fn), Qp.model, 0)
    fp = str(tmp_path / 'plain.bin')
    Qp.update(repeat=1, verbose=False)
    Qp.save(filename=fp)
    with pytest.raises(ValueError, match="kind 'gmm'"):
        Q2.plans[0].load_state(_reader(fp), Q2.model, 0)


def _reader(fn):
    from bayespy_amd.inference import checkpoint
    return checkpoint.Reader(fn)


def test_c_abi_exports_the_step():
    from bayespy_amd import _lib
    assert 'vmp_gmm_natural_step' in _lib.header_symbols()
    assert 'vmp_gmm_natural_init' in _lib.header_symbols()
    lib = _lib.load()
    assert hasattr(lib, 'vmp_gmm_natural_step') and hasattr(lib, 'vmp_gmm_natural_init')
