"""CPU: the fused Poisson-mixture block without a device -- the matcher and its declining reasons
one by one, the new opt-in registry beside the unchanged old ones, the plan's host logic on the
kernel double tests/pmm_host.py (CPUPMMKernels) against every fixture of tests/golden/pmm.npz (live
reference, tools/make_golden_pmm.py), masks, the g++ build of the device header csrc/vmp_pmm_dev.h
against a long-double restatement, the same source under -fsanitize=address,undefined as a
stand-alone program, a save / load round trip and the C ABI."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

L_RTOL = 1e-9
MOM_TOL = dict(rtol=1e-6, atol=1e-9)
PER_CASE = 1 + 4 + 4 + 2                    # L, four bound terms, four moments, two masks


def _mods(after=None, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    m = dict(nodes=nodes, VB=VB, vb_kwargs=kw)
    if after is not None:
        m['after_vb'] = after
    return m


def _on_double(Q):
    from bayespy_amd.device import Runtime
    from pmm_host import CPUPMMKernels
    plan = Q.plans[0]
    assert type(plan).__name__ == 'PoissonMixturePlan'
    rt = Runtime(device='cpu')
    plan._rt, plan._kernels = rt, CPUPMMKernels(rt)


def _golden():
    g = np.load(os.path.join(GOLDEN, 'pmm.npz'))
    gin = {k[3:]: (g[k].astype(np.int64) if k.endswith('_x') else g[k])
           for k in g.files if k.startswith('in_')}
    return g, gin


def _model(tag='d', **kw):
    from pmm_models import build_pmm
    gin = _golden()[1]
    return build_pmm(_mods(), gin[tag + '_x'], gin[tag + '_lam0'].shape[1], **kw)


def _nodes(m):
    return [m['Z'], m['R'], m['X'], m['lam']]


def check_fixture(res, g, cases):
    """Every stored quantity of the cases; returns how many were compared."""
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan') or k[0] not in cases:
            continue
        if k.endswith('_mask'):
            np.testing.assert_array_equal(np.broadcast_to(v, g[k].shape), g[k], err_msg=k)
        elif k.endswith(('_u0', '_u1')):
            np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL, atol=1e-9)
        checked += 1
    return checked


# -- the matcher and the registration ----------------------------------------------------------------
def test_matcher_accepts_the_model():
    from bayespy_amd.inference.plans.pmm import PoissonMixturePlan
    gin = _golden()[1]
    for observe in (True, False):
        m = _model(observe=observe)
        why = []
        r = PoissonMixturePlan.match(_nodes(m), why)
        assert r is not None and why == []
        assert r['X'] is m['X'] and r['lam'] is m['lam'] and r['Z'] is m['Z'] and r['R'] is m['R']
    # constants of any shape that broadcasts, a mask of the full shape, the accepted initialisations
    m = _model('a', a0=gin['a_a0'][:, :1], b0=gin['a_b0'][0], alpha=gin['a_alpha'],
               mask=gin['f_mask'])
    assert PoissonMixturePlan.match(_nodes(m)) is not None
    m['lam'].initialize_from_value(gin['a_lam0'])
    m['Z'].initialize_from_value(gin['a_z0'])
    assert PoissonMixturePlan.match(_nodes(m)) is not None
    m['lam'].initialize_from_parameters(gin['a_a0'], gin['a_b0'])
    assert PoissonMixturePlan.match(_nodes(m)) is not None


def test_matcher_declines_with_reasons():
    from bayespy_amd import nodes
    from bayespy_amd.inference.plans.pmm import PoissonMixturePlan, pmm_limits
    x = _golden()[1]['c_x']
    N, D = x.shape

    def reason(m):
        why = []
        assert PoissonMixturePlan.match(_nodes(m), why) is None and len(why) == 1, why
        assert why[0].startswith('fused Poisson-mixture block, observed node X: ')
        return why[0]

    def silent(ns):
        why = []
        assert PoissonMixturePlan.match(ns, why) is None and why == [], why

    def build(K=2, D=D, N=N, lam=None, R=None, Zkw={}, Xkw={}):
        if R is None:
            R = nodes.Dirichlet(K * [1.0], name='R')
        Z = nodes.Categorical(R, plates=(N, 1), name='Z', **Zkw)
        if lam is None:
            lam = nodes.Gamma(1.0, 1.0, plates=(D, K), name='lam')
        X = nodes.Mixture(Z, nodes.Poisson, lam, name='X', **Xkw)
        return dict(R=R, Z=Z, lam=lam, X=X)
    # a mask that broadcasts over a plate, a scalar mask
    m = build()
    m['X'].observe(x, mask=(np.arange(N) % 2 == 0)[:, None])
    assert 'mask of shape (%d, 1)' % N in reason(m)
    m = build()
    m['X'].observe(x, mask=False)
    assert 'mask of shape ()' in reason(m)
    # plates_multiplier
    assert 'plates_multiplier' in reason(build(Zkw=dict(plates_multiplier=(2.5, 1))))
    # sharded plates
    m = build()
    m['Z']._shard_axis = 0
    assert 'sharded' in reason(m)
    # a node as a prior parameter, of lam and of R
    b = nodes.Gamma(1.0, 1.0, name='b')
    assert 'a parameter of lam is a node (Gamma)' in reason(
        build(lam=nodes.Gamma(1.0, b, plates=(D, 2), name='lam')))
    c = nodes.Concentration(2, name='c')
    assert 'a parameter of R is a node (Concentration)' in reason(
        build(R=nodes.Dirichlet(c, name='R')))
    # other plates, cluster_plate
    assert 'plates' in reason(build(lam=nodes.Gamma(1.0, 1.0, plates=(1, D, 2), name='lam')))
    assert 'cluster_plate' in reason(build(lam=nodes.Gamma(1.0, 1.0, plates=(2, D), name='lam'),
                                           Xkw=dict(cluster_plate=-2)))
    # other children
    m = build()
    nodes.Poisson(m['lam'], name='another')
    assert 'other children' in reason(m)
    # observed roles, other initialisations
    m = build()
    m['R'].observe(np.array([0.5, 0.5]))
    assert 'observed' in reason(m)
    m = build()
    m['R'].initialize_from_value(np.array([0.5, 0.5]))
    assert 'R is initialised by value' in reason(m)
    m = build()
    m['Z'].initialize_from_random()
    assert 'Z is initialised by random' in reason(m)
    m = build()
    m['lam'].initialize_from_random()
    assert 'lam is initialised by random' in reason(m)
    # K, D and a count above the limits; the reason states the cap
    assert pmm_limits() == (64, 1024, 65534)
    assert 'K <= 64' in reason(build(K=65))
    assert 'D <= 1024' in reason(build(D=1025, N=2))
    m = build()
    big = x.copy()
    big[3, 0] = 65535
    m['X'].observe(big)
    r = reason(m)
    assert 'a count of 65535 exceeds' in r and 'at most 65534' in r
    big[3, 0] = 65534
    m = build()
    m['X'].observe(big)
    assert PoissonMixturePlan.match(_nodes(m)) is not None
    # another family, and a hidden Markov model: nothing is said
    Rn = nodes.Dirichlet([1.0, 1.0], name='R')
    Zn = nodes.Categorical(Rn, plates=(N, 1), name='Z')
    Pn = nodes.Beta([0.5, 0.5], plates=(D, 2), name='P')
    silent([Zn, Rn, nodes.Mixture(Zn, nodes.Bernoulli, Pn, name='X'), Pn])
    a0 = nodes.Dirichlet([1.0, 1.0], name='a0')
    A = nodes.Dirichlet([1.0, 1.0], plates=(2,), name='A')
    Zc = nodes.CategoricalMarkovChain(a0, A, states=9, name='Z')
    lh = nodes.Gamma(1.0, 1.0, plates=(2,), name='lam')
    silent([Zc, a0, A, nodes.Mixture(Zc, nodes.Poisson, lh, name='Y'), lh])


def test_the_new_registry_and_the_old_ones():
    from bayespy_amd.inference import plans
    names = lambda ps: [P.__name__ for P in ps]       # noqa: E731
    assert names(plans.OPT_IN_COUNTS) == ['PoissonMixturePlan']
    assert names(plans.OPT_IN_LAST) == ['CategoricalMixturePlan']
    assert names(plans.PLAN_TYPES) == ['PCAPlan', 'MaskedPCAPlan', 'GMMPlan', 'LSSMPlan',
                                       'MaskedLSSMPlan', 'LDAPlan']
    assert names(plans.OPT_IN_TYPES) == ['BernoulliMixturePlan', 'HMMPlan']
    assert names(plans.OPT_IN_MORE) == ['DiagGaussianMixturePlan']


def test_default_engine_keeps_the_generic_plan():
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.plans.pmm import PoissonMixturePlan
    import host_generic
    m = _model()
    host_generic.install()          # the generic engine on the NumPy double of its entry points
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            got = compile_model(_nodes(m))
        assert len(got) == 1 and isinstance(got[0], GenericPlan)
        # the opt-in form is kept only where it is asked for
        fused = compile_model(_nodes(m), engine='fused')
        assert isinstance(fused[0], PoissonMixturePlan)
        assert compile_model(_nodes(m), engine='fused')[0] is fused[0]
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            again = compile_model(_nodes(m))
        assert isinstance(again[0], GenericPlan)
    finally:
        host_generic.uninstall()


def test_engine_fused_builds_the_block_and_declined_models_raise():
    """Fails without the feature: engine='fused' finds no block for the model."""
    from bayespy_amd.inference import VB
    m = _model()
    Q = VB(*_nodes(m), engine='fused')
    assert type(Q.plans[0]).__name__ == 'PoissonMixturePlan'
    m = _model()
    m['X'].observe(_golden()[1]['d_x'], mask=False)
    with pytest.raises(NotImplementedError, match='fused Poisson-mixture block.*mask'):
        VB(*_nodes(m), engine='fused')
    assert all(n._plan is None for n in _nodes(m))


# -- the plan on the kernel double ---------------------------------------------------------------------
def test_plan_reproduces_every_fixture_on_the_kernel_double():
    from pmm_models import run_pmm_cases, CASES
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_pmm_cases(_mods(_on_double, engine='fused'), gin)
    assert check_fixture(res, g, CASES) == len(CASES) * PER_CASE
    calls = res['a_plan'].plans[0].kernels.calls
    # set-up pass + one per sweep; the responsibilities only on request
    assert calls.count('pass') == 1 + 4 and calls.count('pass_r') == 1 and calls.count('pack') == 1
    assert calls.count('update') == 1 + 4 and 'update_M' not in calls
    # a mask of ones: the form without hidden entries and the bits of the unmasked run
    assert res['g_plan'].plans[0].kernels.calls == calls
    for k in ('L', 'Z_u0', 'lam_u0', 'lam_u1', 'R_u0', 'Z_Lterm', 'lam_Lterm', 'X_Lterm'):
        np.testing.assert_array_equal(res['g_' + k], res['a_' + k], err_msg=k)
    # (f): the hidden form; the row of nothing has softmax(c), its column of lam stays at the prior
    plan = res['f_plan'].plans[0]
    assert plan.hidden == 1 and 'pass_hidden' in plan.kernels.calls
    c = plan.c.numpy()                    # of the last Z update, which R's update followed
    np.testing.assert_allclose(res['f_Z_u0'][4, 0], np.exp(c) / np.exp(c).sum(), rtol=1e-12)
    assert np.all(plan.S.numpy()[2] == 0) and np.all(plan.M.numpy()[2] == 0)
    par = plan.lam_par.numpy().reshape(7, 3, 2)
    np.testing.assert_array_equal(par[2, :, 0], gin['a_a0'][2])
    np.testing.assert_array_equal(par[2, :, 1], gin['a_b0'][2])
    # (e): the column of zeros and the large counts
    assert np.all(res['e_plan'].plans[0].S.numpy()[0] == 0)


def test_a_column_at_its_prior_has_a_bound_term_of_exactly_zero():
    from pmm_host import host_update
    rs = np.random.RandomState(5)
    D, K = 6, 3
    a0, b0 = rs.gamma(2.0, size=(D, K)), rs.gamma(2.0, size=(D, K))
    S, M = rs.gamma(3.0, size=(D, K)), rs.gamma(3.0, size=(D, K))
    assert host_update(D, K, 1, a0, b0, None, None)[2] == 0.0
    assert host_update(D, K, 1, a0, b0, 0 * S, 0 * M)[2] == 0.0
    S[1:], M[1:] = 0, 0
    one = host_update(1, K, 1, a0[:1], b0[:1], S[:1], M[:1])[2]
    assert host_update(D, K, 1, a0, b0, S, M)[2] == one and one != 0.0


def test_hidden_values_are_never_interpreted_and_reobserving_keeps_the_posteriors():
    from pmm_models import run_pmm_cases
    g, gin = _golden()
    Q = run_pmm_cases(_mods(_on_double, engine='fused'), gin, only=('f',))['f_plan']
    plan = Q.plans[0]
    X, lam = Q['X'], Q['lam']
    u = lam.get_moments()[0]
    S0, xp0 = plan.S.numpy().copy(), plan.xp.numpy().copy()
    mask = gin['f_mask']
    junk = np.where(mask, gin['a_x'], np.nan).astype(np.float64)
    junk[~mask] = np.resize([np.nan, -1.0, 1e300], int((~mask).sum()))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        X._data, X._mask = junk, mask           # past the host check of observe, as a tensor is
        plan.invalidate(X)
        np.testing.assert_array_equal(lam.get_moments()[0], u)
    assert Q.plans[0] is plan
    np.testing.assert_array_equal(plan.xp.numpy(), xp0)
    np.testing.assert_array_equal(plan.S.numpy(), S0)
    # another mask of the full shape: packed again, the posteriors stay
    m2 = mask.copy()
    m2[4] = True
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        X.observe(gin['a_x'], mask=m2)
        np.testing.assert_array_equal(lam.get_moments()[0], u)
    assert Q.plans[0] is plan and plan.kernels.calls.count('pack') == 3
    assert bool(Q['Z'].mask[4, 0]) is True
    # no mask at all: the other form of the pass, with the tables of the last Z update formed again
    X.observe(gin['a_x'])
    np.testing.assert_array_equal(lam.get_moments()[0], u)
    assert plan.hidden == 0 and plan.kernels.calls[-1] == 'pass'
    ref = run_pmm_cases(_mods(_on_double, engine='fused'), gin, only=('a',), n_iter=1)['a_plan']
    Q.update(repeat=1, verbose=False)
    assert np.isfinite(Q.L[4]) and ref.plans[0].hidden == 0


def test_invalid_counts_raise_the_reference_exceptions_and_the_cap_is_named():
    from bayespy_amd.inference import VB
    _, gin = _golden()
    for bad, exc, text in ((0.5, ValueError, 'Values must be integers'),
                           (np.nan, ValueError, 'Values must be integers'),
                           (-1.0, ValueError, 'Values must be positive'),
                           (65535.0, NotImplementedError, 'fused Poisson-mixture block.*65534')):
        m = _model()
        Q = VB(*_nodes(m), engine='fused')
        _on_double(Q)
        x = gin['d_x'].astype(np.float64)
        x[3, 0] = bad
        m['X']._data = x
        with pytest.raises(exc, match=text):
            Q.update(verbose=False)


def test_parameters_initialisation_of_lam():
    from scipy import special
    from bayespy_amd.inference import VB
    rs = np.random.RandomState(3)
    m = _model()
    D, K = m['lam'].plates
    a, b = rs.gamma(2.0, size=(D, K)), rs.gamma(2.0, size=(D, K))
    m['lam'].initialize_from_parameters(a, b)
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    u = m['lam'].get_moments()
    np.testing.assert_allclose(u[0], a / b, rtol=1e-12)
    np.testing.assert_allclose(u[1], special.digamma(a) - np.log(b), rtol=1e-12)
    assert np.isfinite(Q.compute_lowerbound())
    Q.update(repeat=2, verbose=False)
    assert np.all(np.isfinite(Q.L[:2]))


def test_save_load_round_trip_and_a_differing_mask_is_refused(tmp_path):
    from pmm_models import run_pmm_cases
    g, gin = _golden()
    Q = run_pmm_cases(_mods(_on_double, engine='fused'), gin, only=('f',))['f_plan']
    fn = str(tmp_path / 'pmm.ckpt')
    Q.save(filename=fn)
    L4 = Q.L[:4].copy()
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    assert Q.iter == 4
    np.testing.assert_array_equal(Q.L[:4], L4)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)
    other = run_pmm_cases(_mods(_on_double, engine='fused'), gin, only=('a',))['a_plan']
    with pytest.raises(ValueError, match='checkpoint was saved with a mask on X'):
        other.load(filename=fn)


# -- the device header on the host ---------------------------------------------------------------------
def test_pack_dtypes_hidden_values_the_flags_and_the_cap():
    from pmm_host import host_pack, restate_pack, HIDDEN
    rs = np.random.RandomState(7)
    x = rs.poisson(4.0, size=(37, 9))
    x[0, 0], x[1, 1] = 0, 1
    mask = rs.rand(37, 9) < 0.7
    for a in (x.astype(np.int64), x.astype(np.float64), x.astype(np.int32), x.astype(np.uint8)):
        o = host_pack(a)
        assert not o['flags'].any() and (o['n_observed'], o['n_hidden']) == (x.size, 0)
        np.testing.assert_array_equal(o['xp'], x)
        o = host_pack(a, mask)
        assert not o['flags'].any()
        assert (o['n_observed'], o['n_hidden']) == (int(mask.sum()), int((~mask).sum()))
        np.testing.assert_array_equal(o['xp'], np.where(mask, x, HIDDEN))
        r = restate_pack(a, mask)
        np.testing.assert_array_equal(r['xp'], o['xp'])
        assert abs(o['lgam'] - float(r['lgam'])) <= 4 * np.spacing(float(r['lgam']))
    mask[5, 8], mask[6, 8] = True, False
    want = np.where(mask, x, HIDDEN)
    for v, flags in ((np.nan, (1, 0, 1)), (-1.0, (1, 0, 0)), (1e300, (0, 1, 0)), (0.5, (1, 0, 1)),
                     (-0.5, (1, 0, 1)), (65535.0, (0, 1, 0)), (np.inf, (0, 1, 0)),
                     (-np.inf, (1, 0, 0))):
        hidden = x.astype(np.float64)
        hidden[6, 8] = v
        o = host_pack(hidden, mask)
        assert not o['flags'].any()
        np.testing.assert_array_equal(o['xp'], want)
        bad = x.astype(np.float64)
        bad[5, 8] = v
        o = host_pack(bad, mask)
        assert tuple(o['flags']) == flags and o['xp'][5, 8] == HIDDEN, (v, o['flags'])
        np.testing.assert_array_equal(restate_pack(bad, mask)['flags'], flags)
    for v, flags in ((-1, (1, 0, 0)), (65535, (0, 1, 0)), (2 ** 40, (0, 1, 0)),
                     (-2 ** 40, (1, 0, 0))):
        bad = x.astype(np.int64)
        bad[5, 8] = v
        o = host_pack(bad, mask)
        assert tuple(o['flags']) == flags and o['xp'][5, 8] == HIDDEN
    ok = x.astype(np.int64)
    ok[5, 8] = 65534
    o = host_pack(ok, mask)
    assert not o['flags'].any() and o['xp'][5, 8] == 65534
    o = host_pack(ok.astype(np.float64), mask)
    assert not o['flags'].any() and o['xp'][5, 8] == 65534


SHAPES = [(0, 5, 3), (1, 1, 1), (65, 3, 2), (300, 70, 5), (257, 4, 16), (300, 129, 17),
          (515, 65, 2), (763, 257, 64)]


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_host_build_of_the_device_header_against_long_double(N, D, K):
    """The rule of DESIGN 4.14: the host build may differ from the long-double restatement by 8
    times the deviation of the plain float64 evaluation, floor 4 ulp of the magnitude."""
    from pmm_host import (host_pack, host_pass, host_tables, host_update, restate_pack,
                          restate_pass, restate_tables, restate_update, tolerances, error,
                          mixed_mask, pass_inputs, pmm_host, PASS_QUANTITIES, UPDATE_QUANTITIES)
    inp = pass_inputs(N, D, K)
    x, rs = inp['x'], inp['rs']
    assert pmm_host().pmm_chunk_rows(N, D, K) == 256
    for hidden in (0, 1):
        mask = mixed_mask(N, D, rs, pmm_host().pmm_dblock(1)) if hidden else None
        pk = host_pack(x, mask)
        assert not pk['flags'].any() and pk['n_hidden'] == (0 if mask is None else (~mask).sum())
        ld, f64 = restate_pack(x, mask), restate_pack(x, mask, np.float64)
        tol, _ = tolerances(ld, f64, ('lgam',))
        assert error(pk['lgam'], ld['lgam']) <= tol['lgam']
        for form in (hidden, hidden | 2):       # as they are (the bound of X), centred (the pass)
            l, lb, c, lsum = host_tables(D, K, form, inp['lam_mom'], inp['elog_pi'])
            for got, want in zip((l, lb, c, lsum),
                                 restate_tables(inp['lam_mom'], inp['elog_pi'], D, K, form,
                                                np.float64)):
                np.testing.assert_allclose(got, want, rtol=1e-14, atol=1e-12)
        got = host_pass(N, D, K, hidden, pk['xp'], None, l, lb, c, want_r=True)
        ld = restate_pass(x, mask, l, lb, c, hidden)
        f64 = restate_pass(x, mask, l, lb, c, hidden, np.float64)
        tol, dev = tolerances(ld, f64, PASS_QUANTITIES)
        for key in PASS_QUANTITIES:
            err = error(got[key], ld[key])
            assert err <= tol[key], (key, hidden, err, tol[key])
        if N and K > 1:                         # soft rows: a condition on the inputs
            assert np.mean(np.asarray(ld['r'], dtype=np.float64).max(axis=1) < 0.99) >= 0.5
        # the update from these statistics
        cnt = got['M'] if hidden else got['Nk']
        par, mom, bound = host_update(D, K, hidden, inp['a0'], inp['b0'], got['S'], cnt)
        ld = restate_update(inp['a0'], inp['b0'], got['S'], cnt)
        f64 = restate_update(inp['a0'], inp['b0'], got['S'], cnt, np.float64)
        tol, dev = tolerances(ld, f64, UPDATE_QUANTITIES)
        for key, val in (('par', par), ('mom', mom), ('bound', bound)):
            err = error(val, ld[key])
            assert err <= tol[key], (key, hidden, err, tol[key])
        # fixed labels: one-hot statistics, lse = 0
        h = host_pass(N, D, K, hidden, pk['xp'], inp['labels'], l, lb, c, want_r=True)
        m = np.ones((N, D), dtype=bool) if mask is None else mask
        one = np.eye(K)[inp['labels']] * m.any(axis=1)[:, None]
        np.testing.assert_array_equal(h['Nk'], one.sum(0))
        np.testing.assert_array_equal(h['S'], np.where(m, x, 0).astype(float).T @ one)
        if hidden:
            np.testing.assert_array_equal(h['M'], m.astype(float).T @ one)
        assert h['sum_lse'] == 0
    # a mask of ones packs to the bits of no mask
    np.testing.assert_array_equal(host_pack(x)['xp'], host_pack(x, np.ones((N, D)))['xp'])
    assert host_pack(x, np.ones((N, D)))['n_hidden'] == 0


def test_limits_chunks_workspace_and_the_blocks_of_the_pack():
    from pmm_host import pmm_host
    lib = pmm_host()
    assert (lib.pmm_max_k(), lib.pmm_max_d(), lib.pmm_max_count()) == (64, 1024, 65534)
    assert (lib.pmm_dblock(0), lib.pmm_dblock(1)) == (128, 64)
    for N, D, K in ((0, 1, 1), (10 ** 6, 256, 32), (10 ** 9, 1024, 64), (257, 3, 2)):
        rows, nc = lib.pmm_chunk_rows(N, D, K), lib.pmm_chunks(N, D, K)
        assert rows % 64 == 0 and rows >= 256 and nc <= 1024
        assert nc * rows >= N and (nc == 0 or (nc - 1) * rows < N)
        per = 2 * D * K + K + 1
        assert nc * per * 8 <= 2 ** 28
        assert lib.pmm_workspace_doubles(N, D, K) == max(nc * per + 1026, 2048)
    for n in (1, 255, 256, 257, 10 ** 5, 2 ** 18, 2 ** 18 + 1, 10 ** 9):
        span, nb = lib.pmm_pack_span(n), lib.pmm_pack_blocks(n)
        assert span % 256 == 0 and nb <= 1024 and nb * span >= n and (nb - 1) * span < n


def test_sanitized_stand_alone_program():
    """tests/host/pmm_host_main.cpp under -fsanitize=address,undefined, never loaded into Python."""
    from pmm_host import build_sanitized_program
    exe = build_sanitized_program()
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.count('flag=0') == 4 and 'runtime error' not in out.stdout


# -- the C ABI -----------------------------------------------------------------------------------------
ENTRY_POINTS = ('vmp_pmm_limits', 'vmp_pmm_plan', 'vmp_pmm_pack', 'vmp_pmm_tables', 'vmp_pmm_pass',
                'vmp_pmm_update')


def test_cabi_declares_the_pmm_entry_points_and_the_host_only_ones_answer():
    """Fails without the feature: the library has no such symbols."""
    from bayespy_amd import _lib
    from pmm_host import pmm_host
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    host = pmm_host()
    v = [ctypes.c_int32() for _ in range(3)]
    assert lib.vmp_pmm_limits(*[ctypes.byref(a) for a in v]) == _lib.VMP_OK
    assert tuple(a.value for a in v) == (host.pmm_max_k(), host.pmm_max_d(), host.pmm_max_count())
    assert lib.vmp_pmm_limits(None, None, None) == _lib.VMP_ERR_INVALID
    c, w = ctypes.c_int64(), ctypes.c_int64()
    for N, D, K in ((0, 1, 1), (1000, 7, 5), (10 ** 6, 256, 32), (10 ** 6, 1024, 64)):
        assert lib.vmp_pmm_plan(N, D, K, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_OK
        assert c.value == host.pmm_chunk_rows(N, D, K)
        assert w.value == host.pmm_workspace_doubles(N, D, K)
    for D, K in ((4, 65), (1025, 4)):
        assert lib.vmp_pmm_plan(10, D, K, ctypes.byref(c), ctypes.byref(w)) \
            == _lib.VMP_ERR_UNSUPPORTED
        assert lib.vmp_pmm_plan(10, D, K, None, None) == _lib.VMP_ERR_UNSUPPORTED   # shape first
    for N, D, K in ((-1, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert lib.vmp_pmm_plan(N, D, K, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_plan(10, 4, 4, None, None) == _lib.VMP_ERR_INVALID


def test_argument_rules_of_the_device_entry_points_without_a_context():
    """A null context is refused before anything else is looked at: VMP_ERR_INVALID, no launch."""
    from bayespy_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.vmp_pmm_pack(None, 4, 4, 0, *[p] * 7) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_tables(None, 4, 4, 0, *[p] * 6) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_pass(None, 4, 4, 4, 0, *[p] * 11) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_update(None, 4, 4, 0, *[p] * 7) == _lib.VMP_ERR_INVALID
    assert not buf.any()
