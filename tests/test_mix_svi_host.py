"""CPU: stochastic variational inference on the fused count-mixture blocks without a device -- the
SVI matchers and their declining reasons, the registry, the plans on the kernel doubles of
tests/*_host.py with the step restated in NumPy (tests/mix_svi_host.py) against
tests/golden/mix_svi.npz (live reference, tools/make_golden_mix_svi.py), the one-pass-per-step rule,
the multiplier setter, checkpoints and the C ABI."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

L_RTOL = 1e-9                               # tests/test_pmm_host.py and its siblings
MOM_TOL = dict(rtol=1e-6, atol=1e-9)


def _mods(tag=None, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from mix_svi_host import on_double
    m = dict(nodes=nodes, VB=VB, vb_kwargs=kw)
    if tag is not None:
        m['after_vb'] = on_double(tag)
    return m


def _golden():
    return np.load(os.path.join(GOLDEN, 'mix_svi.npz'))


def _plan_class(tag):
    from bayespy_amd.inference import plans
    from mix_svi_host import PLAN
    return getattr(plans, PLAN[tag])


def _nodes(m):
    return [m['X'], m['Z'], m['par'], m['R']]


def check_trace(res, g, tag, first=0):
    import mix_svi_models as M
    np.testing.assert_allclose(res[tag + '_L'], g[tag + '_L'][first:], rtol=L_RTOL)
    np.testing.assert_allclose(res[tag + '_terms'], g[tag + '_terms'][first:], rtol=L_RTOL,
                               atol=1e-9)
    n = 0
    for k in M.MOMENTS:
        if tag + '_' + k in g.files:
            want = g[tag + '_' + k]
            np.testing.assert_allclose(res[tag + '_' + k],
                                       want if k == 'Z_u0_last' else want[first:],
                                       err_msg=tag + '_' + k, **MOM_TOL)
            n += 1
    return n


# -- matchers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['bmm', 'bmm_mask', 'pmm', 'pmm_value', 'binm', 'cmm', 'mmm'])
def test_svi_matcher_accepts_and_the_block_still_declines(tag):
    import mix_svi_models as M
    g = _golden()
    P = _plan_class(tag)
    block = P.__mro__[2]
    assert block.__name__ == P.__name__.replace('SVI', '')
    for observed in (False, True):
        m = M.build(_mods(), g, tag)
        if observed:
            M.observe(m['X'], *M.batch(g, tag, 0))
        why = []
        r = P.match(_nodes(m), why)
        assert r is not None and why == [], why
        assert r['Z'] is m['Z'] and r['R'] is m['R'] and r[P.PARAM] is m['par']
        why = []
        assert block.match(_nodes(m), why) is None and len(why) == 1
        assert 'plates_multiplier' in why[0] and '(stochastic VI)' not in why[0]
    assert P.KIND == block.KIND + '_svi'


@pytest.mark.parametrize('tag', ['bmm', 'pmm', 'binm', 'cmm', 'mmm'])
def test_svi_matcher_declines_with_reasons(tag):
    import mix_svi_models as M
    g = _golden()
    P = _plan_class(tag)
    vector = tag == 'mmm'

    def reason(m):
        why = []
        assert P.match(_nodes(m), why) is None and len(why) == 1, why
        assert why[0].startswith(P.LABEL + ' (stochastic VI), observed node X: '), why[0]
        return why[0]
    # a factor on a global node: the parameter node, the weights
    m = M.build(_mods(), g, tag)
    m['par'].plates_multiplier = (2.0,) if vector else (1, 2.0)
    assert 'global node (%s)' % m['par'].name in reason(m)
    m = M.build(_mods(), g, tag)
    m['R'].plates_multiplier = (3.0,)
    assert 'global node' in reason(m)
    # different factors on Z and X, a factor that is not positive
    m = M.build(_mods(), g, tag, m=1.0)
    m['X'].plates_multiplier = (2.0,) if vector else (2.0, 1)
    assert 'not one positive factor' in reason(m)
    m = M.build(_mods(), g, tag, m=-2.0)
    assert 'not one positive factor' in reason(m)
    # a factor on another axis
    if not vector:
        m = M.build(_mods(), g, tag)
        m['Z'].plates_multiplier = (M.N / M.NB, 2.0)
        assert 'axis other than the rows' in reason(m)
    # sharded plates
    m = M.build(_mods(), g, tag)
    m['Z']._shard_axis = 0
    assert 'sharded' in reason(m)
    # the checks of the block itself are made as before: a mask that broadcasts
    m = M.build(_mods(), g, tag)
    rows, _ = M.batch(g, tag, 0)
    m['X'].observe(rows, mask=False)
    assert 'mask of shape ()' in reason(m)


def test_registry():
    from bayespy_amd.inference import plans
    assert {P.__name__: [Q.__name__ for Q in v] for P, v in plans.OPT_IN_BATCHES.items()} == {
        'BernoulliMixturePlan': ['BernoulliMixtureSVIPlan'],
        'CategoricalMixturePlan': ['CategoricalMixtureSVIPlan'],
        'PoissonMixturePlan': ['PoissonMixtureSVIPlan'],
        'MultinomialMixturePlan': ['MultinomialMixtureSVIPlan'],
        'BinomialMixturePlan': ['BinomialMixtureSVIPlan']}
    assert [P.__name__ for P in plans.OPT_IN_COUNTS] == ['PoissonMixturePlan']
    assert [P.__name__ for P in plans.OPT_IN_TRIALS] == ['BinomialMixturePlan']
    assert plans.OPT_IN_AFTER[plans.GMMPlan] == [plans.GMMSVIPlan]


@pytest.mark.parametrize('tag', ['bmm', 'pmm', 'binm', 'cmm', 'mmm'])
def test_engine_fused_batches_takes_the_model_and_the_other_engines_do_not(tag):
    """Fails without the feature: no engine builds a fused block for these models."""
    import mix_svi_models as M
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.generic import GenericPlan
    import host_generic
    g = _golden()
    m = M.build(_mods(), g, tag)
    M.observe(m['X'], *M.batch(g, tag, 0))
    Q = VB(*_nodes(m), engine='fused+batches')
    assert type(Q.plans[0]) is _plan_class(tag)
    assert VB(*_nodes(m), engine='fused+batches').plans[0] is Q.plans[0]
    # plain engine='fused' does not try the mini-batch forms: it raises with the block's reason, as
    # before; a plan of that kind is not kept for it, and the engine built above keeps its nodes
    with pytest.raises(NotImplementedError, match='plates_multiplier') as err:
        VB(*_nodes(m), engine='fused')
    assert '(stochastic VI)' not in str(err.value)
    assert all(n._plan is Q.plans[0] for n in _nodes(m))
    host_generic.install()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            got = compile_model(_nodes(m))
        assert len(got) == 1 and isinstance(got[0], GenericPlan)
    finally:
        host_generic.uninstall()
    # the diagonal-Gaussian blocks have no such form: declined with the reason they always gave
    import bayespy_amd.nodes as N_
    R = N_.Dirichlet([1.0, 1.0], name='R')
    Z = N_.Categorical(R, plates=(10, 1), plates_multiplier=(4.0, 1), name='Z')
    mu = N_.GaussianARD(0, 1e-3, plates=(2, 2), name='mu')
    tau = N_.Gamma(1e-3, 1e-3, plates=(2, 2), name='tau')
    Y = N_.Mixture(Z, N_.GaussianARD, mu, tau, name='Y')
    Y.observe(np.zeros((10, 2)))
    with pytest.raises(NotImplementedError, match='plates_multiplier'):
        VB(Y, Z, mu, tau, R, engine='fused+batches')


# -- the traces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['bmm', 'bmm_mask', 'pmm', 'pmm_value', 'binm', 'cmm', 'mmm'])
def test_golden_trace_on_the_kernel_double(tag):
    import mix_svi_models as M
    g = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = M.run_case(_mods(tag, engine='fused+batches'), g, tag)
    assert check_trace(res, g, tag) == (4 if tag.startswith('pmm') else 3)
    plan = res[tag + '_plan'].plans[0]
    calls = [c.replace('_masked', '').replace('_hidden', '') for c in plan.kernels.calls]
    # per step one pack, one table launch for the pass, one pass, one step of both nodes; the set-up
    # adds one pass for the initial state, the responsibilities are written once at the end
    assert calls.count('pack') == M.STEPS
    assert calls.count('pass') == 1 + M.STEPS and calls.count('pass_r') == 1
    assert calls.count('natural_step_3') == M.STEPS
    assert not any(c.startswith('update') for c in calls[3:])
    if tag == 'pmm_value':          # the point mass stepped from its prior: no NaN anywhere
        assert np.all(np.isfinite(plan.lam_par.numpy()))
    if tag == 'pmm':                # the hidden column of batch 2 stayed finite and kept moving
        assert np.all(np.isfinite(res['pmm_par_u1']))


def _step_calls(plan, fn):
    k = plan.kernels
    n = len(k.calls)
    fn()
    return [c.replace('_masked', '').replace('_hidden', '') for c in k.calls[n:]
            if c != 'dot' and not c.startswith('dirichlet')]


@pytest.mark.parametrize('tag', ['bmm_mask', 'pmm', 'binm', 'cmm', 'mmm'])
def test_one_pack_one_table_launch_and_one_pass_per_step(tag):
    import mix_svi_models as M
    g = _golden()
    seen = {}

    def on_step(Q, m, n):
        seen['Q'], seen['m'] = Q, m
    M.run_case(_mods(tag, engine='fused+batches'), g, tag, on_step=on_step)
    Q, m = seen['Q'], seen['m']
    plan = Q.plans[0]
    X, Z, P, R = m['X'], m['Z'], m['par'], m['R']
    pmm = tag.startswith('pmm')
    tables_of_bound = ['tables'] if pmm else []

    def step():
        M.observe(X, *M.batch(g, tag, 1))
        Q.update(Z, verbose=False)
        Q.gradient_step(P, R, scale=0.3)
    # (VB.update evaluates the bound after the update; that of the Poisson block launches its
    # tables in the uncentred form for the term of X -- not a launch of the step)
    assert _step_calls(plan, step) == ['pack', 'tables', 'pass'] + tables_of_bound \
        + ['natural_step_3']
    # the moments of the global nodes depend on no batch: the new data are packed, no pass runs
    M.observe(X, *M.batch(g, tag, 2))
    assert _step_calls(plan, lambda: (P.get_moments(), R.get_moments())) == ['pack']
    assert _step_calls(plan, lambda: Q.update(Z, verbose=False)) \
        == ['tables', 'pass'] + tables_of_bound
    # the statistics of the batch are read before update(Z): the pass runs at that point, once
    M.observe(X, *M.batch(g, tag, 3))
    assert _step_calls(plan, lambda: Q.gradient_step(R, scale=0.5)) \
        == ['pack', 'pass', 'natural_step_2']
    assert _step_calls(plan, lambda: Q.update(Z, verbose=False)) \
        == ['tables', 'pass'] + tables_of_bound
    M.observe(X, *M.batch(g, tag, 4))
    assert _step_calls(plan, Q.compute_lowerbound) == ['pack', 'pass'] + tables_of_bound
    assert _step_calls(plan, Q.compute_lowerbound) == []
    M.observe(X, *M.batch(g, tag, 5))
    assert _step_calls(plan, Z.get_moments) == ['pack', 'pass_r']
    assert _step_calls(plan, lambda: Q.update(P, verbose=False)) \
        == ['natural_step_1'] + tables_of_bound


def test_gradient_step_of_z_is_refused_and_update_is_a_full_step():
    import mix_svi_models as M
    g = _golden()
    res = M.run_case(_mods('cmm', engine='fused+batches'), g, 'cmm')
    Q = res['cmm_plan']
    with pytest.raises(NotImplementedError, match='gradient step of Z: the fused categorical-mixture '
                                                  'block keeps no natural parameters'):
        Q.gradient_step('Z', scale=0.5)
    # update(P) then update(R) leaves what gradient_step(P, R, scale=1) leaves
    plan = Q.plans[0]
    keep = {k: getattr(plan, k).clone() for k in ('alpha_p', 'alpha_r', 'elog_p', 'elog_r')}
    Q.gradient_step('P', 'R', scale=1.0)
    both = {k: getattr(plan, k).numpy().copy() for k in keep}
    for k, v in keep.items():
        getattr(plan, k).copy_(v)
    Q.update('P', verbose=False)
    Q.update('R', verbose=False)
    for k in keep:
        np.testing.assert_array_equal(getattr(plan, k).numpy(), both[k], err_msg=k)
    want = plan.prior_p.numpy() + (M.N / M.NB) * plan.S.numpy()
    np.testing.assert_allclose(plan.alpha_p.numpy(), want, rtol=1e-15)


def test_the_multiplier_setter_keeps_the_state():
    import mix_svi_models as M
    g = _golden()
    res = M.run_case(_mods('pmm_value', engine='fused+batches'), g, 'pmm_value')
    Q = res['pmm_value_plan']
    plan = Q.plans[0]
    Z, X, lam = Q['Z'], Q['X'], Q['lam']
    u = lam.get_moments()[0].copy()
    t0 = [float(n.lower_bound_contribution()) for n in (X, Z, lam)]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        Z.plates_multiplier = (2.0, 1)
    assert Q.plans[0] is plan and plan._ready
    np.testing.assert_array_equal(lam.get_moments()[0], u)
    t1 = [float(n.lower_bound_contribution()) for n in (X, Z, lam)]
    m = M.N / M.NB
    np.testing.assert_allclose(t1[0], t0[0] * 2.0 / m, rtol=1e-13)
    np.testing.assert_allclose(t1[1], t0[1] * 2.0 / m, rtol=1e-13)
    assert t1[2] == t0[2]
    S, a0 = plan.S.numpy().copy(), plan.a0.numpy()
    Q.update(lam, verbose=False)
    np.testing.assert_allclose(plan.lam_par.numpy()[:, 0], (a0 + 2.0 * S).reshape(-1), rtol=1e-15)


@pytest.mark.parametrize('tag', ['bmm_mask', 'pmm', 'mmm'])
def test_checkpoint_at_step_three_continues_the_trace_in_a_fresh_model(tag, tmp_path):
    import mix_svi_models as M
    g = _golden()
    fn = str(tmp_path / 'svi.ckpt')

    def save(Q, m, n):
        if n == 2:
            Q.save(filename=fn)
    M.run_case(_mods(tag, engine='fused+batches'), g, tag, on_step=save)
    assert _plan_class(tag).KIND.endswith('_svi')

    def load(Q, m):
        # the batch of step 2 is observed again first: a checkpoint is refused under another mask
        M.observe(m['X'], *M.batch(g, tag, 2))
        Q.load(filename=fn)
        M.observe(m['X'], *M.batch(g, tag, 3))
    res = M.run_case(_mods(tag, engine='fused+batches'), g, tag, first=3, before=load)
    check_trace(res, g, tag, first=3)


# -- the C ABI -----------------------------------------------------------------------------------------
def test_cabi_declares_the_step_and_its_host_only_entry_answers():
    """Fails without the feature: the library has no such symbols."""
    from bayespy_amd import _lib
    lib = _lib.load()
    for name in ('vmp_mix_natural_step', 'vmp_mix_natural_step_workspace'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    w = ctypes.c_int64()
    q = lib.vmp_mix_natural_step_workspace
    assert q(0, 195, 2, 3, ctypes.byref(w)) == _lib.VMP_OK and w.value == 2
    assert q(0, 64, 1024, 64, ctypes.byref(w)) == _lib.VMP_OK and w.value == 65
    assert q(1, 65536, 2, 64, ctypes.byref(w)) == _lib.VMP_OK and w.value == 257
    assert q(0, 0, 2, 1, ctypes.byref(w)) == _lib.VMP_OK and w.value >= 1
    assert q(2, 4, 2, 1, ctypes.byref(w)) == _lib.VMP_ERR_INVALID
    assert q(0, -1, 2, 1, ctypes.byref(w)) == _lib.VMP_ERR_INVALID
    assert q(0, 4, 2, 1, None) == _lib.VMP_ERR_INVALID
    # a null context is refused before anything else is looked at: nothing is launched or written
    buf = np.zeros(64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.vmp_mix_natural_step(None, 0, 3, 4, 2, 2, 1, p, p, p, p, 0, p, p, 2, p, p, p, p, 1.0,
                                    1.0, p, p) == _lib.VMP_ERR_INVALID
    assert not buf.any()


def test_long_double_special_functions_of_the_restatement():
    """The yardstick of the GPU test against mpmath at 40 digits."""
    import mpmath
    from mix_svi_host import digamma_ld, gammaln_ld
    mpmath.mp.dps = 40
    x = np.array([1e-3, 0.01, 0.5, 1.0, 2.5, 23.9, 24.0, 100.25, 7e4, 3e8])
    for fn, ref in ((digamma_ld, mpmath.digamma), (gammaln_ld, mpmath.loggamma)):
        got = fn(x)
        for v, gv in zip(x, got):
            want = ref(mpmath.mpf(float(v)))
            err = abs(mpmath.mpf(np.format_float_positional(gv, unique=False, precision=25))
                      - want)
            # up to 24 steps of the recurrence, each rounded to half an ulp of long double (5.4e-20
            # at one; ln Gamma of a small x is the difference of two numbers near 55, whose ulp is
            # 3.5e-18): a tenth of the float64 ulp at the worst
            assert err <= 2e-17 * max(1, abs(want)), (fn.__name__, v, err)
