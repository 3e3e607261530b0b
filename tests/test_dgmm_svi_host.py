"""CPU: stochastic variational inference on the two fused diagonal-Gaussian blocks without a device
-- the new engine value and the answers of the others, the registry, the matchers' declining reasons,
the g++ build of csrc/vmp_dgmm_svi_dev.h against a long-double restatement, the plans on the kernel
doubles (tests/dgmm_svi_host.py) against tests/golden/dgmm_svi.npz (live reference,
tools/make_golden_dgmm_svi.py), the one-pass-per-step rule, checkpoints, annealing and the C ABI."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ENGINE = 'fused+batches+gaussian'


def _tolerances():
    from test_dgmm_host import L_RTOL, MOM_TOL      # the tolerances of the block
    return L_RTOL, MOM_TOL


def _mods(tag=None, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from dgmm_svi_host import on_double
    m = dict(nodes=nodes, VB=VB, vb_kwargs=kw)
    if tag is not None:
        m['after_vb'] = on_double(tag)
    return m


def _golden():
    return np.load(os.path.join(GOLDEN, 'dgmm_svi.npz'))


def _plan_class(tag):
    from bayespy_amd.inference import plans
    from dgmm_svi_host import PLAN
    return getattr(plans, PLAN[tag])


def check_trace(res, g, tag, first=0):
    """``check_trace`` of tests/test_mix_svi_host.py for the moments these models record, with the
    tolerances of tests/test_dgmm_host.py."""
    import dgmm_svi_models as M
    L_RTOL, MOM_TOL = _tolerances()
    np.testing.assert_allclose(res[tag + '_L'], g[tag + '_L'][first:], rtol=L_RTOL)
    np.testing.assert_allclose(res[tag + '_terms'], g[tag + '_terms'][first:], rtol=L_RTOL,
                               atol=1e-9)
    n = 0
    for k in M.MOMENTS:
        want = g[tag + '_' + k]
        np.testing.assert_allclose(res[tag + '_' + k], want if k == 'Z_u0_last' else want[first:],
                                   err_msg=tag + '_' + k, **MOM_TOL)
        n += 1
    return n


def _observed(tag, g=None, m=None):
    import dgmm_svi_models as M
    g = _golden() if g is None else g
    m = M.build(_mods(), g, tag) if m is None else m
    M.observe(m['Y'], *M.batch(g, tag, 0))
    return m


# -- the engine values -----------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['par', 'value', 'mask'])
def test_the_new_engine_value_builds_the_svi_plans_and_the_others_answer_as_before(tag):
    """Fails without the feature: no engine value builds a fused block for these models."""
    import dgmm_svi_models as M
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.generic import GenericPlan
    import host_generic
    m = _observed(tag)
    nodes = M.nodes_of(m)
    Q = VB(*nodes, engine=ENGINE)
    assert type(Q.plans[0]) is _plan_class(tag) and len(Q.plans) == 1
    assert VB(*nodes, engine=ENGINE).plans[0] is Q.plans[0]
    # 'fused' and 'fused+batches' do not try these forms: they raise with the block's reason, as
    # before; a plan of that kind is not kept for them, and the engine built above keeps its nodes
    for engine in ('fused', 'fused+batches'):
        with pytest.raises(NotImplementedError, match='plates_multiplier') as err:
            VB(*nodes, engine=engine)
        assert '(stochastic VI)' not in str(err.value)
        assert all(n._plan is Q.plans[0] for n in nodes)
    host_generic.install()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            got = compile_model(nodes)
        assert len(got) == 1 and isinstance(got[0], GenericPlan)
    finally:
        host_generic.uninstall()


def test_the_engine_value_comes_through_the_environment_and_keeps_the_count_forms(monkeypatch):
    import dgmm_svi_models as M
    import mix_svi_models as MM
    from bayespy_amd.inference import VB
    m = _observed('par')
    monkeypatch.setenv('BAYESPY_AMD_ENGINE', ENGINE)
    assert type(VB(*M.nodes_of(m)).plans[0]) is _plan_class('par')
    monkeypatch.delenv('BAYESPY_AMD_ENGINE')
    # everything 'fused+batches' gives
    g = np.load(os.path.join(GOLDEN, 'mix_svi.npz'))
    mm = MM.build(_mods(), g, 'pmm')
    MM.observe(mm['X'], *MM.batch(g, 'pmm', 0))
    Q = VB(mm['X'], mm['Z'], mm['par'], mm['R'], engine=ENGINE)
    assert type(Q.plans[0]).__name__ == 'PoissonMixtureSVIPlan'


def test_registry():
    from bayespy_amd.inference import plans
    assert {P.__name__: [Q.__name__ for Q in v]
            for P, v in plans.OPT_IN_GAUSSIAN_BATCHES.items()} == {
        'DiagGaussianMixturePlan': ['DiagGaussianMixtureSVIPlan'],
        'MaskedDiagGaussianMixturePlan': ['MaskedDiagGaussianMixtureSVIPlan']}
    for P, (Q,) in plans.OPT_IN_GAUSSIAN_BATCHES.items():
        assert issubclass(Q, P) and Q.KIND == 'dgmm_svi' and Q.ANNEALING is False
    assert not any(Q in v for Q in (plans.DiagGaussianMixtureSVIPlan,
                                    plans.MaskedDiagGaussianMixtureSVIPlan)
                   for v in plans.OPT_IN_BATCHES.values())


# -- matchers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', ['par', 'mask'])
def test_svi_matcher_accepts_and_the_block_still_declines(tag):
    import dgmm_svi_models as M
    P = _plan_class(tag)
    block = P.__mro__[3]
    assert block.__name__ == P.__name__.replace('SVI', '')
    m = _observed(tag)
    why = []
    r = P.match(M.nodes_of(m), why)
    assert r is not None and why == [], why
    assert all(r[k] is m[k] for k in ('Y', 'Z', 'mu', 'tau', 'alpha'))
    why = []
    assert block.match(M.nodes_of(m), why) is None and len(why) == 1
    assert 'plates_multiplier' in why[0] and '(stochastic VI)' not in why[0]


@pytest.mark.parametrize('tag', ['par', 'mask'])
def test_svi_matcher_declines_with_reasons(tag):
    import dgmm_svi_models as M
    g = _golden()
    P = _plan_class(tag)

    def reason(m):
        why = []
        assert P.match(M.nodes_of(m), why) is None and len(why) == 1, why
        assert why[0].startswith(P.LABEL + ' (stochastic VI), observed node Y: '), why[0]
        return why[0]
    # a factor on a global node: mu, tau, the weights
    for key, mult in (('mu', (1, 2.0)), ('tau', (1, 2.0)), ('alpha', (3.0,))):
        m = _observed(tag, g)
        m[key].plates_multiplier = mult
        assert 'global node (%s)' % key in reason(m)
    # different factors on Z and Y, a factor that is not positive
    m = _observed(tag, g, M.build(_mods(), g, tag, m=1.0))
    m['Y'].plates_multiplier = (2.0, 1)
    assert 'not one positive factor' in reason(m)
    m = _observed(tag, g, M.build(_mods(), g, tag, m=-2.0))
    assert 'not one positive factor' in reason(m)
    # a factor on another axis
    m = _observed(tag, g)
    m['Z'].plates_multiplier = (M.N / M.NB, 2.0)
    assert 'axis other than the rows' in reason(m)
    # sharded plates
    m = _observed(tag, g)
    m['Z']._shard_axis = 0
    assert 'sharded' in reason(m)
    # the checks of the block itself are made as before: a mask that broadcasts, tau from a value
    m = _observed(tag, g)
    m['Y'].observe(M.batch(g, tag, 0)[0], mask=False)
    assert 'mask of shape ()' in reason(m) or 'it has a mask' in reason(m)
    m = _observed(tag, g)
    m['tau'].initialize_from_value(np.ones((M.D, M.K)))
    assert 'tau is initialised by value' in reason(m)


# -- the host build of the device header -------------------------------------------------------------------
@pytest.mark.parametrize('D,K', [(1, 1), (3, 2), (65, 5)])
@pytest.mark.parametrize('per_element', [0, 1])
@pytest.mark.parametrize('mult,scale', [(1.0, 1.0), (400 / 70, 0.37), (4.0, 1.0)])
def test_host_build_against_long_double(D, K, per_element, mult, scale):
    """8 times the deviation of the float64 evaluation of the reference's own form from long
    double, floor 4 ulp of the magnitude: the rule of tests/test_dgmm_gpu.py."""
    from dgmm_host import tolerances, error
    from dgmm_svi_host import host_step, restate_step, step_inputs, STEP_QUANTITIES
    x = step_inputs(D, K, per_element)
    args = (x['m0'], x['beta0'], x['a0'], x['b0'], x['S1'], x['S2'])
    tabs = (x['mu_par'], x['mu_mom'], x['tau_par'], x['tau_mom'])
    ld = restate_step(*args, x['full'], *tabs, mult, scale, np.longdouble)
    f64 = restate_step(*args, x['full'], *tabs, mult, scale, np.float64)
    tol, _ = tolerances(ld, f64, STEP_QUANTITIES)
    got = host_step(D, K, 3, per_element, *args, x['cnt'], *tabs, mult, scale)
    got['mu_bound'], got['tau_bound'] = got['bound']
    for q in STEP_QUANTITIES:
        print('%s: error %.3g allowed %.3g' % (q, error(got[q], ld[q]), tol[q]))
    for q in STEP_QUANTITIES:
        assert error(got[q], ld[q]) <= tol[q], (q, error(got[q], ld[q]), tol[q])


def test_host_build_leaves_the_bits_of_the_updates_and_of_unnamed_nodes():
    from dgmm_host import host_update
    from dgmm_masked_host import host_update_masked
    from dgmm_svi_host import host_step, step_inputs
    D, K = 65, 5
    nan = np.full((D * K, 2), np.nan)
    for per_element, upd in ((0, host_update), (1, host_update_masked)):
        x = step_inputs(D, K, per_element)
        S1, S2, cnt = x['S1'], x['S2'], x['cnt']
        args = (x['m0'], x['beta0'], x['a0'], x['b0'], S1, S2, cnt)
        both = host_step(D, K, 3, per_element, *args, nan, x['mu_mom'], nan, x['tau_mom'], 1.0, 1.0)
        for bit, which, name, pa, pb, other in ((1, 0, 'mu', x['m0'], x['beta0'], x['tau_mom']),
                                                (2, 1, 'tau', x['a0'], x['b0'], x['mu_mom'])):
            par, mom, bound = upd(D, K, which, pa, pb, S1, S2, cnt, other)
            one = host_step(D, K, bit, per_element, *args, nan, x['mu_mom'], nan, x['tau_mom'],
                            1.0, 1.0)
            for got in (one, both):     # each optimum comes from the state at entry
                np.testing.assert_array_equal(got[name + '_par'], par)
                np.testing.assert_array_equal(got[name + '_mom'], mom)
                assert got['bound'][which] == bound
            # the node that is not named keeps every bit, its bound slot too
            quiet = 'tau' if name == 'mu' else 'mu'
            assert np.all(np.isnan(one[quiet + '_par'])) and np.isnan(one['bound'][1 - which])
            np.testing.assert_array_equal(one[quiet + '_mom'], x[quiet + '_mom'])


# -- the traces ----------------------------------------------------------------------------------------
def _counted(calls):
    return [c.replace('_masked', '') for c in calls if c != 'dot' and not c.startswith('dirichlet')]


@pytest.mark.parametrize('tag', ['par', 'value', 'mask'])
def test_golden_trace_on_the_kernel_double(tag):
    import dgmm_svi_models as M
    g = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = M.run_case(_mods(tag, engine=ENGINE), g, tag)
    assert check_trace(res, g, tag) == 6
    plan = res[tag + '_plan'].plans[0]
    calls = _counted(plan.kernels.calls)
    # per step one pack (with a mask), one pass, one step of the three nodes; the set-up adds one
    # pass for the initial state, the responsibilities are written once at the end
    if tag == 'mask':
        assert calls.count('pack') == M.STEPS
    assert calls.count('pass') == 1 + M.STEPS and calls.count('pass_r') == 1
    assert calls.count('natural_step_7') == M.STEPS
    first = calls.index('pass')
    assert not any(c.startswith('update') for c in calls[first:])
    for name in ('mu_par', 'mu_mom', 'tau_par', 'tau_mom'):     # no NaN anywhere
        assert np.all(np.isfinite(getattr(plan, name).numpy())), (tag, name)
    if tag == 'mask':       # the hidden column of batch 2 stayed finite and kept moving
        col, n = M.HIDDEN_COLUMN, M.HIDDEN_BATCH
        for k in ('mu_u0', 'mu_u1', 'tau_u0', 'tau_u1'):
            u = res['mask_' + k]
            assert np.all(np.isfinite(u))
            assert np.all(u[n, col] != u[n - 1, col]) and np.all(u[n + 1, col] != u[n, col])


@pytest.mark.parametrize('tag', ['par', 'mask'])
def test_one_upload_one_table_launch_one_pass_and_one_step_per_step(tag):
    import dgmm_svi_models as M
    g = _golden()
    seen = {}
    M.run_case(_mods(tag, engine=ENGINE), g, tag, on_step=lambda Q, m, n: seen.update(Q=Q, m=m))
    Q, m = seen['Q'], seen['m']
    plan = Q.plans[0]
    Y, Z, mu, tau, alpha = M.nodes_of(m)
    k = plan.kernels
    upload = type(plan)._upload_y

    def counted_upload():       # the block without a mask uploads y with no kernel of its own
        if tag != 'mask':
            k.calls.append('pack')
        upload(plan)
    plan._upload_y = counted_upload

    def calls(fn):
        n = len(k.calls)
        fn()
        return _counted(k.calls[n:])

    def step():
        M.observe(Y, *M.batch(g, tag, 1))
        Q.update(Z, verbose=False)
        Q.gradient_step(mu, tau, alpha, scale=0.3)
    # (VB.update evaluates the bound after the update; the bound launches the tables of the present
    # moments for the term of Y -- not a launch of the step)
    assert calls(step) == ['pack', 'tables', 'pass', 'tables', 'natural_step_7']
    # the moments of the global nodes depend on no batch: the new data are packed, no pass runs
    M.observe(Y, *M.batch(g, tag, 2))
    assert calls(lambda: (mu.get_moments(), tau.get_moments(), alpha.get_moments())) == ['pack']
    assert calls(lambda: Q.update(Z, verbose=False)) == ['tables', 'pass', 'tables']
    # the statistics of the batch are read before update(Z): the pass runs at that point, once
    M.observe(Y, *M.batch(g, tag, 3))
    assert calls(lambda: Q.gradient_step(tau, alpha, scale=0.5)) == ['pack', 'pass', 'natural_step_6']
    assert calls(lambda: Q.update(Z, verbose=False)) == ['tables', 'pass', 'tables']
    M.observe(Y, *M.batch(g, tag, 4))
    assert calls(Q.compute_lowerbound) == ['pack', 'pass', 'tables']
    assert calls(Q.compute_lowerbound) == []
    M.observe(Y, *M.batch(g, tag, 5))
    assert calls(Z.get_moments) == ['pack', 'pass_r']
    assert calls(lambda: Q.update(mu, verbose=False)) == ['natural_step_1', 'tables']
    assert calls(lambda: Q.update(alpha, verbose=False)) == ['natural_step_4', 'tables']


@pytest.mark.parametrize('tag', ['par', 'mask'])
def test_gradient_step_of_one_node_leaves_the_others_and_update_is_a_full_step(tag):
    import dgmm_svi_models as M
    g = _golden()
    Q = M.run_case(_mods(tag, engine=ENGINE), g, tag)[tag + '_plan']
    plan = Q.plans[0]
    names = ('mu_par', 'mu_mom', 'tau_par', 'tau_mom', 'alpha_r', 'elog_r', 'scal')
    keep = {k: getattr(plan, k).numpy().copy() for k in names}
    Q.gradient_step('mu', scale=0.4)
    for k in names[2:6]:
        np.testing.assert_array_equal(getattr(plan, k).numpy(), keep[k], err_msg=k)
    np.testing.assert_array_equal(plan.scal.numpy()[4:6], keep['scal'][4:6])
    assert np.all(plan.mu_par.numpy() != keep['mu_par'])
    with pytest.raises(NotImplementedError, match='gradient step of Z: the fused diagonal-Gaussian-'
                                                  'mixture block keeps no natural parameters'):
        Q.gradient_step('Z', scale=0.5)
    # update(mu), update(tau), update(alpha) from one state leave what gradient_step(all, scale=1)
    # leaves of each: every optimum comes from the state at entry
    def restore():
        for k in names:
            getattr(plan, k).copy_(plan.rt.torch.from_numpy(keep[k]))
    restore()
    Q.gradient_step('mu', 'tau', 'alpha', scale=1.0)
    both = {k: getattr(plan, k).numpy().copy() for k in names}
    for node, mine in (('mu', names[0:2]), ('tau', names[2:4]), ('alpha', names[4:6])):
        restore()
        Q.update(node, verbose=False)
        for k in mine:
            np.testing.assert_array_equal(getattr(plan, k).numpy(), both[k], err_msg=k)
    m = M.N / M.NB
    cnt = plan.M.numpy() if tag == 'mask' else np.broadcast_to(plan.Nk.numpy(), (M.D, M.K))
    np.testing.assert_allclose(both['tau_par'][:, 0],
                               (plan.a0.numpy() + 0.5 * m * cnt).reshape(-1), rtol=1e-15)


@pytest.mark.parametrize('tag', ['value', 'mask'])
def test_checkpoint_at_step_three_continues_the_trace_in_a_fresh_model(tag, tmp_path):
    import dgmm_svi_models as M
    g = _golden()
    fn = str(tmp_path / 'svi.ckpt')
    full = {}

    def save(Q, m, n):
        if n == 2:
            Q.save(filename=fn)
    full.update(M.run_case(_mods(tag, engine=ENGINE), g, tag, on_step=save))

    def load(Q, m):
        # the batch of step 2 is observed again first: a checkpoint is refused under another mask
        M.observe(m['Y'], *M.batch(g, tag, 2))
        Q.load(filename=fn)
        M.observe(m['Y'], *M.batch(g, tag, 3))
    res = M.run_case(_mods(tag, engine=ENGINE), g, tag, first=3, before=load)
    check_trace(res, g, tag, first=3)
    for k in ('L', 'terms') + M.MOMENTS:        # bit for bit
        want = full[tag + '_' + k]
        np.testing.assert_array_equal(res[tag + '_' + k], want if k == 'Z_u0_last' else want[3:],
                                      err_msg=k)


def test_annealing_other_than_one_is_declined():
    import dgmm_svi_models as M
    g = _golden()
    Q = M.run_case(_mods('par', engine=ENGINE), g, 'par')['par_plan']
    Q.set_annealing(1.0)
    with pytest.raises(NotImplementedError, match='annealing is not built into the fused '
                                                  'DiagGaussianMixtureSVIPlan plan'):
        Q.set_annealing(0.5)
    Q['mu'].annealing = 0.5         # past VB.set_annealing: the plan declines at the step
    with pytest.raises(NotImplementedError, match='annealing is not built into the fused '
                                                  'DiagGaussianMixtureSVIPlan plan'):
        Q.gradient_step('mu', scale=0.5)


# -- the C ABI -----------------------------------------------------------------------------------------
def test_cabi_declares_the_step_and_its_host_only_entry_answers():
    """Fails without the feature: the library has no such symbols."""
    from bayespy_amd import _lib
    lib = _lib.load()
    for name in ('vmp_dgmm_natural_step', 'vmp_dgmm_natural_step_workspace'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    w = ctypes.c_int64()
    q = lib.vmp_dgmm_natural_step_workspace
    assert q(5, 3, ctypes.byref(w)) == _lib.VMP_OK and w.value == 31
    assert q(1024, 64, ctypes.byref(w)) == _lib.VMP_OK and w.value == 2 * 65536 + 1
    assert q(0, 3, ctypes.byref(w)) == _lib.VMP_ERR_INVALID
    assert q(5, 3, None) == _lib.VMP_ERR_INVALID
    assert q(1025, 3, ctypes.byref(w)) == _lib.VMP_ERR_UNSUPPORTED
    assert q(5, 65, ctypes.byref(w)) == _lib.VMP_ERR_UNSUPPORTED
    # a null context is refused before anything else is looked at: nothing is launched or written
    buf = np.zeros(64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.vmp_dgmm_natural_step(None, 2, 2, 7, p, p, p, p, p, p, p, 0, p, p, p, p, p, p, p, p,
                                     1.0, 1.0, p, p) == _lib.VMP_ERR_INVALID
    assert not buf.any()
