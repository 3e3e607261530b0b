"""CPU: the fused categorical-mixture block without a device -- the matcher and its declining
reasons one by one, the new opt-in registry beside the unchanged old ones, the plan's host logic on
the kernel double tests/cmm_host.py (CPUCMMKernels) against every fixture of tests/golden/cmm.npz
(live reference, tools/make_golden_cmm.py), masks, the g++ build of the device header
csrc/vmp_cmm_dev.h against a long-double restatement, the same source under
-fsanitize=address,undefined as a stand-alone program, a save / load round trip and the C ABI."""
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

L_RTOL = 1e-9                               # tests/test_bmm_host.py
MOM_TOL = dict(rtol=1e-6, atol=1e-9)


def _mods(after=None, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    m = dict(nodes=nodes, VB=VB, vb_kwargs=kw)
    if after is not None:
        m['after_vb'] = after
    return m


def _on_double(Q):
    from bayespy_amd.device import Runtime
    from cmm_host import CPUCMMKernels
    plan = Q.plans[0]
    assert type(plan).__name__ == 'CategoricalMixturePlan'
    rt = Runtime(device='cpu')
    plan._rt, plan._kernels = rt, CPUCMMKernels(rt)


def _golden():
    g = np.load(os.path.join(GOLDEN, 'cmm.npz'))
    gin = {k[3:]: (g[k].astype(np.int64) if k.endswith('_x') else g[k])
           for k in g.files if k.startswith('in_')}
    return g, gin


def _model(tag='e', **kw):
    from cmm_models import build_cmm
    gin = _golden()[1]
    p0 = gin[tag + '_p0']
    return build_cmm(_mods(), gin[tag + '_x'], p0.shape[1], p0.shape[2], **kw)


def _nodes(m):
    return [m['Z'], m['R'], m['X'], m['P']]


def check_fixture(res, g, cases):
    """Every stored quantity of the cases; returns how many were compared."""
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan') or k[0] not in cases:
            continue
        if k.endswith('_mask'):
            np.testing.assert_array_equal(np.broadcast_to(v, g[k].shape), g[k], err_msg=k)
        elif k.endswith('_u0'):
            np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL, atol=1e-9)
        checked += 1
    return checked


# -- the matcher and the registration ----------------------------------------------------------------
def test_matcher_accepts_the_model():
    from bayespy_amd.inference.plans.cmm import CategoricalMixturePlan
    for observe in (True, False):
        m = _model(observe=observe)
        why = []
        r = CategoricalMixturePlan.match(_nodes(m), why)
        assert r is not None and why == []
        assert r['X'] is m['X'] and r['P'] is m['P'] and r['Z'] is m['Z'] and r['R'] is m['R']
    gin = _golden()[1]
    m = _model('a', mask=gin['f_mask'])
    assert CategoricalMixturePlan.match(_nodes(m)) is not None
    m['P'].initialize_from_random()
    m['Z'].initialize_from_value(gin['a_z0'])
    assert CategoricalMixturePlan.match(_nodes(m)) is not None


def test_matcher_declines_with_reasons():
    from bayespy_amd import nodes
    from bayespy_amd.inference.plans.cmm import CategoricalMixturePlan, cmm_limits
    x = _golden()[1]['e_x']
    N, D = x.shape

    def reason(m):
        why = []
        assert CategoricalMixturePlan.match(_nodes(m), why) is None and len(why) == 1, why
        assert why[0].startswith('fused categorical-mixture block, observed node X: ')
        return why[0]

    def silent(ns):
        why = []
        assert CategoricalMixturePlan.match(ns, why) is None and why == [], why

    def build(K=2, D=D, N=N, M=2, P=None, R=None, Zkw={}, Xkw={}, mixed=nodes.Categorical):
        if R is None:
            R = nodes.Dirichlet(K * [1.0], name='R')
        Z = nodes.Categorical(R, plates=(N, 1), name='Z', **Zkw)
        if P is None:
            P = nodes.Dirichlet(M * [0.5], plates=(D, K), name='P')
        X = nodes.Mixture(Z, mixed, P, name='X', **Xkw)
        return dict(R=R, Z=Z, P=P, X=X)
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
    # a Concentration parent on P and on R
    c = nodes.Concentration(2, name='c')
    assert 'concentration of P is a node (Concentration)' in reason(
        build(P=nodes.Dirichlet(c, plates=(D, 2), name='P')))
    c = nodes.Concentration(2, name='c')
    assert 'concentration of R is a node (Concentration)' in reason(
        build(R=nodes.Dirichlet(c, name='R')))
    # other plates, cluster_plate
    assert 'plates' in reason(build(P=nodes.Dirichlet([0.5, 0.5], plates=(1, D, 2), name='P')))
    assert 'plates' in reason(build(P=nodes.Dirichlet([0.5, 0.5], plates=(2, D), name='P'),
                                    Xkw=dict(cluster_plate=-2)))
    # other children
    m = build()
    nodes.Categorical(m['P'], name='another')
    assert 'other children' in reason(m)
    # observed or value-initialised R / P beyond what the siblings accept
    m = build()
    m['R'].observe(np.array([0.5, 0.5]))
    assert 'observed' in reason(m)
    m = build()
    m['R'].initialize_from_value(np.array([0.5, 0.5]))
    assert 'R is initialised by value' in reason(m)
    m = build()
    m['Z'].initialize_from_random()
    assert 'Z is initialised by random' in reason(m)
    # Multinomial emissions
    m = build()
    m['X'].node_class = nodes.Multinomial
    assert 'Multinomial, not Categorical' in reason(m)
    # K, M and the count table above the limits; the reason states the cap
    max_K, min_M, max_M, max_cells = cmm_limits()
    assert (max_K, min_M, max_M) == (64, 2, 32) and max_cells >= 8192
    assert 'K <= 64' in reason(build(K=65))
    assert 'M <= 32' in reason(build(M=33))
    big = max_cells // (2 * 16) + 4                       # K = 2: KP = 16, four groups
    r = reason(build(D=big, N=3))
    assert 'exceed the limits' in r and '<= %d doubles' % max_cells in r
    # another family, and a hidden Markov model: nothing is said
    Rn = nodes.Dirichlet([1.0, 1.0], name='R')
    Zn = nodes.Categorical(Rn, plates=(N, 1), name='Z')
    Pn = nodes.Beta([0.5, 0.5], plates=(D, 2), name='P')
    silent([Zn, Rn, nodes.Mixture(Zn, nodes.Bernoulli, Pn, name='X'), Pn])
    a0 = nodes.Dirichlet([1.0, 1.0], name='a0')
    A = nodes.Dirichlet([1.0, 1.0], plates=(2,), name='A')
    Zc = nodes.CategoricalMarkovChain(a0, A, states=9, name='Z')
    Ph = nodes.Dirichlet([0.5, 0.5, 0.5], plates=(2,), name='P')
    silent([Zc, a0, A, nodes.Mixture(Zc, nodes.Categorical, Ph, name='Y'), Ph])


def test_the_new_registry_and_the_old_ones():
    from bayespy_amd.inference import plans
    names = lambda ps: [P.__name__ for P in ps]       # noqa: E731
    assert names(plans.OPT_IN_LAST) == ['CategoricalMixturePlan']
    assert names(plans.PLAN_TYPES) == ['PCAPlan', 'MaskedPCAPlan', 'GMMPlan', 'LSSMPlan',
                                       'MaskedLSSMPlan', 'LDAPlan']
    assert names(plans.OPT_IN_TYPES) == ['BernoulliMixturePlan', 'HMMPlan']
    assert names(plans.opt_in_types()) == ['BernoulliMixturePlan', 'HMMPlan', 'CategoricalHMMPlan']
    assert names(plans.OPT_IN_MORE) == ['DiagGaussianMixturePlan']
    assert plans.OPT_IN_FORMS == {plans.LDAPlan: plans.LDASVIPlan}
    assert plans.OPT_IN_EMISSIONS == {plans.HMMPlan: [plans.CategoricalHMMPlan]}
    assert plans.OPT_IN_AFTER == {plans.GMMPlan: [plans.GMMSVIPlan]}
    assert plans.OPT_IN_MASKED == {plans.DiagGaussianMixturePlan:
                                   [plans.MaskedDiagGaussianMixturePlan]}


def test_default_engine_keeps_the_generic_plan():
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.plans.cmm import CategoricalMixturePlan
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
        assert isinstance(fused[0], CategoricalMixturePlan)
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
    assert type(Q.plans[0]).__name__ == 'CategoricalMixturePlan'
    m = _model()
    m['X'].observe(_golden()[1]['e_x'], mask=False)
    with pytest.raises(NotImplementedError, match='fused categorical-mixture block.*mask'):
        VB(*_nodes(m), engine='fused')
    assert all(n._plan is None for n in _nodes(m))


# -- the plan on the kernel double ---------------------------------------------------------------------
def test_plan_reproduces_every_fixture_on_the_kernel_double():
    from cmm_models import run_cmm_cases, CASES
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_cmm_cases(_mods(_on_double, engine='fused'), gin)
    assert check_fixture(res, g, CASES) == len(CASES) * (1 + 4 + 3 + 2)
    calls = res['a_plan'].plans[0].kernels.calls
    # set-up pass + one per sweep; the responsibilities only on request
    assert calls.count('pass') == 1 + 4 and calls.count('pass_r') == 1 and calls.count('pack') == 1
    # a mask of ones: the bits of the unmasked run
    for k in ('L', 'Z_u0', 'P_u0', 'R_u0', 'Z_Lterm'):
        np.testing.assert_array_equal(res['g_' + k], res['a_' + k], err_msg=k)
    # (f): the row of nothing has softmax(<log pi>) and its column of P stays at the prior
    plan = res['f_plan'].plans[0]
    c = plan.c.numpy()                    # of the last Z update, which R's update followed
    np.testing.assert_allclose(res['f_Z_u0'][4, 0], np.exp(c) / np.exp(c).sum(), rtol=1e-12)
    S = plan.S.numpy().reshape(5, 7, 3)
    assert np.all(S[:, 2] == 0)
    np.testing.assert_array_equal(plan.alpha_p.numpy().reshape(5, 7, 3)[:, 2],
                                  np.broadcast_to(gin['a_conc'][:, None], (5, 3)))


def test_hidden_values_are_never_interpreted_and_reobserving_keeps_the_posteriors():
    from cmm_models import run_cmm_cases
    g, gin = _golden()
    Q = run_cmm_cases(_mods(_on_double, engine='fused'), gin, only=('f',))['f_plan']
    plan = Q.plans[0]
    X, P = Q['X'], Q['P']
    p = P.get_moments()[0]
    S0, xb0 = plan.S.numpy().copy(), plan.xb.numpy().copy()
    mask = gin['f_mask']
    junk = np.where(mask, gin['a_x'], np.nan).astype(np.float64)
    junk[~mask] = np.resize([np.nan, -1.0, 1e300], int((~mask).sum()))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        X._data, X._mask = junk, mask           # past the host check of observe, as a tensor is
        plan.invalidate(X)
        np.testing.assert_array_equal(P.get_moments()[0], p)
    assert Q.plans[0] is plan
    np.testing.assert_array_equal(plan.xb.numpy(), xb0)
    np.testing.assert_array_equal(plan.S.numpy(), S0)
    # another mask of the full shape: packed again, the posteriors stay
    m2 = mask.copy()
    m2[4] = True
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        X.observe(gin['a_x'], mask=m2)
        np.testing.assert_array_equal(P.get_moments()[0], p)
    assert Q.plans[0] is plan and plan.kernels.calls.count('pack') == 3
    assert bool(Q['Z'].mask[4, 0]) is True


def test_invalid_category_raises_the_reference_exception():
    from bayespy_amd.inference import VB
    _, gin = _golden()
    for bad in (2, -1, 0.5):
        m = _model()
        Q = VB(*_nodes(m), engine='fused')
        _on_double(Q)
        x = gin['e_x'].astype(np.float64)
        x[3, 4] = bad
        m['X']._data = x
        with pytest.raises(ValueError, match='Invalid category index'):
            Q.update(verbose=False)


def test_parameters_and_random_initialisation_of_P():
    from scipy import special
    from bayespy_amd.inference import VB
    _, gin = _golden()
    D, K, M = 6, 2, 2
    a = np.random.RandomState(3).gamma(2.0, size=(D, K, M))
    m = _model()
    m['P'].initialize_from_parameters(a)
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    np.testing.assert_allclose(m['P'].get_moments()[0],
                               special.digamma(a) - special.digamma(a.sum(-1, keepdims=True)),
                               rtol=1e-12)
    assert np.isfinite(Q.compute_lowerbound())
    m = _model()
    m['P'].initialize_from_random()
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    e = m['P'].get_moments()[0]
    assert e.shape == (D, K, M)
    np.testing.assert_allclose(np.exp(e).sum(-1), 1.0, rtol=1e-12)      # a point mass
    Q.update(repeat=2, verbose=False)
    assert np.all(np.isfinite(Q.L[:2]))


def test_save_load_round_trip_and_a_differing_mask_is_refused(tmp_path):
    from cmm_models import run_cmm_cases
    g, gin = _golden()
    Q = run_cmm_cases(_mods(_on_double, engine='fused'), gin, only=('f',))['f_plan']
    fn = str(tmp_path / 'cmm.ckpt')
    Q.save(filename=fn)
    L4 = Q.L[:4].copy()
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    assert Q.iter == 4
    np.testing.assert_array_equal(Q.L[:4], L4)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)
    other = run_cmm_cases(_mods(_on_double, engine='fused'), gin, only=('a',))['a_plan']
    with pytest.raises(ValueError, match='checkpoint was saved with a mask on X'):
        other.load(filename=fn)


# -- the device header on the host ---------------------------------------------------------------------
def test_pack_dtypes_hidden_values_and_the_flag():
    from cmm_host import host_pack, restate_pack, HIDDEN
    rs = np.random.RandomState(7)
    M = 5
    x = rs.randint(M, size=(37, 9))
    mask = rs.rand(37, 9) < 0.7
    for a in (x.astype(np.int64), x.astype(np.float64), x.astype(np.int32), x.astype(np.uint8)):
        xb, flag = host_pack(a, M)
        assert flag == 0
        np.testing.assert_array_equal(xb, x)
        xb, flag = host_pack(a, M, mask)
        assert flag == 0
        np.testing.assert_array_equal(xb, np.where(mask, x, HIDDEN))
        np.testing.assert_array_equal(restate_pack(a, M, mask)[0], xb)
    mask[5, 8], mask[6, 8] = True, False
    want = np.where(mask, x, HIDDEN)
    for v in (np.nan, -1.0, 1e300, 0.5, 5.0, np.inf):
        hidden = x.astype(np.float64)
        hidden[6, 8] = v
        xb, flag = host_pack(hidden, M, mask)
        assert flag == 0
        np.testing.assert_array_equal(xb, want)
        bad = x.astype(np.float64)
        bad[5, 8] = v
        xb, flag = host_pack(bad, M, mask)
        assert flag == 1 and xb[5, 8] == HIDDEN
        assert restate_pack(bad, M, mask)[1] == 1
    for v in (-1, 5, 2 ** 40, -2 ** 40):
        bad = x.astype(np.int64)
        bad[5, 8] = v
        xb, flag = host_pack(bad, M, mask)
        assert flag == 1 and xb[5, 8] == HIDDEN


SHAPES = [(0, 5, 3, 4), (1, 1, 1, 2), (65, 3, 2, 3), (300, 7, 15, 5), (257, 4, 16, 5),
          (515, 17, 17, 2), (300, 5, 33, 32), (763, 7, 64, 32)]


@pytest.mark.parametrize('N,D,K,M', SHAPES)
def test_host_build_of_the_device_header_against_long_double(N, D, K, M):
    """The rule of DESIGN 4.14: the host build may differ from the long-double restatement by 8
    times the deviation of the plain float64 evaluation, floor 4 ulp of the magnitude."""
    from cmm_host import (host_pack, host_pass, host_tables, restate, restate_tables, tolerances,
                          error, mixed_mask, pass_inputs, QUANTITIES, cmm_host)
    x, L, c, rs = pass_inputs(N, D, K, M)
    assert cmm_host().cmm_chunk_rows(N, D, K, M) == 256
    for mask in (None, mixed_mask(N, D, rs)):
        xb, flag = host_pack(x, M, mask)
        assert flag == 0
        got = host_pass(N, D, K, M, xb, None, L, c, want_r=True)
        ld, f64 = restate(x, mask, L, c), restate(x, mask, L, c, np.float64)
        tol, dev = tolerances(ld, f64)
        for key in QUANTITIES:
            err = error(got[key], ld[key])
            assert err <= tol[key], (key, err, tol[key])
        if N:
            assert got['r'].max() < 0.999 or K == 1          # soft rows
        # fixed labels: one-hot statistics, lse = 0
        lab = rs.randint(K, size=N).astype(np.int32)
        h = host_pass(N, D, K, M, xb, lab, L, c, want_r=True)
        m = np.ones((N, D), dtype=bool) if mask is None else mask
        one = np.eye(K)[lab] * m.any(axis=1)[:, None]
        np.testing.assert_array_equal(h['Nk'], one.sum(0))
        onehot = ((x[:, :, None] == np.arange(M)) & m[:, :, None]).astype(float)
        np.testing.assert_array_equal(h['S'], np.einsum('ndm,nk->mdk', onehot, one))
        assert h['sum_lse'] == 0
    # a mask of ones gives the bits of no mask
    a = host_pass(N, D, K, M, host_pack(x, M)[0], None, L, c, want_r=True)
    b = host_pass(N, D, K, M, host_pack(x, M, np.ones((N, D)))[0], None, L, c, want_r=True)
    for key in QUANTITIES:
        np.testing.assert_array_equal(a[key], b[key])
    # tables
    elog_pi = rs.normal(size=K) - 1e5
    for ep in (None, L):
        Lh, ch = host_tables(D, K, M, ep, elog_pi)
        Lr, cr = restate_tables(ep, elog_pi, (M, D * K))
        np.testing.assert_array_equal(Lh, Lr)
        np.testing.assert_array_equal(ch, cr)


def test_limits_lds_budget_chunks_and_workspace():
    from cmm_host import cmm_host
    lib = cmm_host()
    cap = lib.cmm_max_cells()
    assert cap >= 8192
    worst = 0
    for K in (1, 16, 17, 32, 33, 64):
        KP, G = lib.cmm_kpad(K), 64 // lib.cmm_kpad(K)
        for M in range(2, 33):
            D = cap // (M * KP) // G * G          # the largest D of this (K, M)
            if D < 1:
                assert not lib.cmm_supported(1, K, M)
                continue
            assert lib.cmm_supported(D, K, M) and lib.cmm_cells(D, K, M) <= cap
            assert not lib.cmm_supported(D + 1, K, M)
            worst = max(worst, lib.cmm_lds_bytes(D, K, M))
    assert worst <= 160 * 1024                    # the LDS of a CU
    assert lib.cmm_supported(7, 64, 32) and lib.cmm_cells(7, 64, 32) == cap
    assert not lib.cmm_supported(8, 64, 32)
    assert not lib.cmm_supported(4, 65, 4) and not lib.cmm_supported(4, 4, 33)
    assert not lib.cmm_supported(4, 4, 1)
    for N, D, K, M in ((0, 1, 1, 2), (10 ** 7, 32, 32, 8), (10 ** 9, 7, 64, 32), (257, 3, 2, 2)):
        rows, nc = lib.cmm_chunk_rows(N, D, K, M), lib.cmm_chunks(N, D, K, M)
        assert rows % 64 == 0 and rows >= 256 and nc <= 1024
        assert nc * rows >= N and (nc == 0 or (nc - 1) * rows < N)
        assert nc * lib.cmm_partial_doubles(D, K, M) * 8 <= 2 ** 28


def test_sanitized_stand_alone_program():
    """tests/host/cmm_host_main.cpp under -fsanitize=address,undefined, never loaded into Python."""
    from cmm_host import build_sanitized_program
    exe = build_sanitized_program()
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.count('flag=0') == 4 and 'runtime error' not in out.stdout


# -- the C ABI -----------------------------------------------------------------------------------------
def test_cabi_declares_the_cmm_entry_points():
    """Fails without the feature: the library has no such symbols."""
    from bayespy_amd import _lib
    from cmm_host import cmm_host
    lib = _lib.load()
    for name in ('vmp_cmm_limits', 'vmp_cmm_plan', 'vmp_cmm_pack', 'vmp_cmm_tables',
                 'vmp_cmm_pass'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    host = cmm_host()
    v = [ctypes.c_int32() for _ in range(4)]
    assert lib.vmp_cmm_limits(*[ctypes.byref(a) for a in v]) == _lib.VMP_OK
    assert tuple(a.value for a in v) == (host.cmm_max_k(), host.cmm_min_m(), host.cmm_max_m(),
                                         host.cmm_max_cells())
    assert lib.vmp_cmm_limits(None, None, None, None) == _lib.VMP_ERR_INVALID
    c, w = ctypes.c_int64(), ctypes.c_int64()
    for N, D, K, M in ((0, 1, 1, 2), (1000, 7, 5, 5), (10 ** 7, 32, 32, 8), (10 ** 6, 7, 64, 32)):
        assert lib.vmp_cmm_plan(N, D, K, M, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_OK
        assert c.value == host.cmm_chunk_rows(N, D, K, M)
        assert w.value == host.cmm_chunks(N, D, K, M) * host.cmm_partial_doubles(D, K, M) + 1024
    for D, K, M in ((4, 65, 4), (4, 4, 33), (4, 4, 1), (8, 64, 32)):
        assert lib.vmp_cmm_plan(10, D, K, M, ctypes.byref(c), ctypes.byref(w)) \
            == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_cmm_plan(-1, 4, 4, 4, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_ERR_INVALID
    assert lib.vmp_cmm_plan(10, 4, 4, 4, None, None) == _lib.VMP_ERR_INVALID
