"""CPU: the fused Bernoulli-mixture block without a device -- the matcher and its declining
reasons, the opt-in registration, the plan's host logic on the kernel double tests/bmm_host.py
(CPUBMMKernels) against every fixture of tests/golden/bmm_fused.npz (live reference,
tools/make_golden_bmm.py) and the bmm.rst doctest, the g++ build of the device header
csrc/vmp_bmm_dev.h against a long-double restatement, a save / load round trip and the C ABI."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

L_RTOL = 1e-9                               # tests/test_generic_engine_gpu.py on the same data
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
    from bmm_host import CPUBMMKernels
    plan = Q.plans[0]
    assert type(plan).__name__ == 'BernoulliMixturePlan'
    rt = Runtime(device='cpu')
    plan._rt, plan._kernels = rt, CPUBMMKernels(rt)


def _golden():
    g = np.load(os.path.join(GOLDEN, 'bmm_fused.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


def _model(x=None, K=3, **kw):
    from bmm_models import build_bmm
    if x is None:
        x = _golden()[1]['e_x']
    return build_bmm(_mods(), x, K, **kw)


def _nodes(m):
    return [m['Z'], m['R'], m['X'], m['P']]


# -- the matcher and the registration ----------------------------------------------------------------
def test_matcher_accepts_the_doc_graph():
    from bayespy_amd.inference.plans.bmm import BernoulliMixturePlan
    for observe in (True, False):       # bmm.rst observes after VB(...)
        m = _model(observe=observe)
        why = []
        r = BernoulliMixturePlan.match(_nodes(m), why)
        assert r is not None and why == []
        assert r['X'] is m['X'] and r['P'] is m['P'] and r['Z'] is m['Z'] and r['R'] is m['R']


def test_matcher_declines_with_reasons():
    from bayespy_amd import nodes
    from bayespy_amd.inference.plans.bmm import BernoulliMixturePlan
    x = _golden()[1]['e_x']
    N, D = x.shape

    def reason(m):
        why = []
        assert BernoulliMixturePlan.match(_nodes(m), why) is None and len(why) == 1, why
        return why[0]

    def build(K=2, D=D, N=N, P=None, Zkw={}, mixed=nodes.Bernoulli, extra=()):
        R = nodes.Dirichlet(K * [1.0], name='R')
        Z = nodes.Categorical(R, plates=(N, 1), name='Z', **Zkw)
        if P is None:
            P = nodes.Beta([0.5, 0.5], plates=(D, K), name='P')
        X = nodes.Mixture(Z, mixed, *(tuple(extra) + (P,)), name='X')
        return dict(R=R, Z=Z, P=P, X=X)
    # a mask
    m = build()
    m['X'].observe(x, mask=(np.arange(N) % 2 == 0)[:, None])
    assert 'mask' in reason(m)
    # Binomial observations
    # (Mixture takes every positional argument of Binomial for a parent, so the mixed class of a
    # built node is exchanged here)
    m = build()
    m['X'].node_class = nodes.Binomial
    assert 'Binomial, not Bernoulli' in reason(m)
    # a BetaConcentration parent
    c = nodes.BetaConcentration(name='c')
    assert 'is a node (Concentration)' in reason(build(P=nodes.Beta(c, plates=(D, 2), name='P')))
    # the limits
    assert 'exceed the limits' in reason(build(K=65))
    assert 'exceed the limits' in reason(build(D=1025))
    # a second child of P
    m = build()
    nodes.Bernoulli(m['P'], name='another')
    assert 'other children' in reason(m)
    # plates_multiplier
    assert 'plates_multiplier' in reason(build(Zkw=dict(plates_multiplier=(2.5, 1))))
    # an initialisation the block does not take
    m = build()
    m['Z'].initialize_from_random()
    assert 'initialised by random' in reason(m)


def test_default_engine_keeps_the_generic_plan():
    from bayespy_amd.inference import plans
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.plans.bmm import BernoulliMixturePlan
    from bayespy_amd.inference.plans.hmm import HMMPlan
    assert [P.__name__ for P in plans.PLAN_TYPES] == [
        'PCAPlan', 'MaskedPCAPlan', 'GMMPlan', 'LSSMPlan', 'MaskedLSSMPlan', 'LDAPlan']
    assert plans.OPT_IN_TYPES == [BernoulliMixturePlan, HMMPlan]
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
        assert isinstance(fused[0], BernoulliMixturePlan)
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
    assert type(Q.plans[0]).__name__ == 'BernoulliMixturePlan'
    m = _model()
    m['X'].observe(_golden()[1]['e_x'], mask=False)
    with pytest.raises(NotImplementedError, match='fused Bernoulli-mixture block.*mask'):
        VB(*_nodes(m), engine='fused')
    assert all(n._plan is None for n in _nodes(m))


# -- the plan on the kernel double ---------------------------------------------------------------------
def test_plan_reproduces_every_fixture_on_the_kernel_double():
    from bmm_models import run_bmm_cases, CASES
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_bmm_cases(_mods(_on_double, engine='fused'), gin)
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan'):
            continue
        if k.endswith('_u0'):
            np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL, atol=1e-9)
        checked += 1
    assert checked == len(CASES) * (1 + 4 + 3)
    calls = res['a_plan'].plans[0].kernels.calls
    # set-up pass + one per sweep; the responsibilities only on request
    assert calls.count('pass') == 1 + 4 and calls.count('pass_r') == 1 and calls.count('pack') == 1


def test_doctest_known_answer_on_the_kernel_double():
    """doc/source/examples/bmm.rst with engine='fused': the printed first and last loglike."""
    from bayespy_amd.nodes import Categorical, Dirichlet, Beta, Mixture, Bernoulli
    from bayespy_amd.inference import VB
    g = np.load(os.path.join(GOLDEN, 'bmm_doctest.npz'))
    N, D, K = 100, 10, 10
    R = Dirichlet(K * [1e-5], name='R')
    Z = Categorical(R, plates=(N, 1), name='Z')
    P = Beta([0.5, 0.5], plates=(D, K), name='P')
    X = Mixture(Z, Bernoulli, P)
    Q = VB(Z, R, X, P, engine='fused')
    _on_double(Q)
    P.initialize_from_value(g['p_init'])
    X.observe(g['x'])
    plan = Q.plans[0]
    Q.update(repeat=1000, verbose=False)
    assert Q.plans[0] is plan
    L = Q.L[:Q.iter]
    assert '%e' % L[0] == '-6.872145e+02'
    assert Q.iter == 17 and '%e' % L[-1] == '-5.236921e+02'
    np.testing.assert_allclose(L, g['L'], rtol=L_RTOL)
    np.testing.assert_allclose(R.u[0], g['R_u0'], rtol=1e-6)
    np.testing.assert_allclose(P.u[0], g['P_u0'], rtol=1e-6, atol=1e-9)


def test_count_nodes_fixture_with_per_node_terms():
    """The bmm_* keys of tests/golden/count_nodes.npz (tests/models.py case 4)."""
    g = np.load(os.path.join(GOLDEN, 'count_nodes.npz'))
    from bayespy_amd import nodes as N_
    from bayespy_amd.inference import VB
    x, p0 = g['in_bmm_x'], g['in_bmm_p0']
    N, D = x.shape
    K = p0.shape[1]
    R = N_.Dirichlet(K * [1e-5], name='R')
    Z = N_.Categorical(R, plates=(N, 1), name='Z')
    P = N_.Beta([0.5, 0.5], plates=(D, K), name='P')
    X = N_.Mixture(Z, N_.Bernoulli, P, name='X')
    Q = VB(Z, R, X, P, engine='fused')
    _on_double(Q)
    P.initialize_from_value(p0)
    X.observe(x)
    Q.ignore_bound_checks = True
    Q.update(repeat=6, verbose=False)
    np.testing.assert_allclose(Q.L[:6], g['bmm_L'], rtol=L_RTOL)
    for nm, nd in dict(R=R, P=P, Z=Z).items():
        np.testing.assert_allclose(Q.l[nd][:6], g['bmm_%s_Lterm' % nm], rtol=L_RTOL, atol=1e-9)
        np.testing.assert_allclose(nd.u[0], g['bmm_%s_u_0' % nm], err_msg=nm, **MOM_TOL)


def test_parameters_and_random_initialisation_of_P():
    from scipy import special
    from bayespy_amd.inference import VB
    g, gin = _golden()
    x = gin['e_x']
    D = x.shape[1]
    a = np.random.RandomState(3).gamma(2.0, size=(D, 2, 2))
    m = _model(x, 2)
    m['P'].initialize_from_parameters(a)
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    np.testing.assert_allclose(m['P'].get_moments()[0],
                               special.digamma(a) - special.digamma(a.sum(-1, keepdims=True)),
                               rtol=1e-12)
    assert np.isfinite(Q.compute_lowerbound())
    m = _model(x, 2)
    m['P'].initialize_from_random()
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    e = m['P'].get_moments()[0]
    np.testing.assert_allclose(np.exp(e).sum(-1), 1.0, rtol=1e-12)      # a point mass
    assert Q.compute_lowerbound() == -np.inf
    Q.update(repeat=2, verbose=False)
    assert np.all(np.isfinite(Q.L[:2]))


def test_non_binary_observation_raises_the_reference_exception():
    from bayespy_amd.inference import VB
    _, gin = _golden()
    x = gin['e_x'].copy()
    bad = x.copy()
    bad[3, 4] = 2
    m = _model(x, 2)
    with pytest.raises(ValueError, match='Invalid count'):
        m['X'].observe(bad)                         # host arrays: Bernoulli's own check
    # a value that reaches the block unchecked (a device tensor does): the flag of the pack entry
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    m['X']._data = bad
    with pytest.raises(ValueError, match='Invalid count'):
        Q.update(verbose=False)


def test_save_load_round_trip_on_the_double(tmp_path):
    from bmm_models import run_bmm_cases
    g, gin = _golden()
    Q = run_bmm_cases(_mods(_on_double, engine='fused'), gin, only=('e',))['e_plan']
    fn = str(tmp_path / 'bmm.ckpt')
    Q.save(filename=fn)
    L4 = Q.L[:4].copy()
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    assert Q.iter == 4
    np.testing.assert_array_equal(Q.L[:4], L4)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)


def test_reobserve_repacks_and_keeps_the_posteriors():
    from bmm_models import run_bmm_cases
    g, gin = _golden()
    Q = run_bmm_cases(_mods(_on_double, engine='fused'), gin, only=('e',))['e_plan']
    plan = Q.plans[0]
    X, P = Q['X'], Q['P']
    p = P.get_moments()[0]
    S0 = plan.S.numpy().copy()
    perm = np.random.RandomState(0).permutation(gin['e_x'].shape[0])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        X.observe(gin['e_x'][perm].astype(bool))
    assert Q.plans[0] is plan
    np.testing.assert_array_equal(P.get_moments()[0], p)
    # the same multiset of rows: the same statistics up to the order of the additions
    np.testing.assert_allclose(plan.S.numpy(), S0, rtol=1e-12, atol=1e-13)
    assert plan.kernels.calls.count('pack') == 2


# -- the device header on the host ---------------------------------------------------------------------
@pytest.mark.parametrize('D', [63, 64, 65])
def test_pack_and_unpack(D):
    from bmm_host import host_pack, host_unpack, bmm_host
    rs = np.random.RandomState(D)
    x = rs.randint(2, size=(37, D))
    x[0], x[1] = 0, 1
    for a in (x.astype(np.int64), x.astype(np.float64), x.astype(bool)):
        xw, flag = host_pack(a)
        assert flag == 0 and xw.shape == (37, bmm_host().bmm_words(D)) == (37, (D + 63) // 64)
        np.testing.assert_array_equal(host_unpack(xw, D), x)
        if D % 64:
            assert not np.any(xw[:, -1] >> np.uint64(D % 64))         # unused high bits are zero
    for v in (2, -1, 0.5, np.nan):
        b = x.astype(np.float64)
        b[5, D - 1] = v
        assert host_pack(b)[1] == 1


@pytest.mark.parametrize('N,D,K', [(0, 5, 3), (1, 1, 1), (65, 63, 2), (300, 65, 15), (257, 64, 16),
                                   (515, 70, 17), (763, 257, 64)])
def test_host_build_of_the_device_header_against_long_double(N, D, K):
    """The host build may differ from a long-double restatement by the rounding of its own float64
    steps.  The float64 NumPy evaluation of the same formulas (the reference's arithmetic) differs
    from long double by roundings of the same kind in another order of additions: 8 times its
    deviation, with a floor of 4 ulp of the quantity's magnitude, bounds the host build."""
    from bmm_host import host_pack, host_pass, restate, bmm_host
    rs = np.random.RandomState(N + D + K)
    assert bmm_host().bmm_chunk_rows(N, D, K) == 256
    x = rs.randint(2, size=(N, D)).astype(np.int64)
    w = rs.normal(size=(D, K))
    c = rs.normal(size=K) - 0.7 * D
    xw, _ = host_pack(x)
    S, Nk, counts, sl, r = host_pass(N, D, K, xw, None, w, c, want_r=True)
    ld, f64 = restate(x, w, c), restate(x, w, c, np.float64)
    got = dict(r=r, Nk=Nk, S=S, sum_lse=sl)
    for key, val in got.items():
        ref = np.asarray(ld[key], dtype=np.longdouble)
        dev = np.max(np.abs(np.asarray(f64[key], dtype=np.longdouble) - ref)) if ref.size else 0.0
        mag = float(np.max(np.abs(ref))) if ref.size else 0.0
        tol = max(8 * float(dev), 4 * np.spacing(mag))
        err = float(np.max(np.abs(val - ref))) if ref.size else 0.0
        assert err <= tol, (key, err, tol)
    np.testing.assert_array_equal(counts[:, 0], S.reshape(-1))
    np.testing.assert_array_equal(counts[:, 1], (Nk[None, :] - S).reshape(-1))
    # fixed labels: one-hot statistics, lse = 0
    lab = rs.randint(K, size=N).astype(np.int32)
    S, Nk, _, sl, r = host_pass(N, D, K, xw, lab, w, c, want_r=True)
    np.testing.assert_array_equal(Nk, np.bincount(lab, minlength=K))
    np.testing.assert_array_equal(S, x.T @ np.eye(K)[lab])
    assert sl == 0


def test_chunk_rows_and_workspace_stay_bounded():
    from bmm_host import bmm_host
    lib = bmm_host()
    for N, D, K in ((0, 1, 1), (10 ** 7, 64, 32), (10 ** 6, 1024, 64), (10 ** 9, 1024, 64),
                    (10 ** 5, 64, 32), (257, 3, 2)):
        rows, nc = lib.bmm_chunk_rows(N, D, K), lib.bmm_chunks(N, D, K)
        assert rows % 64 == 0 and rows >= 256 and nc <= 1024
        assert nc * rows >= N and (nc == 0 or (nc - 1) * rows < N)
        assert nc * lib.bmm_partial_doubles(D, K) * 8 <= 2 ** 28


# -- the C ABI -----------------------------------------------------------------------------------------
def test_cabi_declares_the_bmm_entry_points():
    """Fails without the feature: the library has no such symbols."""
    from bayespy_amd import _lib
    from bmm_host import bmm_host
    lib = _lib.load()
    for name in ('vmp_bmm_limits', 'vmp_bmm_plan', 'vmp_bmm_pack', 'vmp_bmm_tables',
                 'vmp_bmm_pass'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    mk, md = ctypes.c_int32(), ctypes.c_int32()
    assert lib.vmp_bmm_limits(ctypes.byref(mk), ctypes.byref(md)) == _lib.VMP_OK
    from bayespy_amd.inference.plans.bmm import BMM_MAX_K, BMM_MAX_D
    assert (mk.value, md.value) == (BMM_MAX_K, BMM_MAX_D) == (64, 1024)
    assert lib.vmp_bmm_limits(None, None) == _lib.VMP_ERR_INVALID
    host = bmm_host()
    c, w = ctypes.c_int64(), ctypes.c_int64()
    for N, D, K in ((0, 1, 1), (1000, 70, 5), (10 ** 7, 64, 32), (10 ** 6, 1024, 64)):
        assert lib.vmp_bmm_plan(N, D, K, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_OK
        assert c.value == host.bmm_chunk_rows(N, D, K)
        assert w.value == host.bmm_chunks(N, D, K) * host.bmm_partial_doubles(D, K) + 1024
    assert lib.vmp_bmm_plan(10, 4, 65, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_bmm_plan(10, 1025, 4, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_bmm_plan(-1, 4, 4, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_plan(10, 4, 4, None, None) == _lib.VMP_ERR_INVALID
