"""CPU: the fused hidden-Markov-model block without a device -- the matcher and its declining
reasons, the opt-in registration, the plan's host logic on the kernel double
tests/hmm_fused_host.py (CPUHMMKernels) against every fixture of tests/golden/hmm_fused.npz (live
reference, tools/make_golden_hmm.py) and hmm.rst's known answer (the hmm2 case of
tests/golden/markov_chains.npz), the g++ build of the device header csrc/vmp_hmm_fused_dev.h
against a long-double restatement, a save / load round trip and the C ABI."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

L_RTOL = 1e-9                               # tests/test_bmm_host.py on the same kind of data
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
    from hmm_fused_host import CPUHMMKernels
    plan = Q.plans[0]
    assert type(plan).__name__ == 'HMMPlan'
    rt = Runtime(device='cpu')
    plan._rt, plan._kernels = rt, CPUHMMKernels(rt)


def _golden():
    g = np.load(os.path.join(GOLDEN, 'hmm_fused.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


def _model(tag='a', **kw):
    from hmm_models import build_hmm
    gin = _golden()[1]
    return build_hmm(_mods(), gin[tag + '_y'], gin[tag + '_mu'], gin[tag + '_Lambda'], **kw)


def _nodes(m):
    from bayespy_amd.nodes.node import Constant
    return [m['Y'], m['Z'], m['A'], m['a0']] + [m[k] for k in ('mu', 'Lambda')
                                                if k in m and not isinstance(m[k], Constant)
                                                and hasattr(m[k], 'parents')]


# -- the matcher and the registration ----------------------------------------------------------------
def test_matcher_accepts_both_emission_forms():
    from bayespy_amd.inference.plans.hmm import HMMPlan
    for tag in ('a', 'b', 'e', 'f'):        # plates () and (B,); Lambda (D, D) and (K, D, D); nodes
        for observe in (True, False):
            m = _model(tag, observe=observe, learned=tag in 'ef')
            why = []
            r = HMMPlan.match(_nodes(m), why)
            assert r is not None and why == []
            assert r['Y'] is m['Y'] and r['Z'] is m['Z'] and r['A'] is m['A'] and r['a0'] is m['a0']
            assert ('mu' in r) == (tag in 'ef')
            if tag in 'ef':
                assert r['mu'] is m['mu'] and r['Lambda'] is m['Lambda']
                assert len(_nodes(m)) == 6


def test_matcher_declines_with_reasons():
    from bayespy_amd import nodes as N_
    from bayespy_amd.inference.plans.hmm import HMMPlan
    gin = _golden()[1]
    y, mu, Lam = gin['b_y'], gin['b_mu'], gin['b_Lambda']
    B, T, D = y.shape
    K = len(mu)

    def reason(m):
        why = []
        assert HMMPlan.match(_nodes(m), why) is None and len(why) == 1, why
        return why[0]

    def build(a0=None, A=None, mu=mu, Lam=Lam, mixed=N_.Gaussian, K=K, Zkw={}):
        a0 = N_.Dirichlet(np.ones(K), name='a0') if a0 is None else a0
        A = N_.Dirichlet(np.ones((K, K)), name='A') if A is None else A
        Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z', **Zkw)
        Y = N_.Mixture(Z, mixed, mu, *(() if Lam is None else (Lam,)), name='Y')
        return dict(a0=a0, A=A, Z=Z, Y=Y, mu=mu, Lambda=Lam)

    def learned():
        return dict(mu=N_.GaussianARD(0, 1e-2, shape=(D,), plates=(K,), name='mu'),
                    Lam=N_.Wishart(D + 1.0, np.identity(D), plates=(K,), name='Lambda'))
    # a mask
    m = build()
    m['Y'].observe(y, mask=(np.arange(T) % 2 == 0))
    assert 'mask' in reason(m)
    # a concentration that is a node
    c = N_.DirichletConcentration(K, name='c')
    assert 'concentration of a0 is a node' in reason(build(a0=N_.Dirichlet(c, name='a0')))
    # A with a time plate (the hmm3 form of tests/models.py), a0 with plates
    assert 'A has plates' in reason(build(A=N_.Dirichlet(np.ones((T - 1, K, K)), name='A')))
    assert 'a0 has plates' in reason(build(a0=N_.Dirichlet(np.ones(K), plates=(B,), name='a0')))
    # other emissions
    m = build(mu=N_.GaussianARD(0, 1e-2, plates=(K,), name='m'),
              Lam=N_.Gamma(1e-1, 1e-1, plates=(K,), name='t'), mixed=N_.GaussianARD)
    assert 'GaussianARD, not Gaussian' in reason(m)
    m = build(mu=np.full((K, 3), 1.0 / 3), Lam=None, mixed=N_.Categorical)
    assert 'Categorical, not Gaussian' in reason(m)
    m = build(mu=np.ones(K), Lam=np.ones(K), mixed=N_.Gamma)
    assert 'Gamma, not Gaussian' in reason(m)
    # form (b) with other priors or states of mu and Lambda
    assert 'takes two constants or' in reason(build(mu=learned()['mu']))
    m = build(**dict(learned(), mu=N_.GaussianARD(1.0, 1e-2, shape=(D,), plates=(K,), name='mu')))
    assert 'prior of the means' in reason(m)
    m = build(**learned())
    m['mu'].initialize_from_value(np.zeros((K, D)))
    assert 'mu is initialised by value' in reason(m)
    m = build(**learned())
    m['Lambda'].observe(np.tile(np.identity(D), (K, 1, 1)))
    assert 'mu or Lambda is observed' in reason(m)
    # plates_multiplier, a sharded plate
    assert 'plates_multiplier' in reason(build(Zkw=dict(plates_multiplier=(2.5,))))
    m = build()
    m['Z'].shard(0)
    assert 'sharded' in reason(m)
    # observed or initialised parents
    m = build()
    m['A'].initialize_from_value(np.full((K, K), 1.0 / K))
    assert 'A is initialised by value' in reason(m)
    m = build()
    m['a0'].observe(np.full(K, 1.0 / K))
    assert 'a0 or A is observed' in reason(m)
    m = build()
    m['A'].observe(np.full((K, K), 1.0 / K))
    assert 'a0 or A is observed' in reason(m)
    # T < 2 (the node's constructor refuses it, so the attribute of a built chain is changed)
    m = build()
    m['Z'].states = 1
    assert 'T = 1 < 2' in reason(m)
    # a second child
    m = build()
    N_.CategoricalMarkovChain(m['a0'], np.full((K, K), 1.0 / K), states=3, name='other')
    assert 'other children' in reason(m)
    # the limits
    assert 'exceed the limits' in reason(build(K=65, mu=np.zeros((65, D)), Lam=np.identity(D)))
    assert 'exceed the limits' in reason(build(mu=np.zeros((K, 9)), Lam=np.identity(9)))


def test_block_is_opt_in():
    from bayespy_amd.inference import plans
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.plans.hmm import HMMPlan
    assert HMMPlan not in plans.PLAN_TYPES and HMMPlan in plans.OPT_IN_TYPES
    import host_generic
    m = _model()
    host_generic.install()
    try:
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            got = compile_model(_nodes(m))
        assert len(got) == 1 and isinstance(got[0], GenericPlan)
        fused = compile_model(_nodes(m), engine='fused')
        assert isinstance(fused[0], HMMPlan)
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
    assert type(Q.plans[0]).__name__ == 'HMMPlan'
    m = _model()
    m['Y'].observe(_golden()[1]['a_y'], mask=False)
    with pytest.raises(NotImplementedError, match='fused hidden-Markov-model block.*mask'):
        VB(*_nodes(m), engine='fused')
    assert all(n._plan is None for n in _nodes(m))


# -- the plan on the kernel double ---------------------------------------------------------------------
def check_fixtures(res, g):
    from hmm_models import CASES, LEARNED
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan'):
            continue
        if '_u' in k:
            np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL, atol=1e-9)
        checked += 1
    assert checked == len(CASES) * (1 + 4 + 4) + len(LEARNED) * (1 + 6 + 8)


def test_plan_reproduces_every_fixture_on_the_kernel_double():
    from hmm_models import run_hmm_cases
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_hmm_cases(_mods(_on_double, engine='fused'), gin)
    check_fixtures(res, g)
    calls = res['a_plan'].plans[0].kernels.calls
    # set-up pass + one per sweep; gamma, z0 and zz only on request
    assert calls.count('pass') == 1 + 4 and calls.count('pass_out') == 1
    k = res['e_plan'].plans[0].kernels
    # form (b): the mixture block's entry points on its state, one of each per sweep
    assert k.calls.count('pass') == 1 + 4
    assert [k.gmm.calls.count(n) for n in ('init_state', 'update_mu', 'update_lambda',
                                           'prepare_z')] == [1, 4, 4, 4]


def run_hmm_rst(after):
    """doc/source/examples/hmm.rst, second model, with engine='fused'."""
    from bayespy_amd.nodes import Dirichlet, CategoricalMarkovChain, Mixture, Gaussian
    from bayespy_amd.inference import VB
    g = np.load(os.path.join(GOLDEN, 'markov_chains.npz'))
    y = g['in_hmm2_y']
    K = 3
    a0 = Dirichlet(1e-3 * np.ones(K), name='a0')
    A = Dirichlet(1e-3 * np.ones((K, K)), name='A')
    Z = CategoricalMarkovChain(a0, A, states=len(y), name='Z')
    mu = np.array([[0, 0], [3, 4], [6, 0]])
    Lambda = 2.0 ** (-2) * np.identity(2)
    Y = Mixture(Z, Gaussian, mu, Lambda, name='Y')
    Y.observe(y)
    Q = VB(Y, Z, A, a0, engine='fused')
    after(Q)
    Q.update(repeat=1000, verbose=False)
    L = Q.L[:Q.iter]
    assert '%e' % L[0] == '-9.963054e+02'
    assert Q.iter == 8 and '%e' % L[-1] == '-9.235053e+02'
    np.testing.assert_allclose(L, g['hmm2_L'], rtol=L_RTOL)
    for nm, nd in dict(Z=Z, A=A, a0=a0).items():
        for i, u in enumerate(nd.get_moments()):
            np.testing.assert_allclose(u, g['hmm2_%s_u_%d' % (nm, i)], err_msg=nm, **MOM_TOL)
    np.testing.assert_allclose(Y.parents[0].get_moments()[0].sum(-1), 1.0, rtol=1e-12)


def test_hmm_rst_known_answer_on_the_kernel_double():
    run_hmm_rst(_on_double)


def test_random_initialisation_and_device_shapes():
    from bayespy_amd.inference import VB
    m = _model('b')
    m['Z'].initialize_from_random()
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    assert Q.compute_lowerbound() == -np.inf           # a point mass
    z0, zz = m['Z'].get_moments()
    B, T, K = 7, 12, 4
    assert z0.shape == (B, K) and zz.shape == (B, T - 1, K, K)
    assert set(np.unique(zz)) <= {0.0, 1.0} and np.all(zz.sum((-1, -2)) == 1)
    assert m['Y'].parents[0].get_moments()[0].shape == (B, T, K)
    Q.update(repeat=2, verbose=False)
    assert np.all(np.isfinite(Q.L[:2]))


def test_save_load_round_trip_on_the_double(tmp_path):
    _save_load(tmp_path, 'd')


def test_save_load_round_trip_with_learned_emissions(tmp_path):
    _save_load(tmp_path, 'e')


def _save_load(tmp_path, tag):
    from hmm_models import run_hmm_cases
    g, gin = _golden()
    Q = run_hmm_cases(_mods(_on_double, engine='fused'), gin, only=(tag,))[tag + '_plan']
    fn = str(tmp_path / 'hmm.ckpt')
    Q.save(filename=fn)
    L4 = Q.L[:4].copy()
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    assert Q.iter == 4
    np.testing.assert_array_equal(Q.L[:4], L4)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)


# -- the device header on the host ---------------------------------------------------------------------
def pass_inputs(B, T, D, K, seed=None):
    from scipy import special
    rs = np.random.RandomState(B + 3 * T + 5 * D + 7 * K if seed is None else seed)
    mu = 3.0 * rs.normal(size=(K, D))
    W = rs.normal(size=(K, D, D + 2))
    from bayespy_amd.inference.plans.hmm import emission_tables
    C, _ = emission_tables(mu, np.einsum('kab,kcb->kac', W, W) / (D + 2))
    Y = mu[rs.randint(K, size=(B, T))] + rs.normal(size=(B, T, D))
    al0, alA = rs.gamma(1.0, size=K) + 0.05, rs.gamma(1.0, size=(K, K)) + 0.05
    la0 = special.digamma(al0) - special.digamma(al0.sum())
    lA = special.digamma(alA) - special.digamma(alA.sum(-1, keepdims=True))
    return Y, C, la0, lA


HOST_SHAPES = [(1, 2, 1, 1), (3, 2, 1, 2), (5, 3, 3, 3), (33, 7, 2, 2), (9, 65, 8, 5), (4, 5, 3, 17),
               (3, 4, 2, 33), (2, 3, 8, 64)]


@pytest.mark.parametrize('B,T,D,K', HOST_SHAPES)
def test_host_build_of_the_device_header_against_long_double(B, T, D, K):
    """The rule of DESIGN 4.15: 8 times the deviation of the float64 evaluation of the reference
    formulas from long double, floor 4 ulp of the quantity's magnitude."""
    from hmm_fused_host import host_pass, compare
    Y, C, la0, lA = pass_inputs(B, T, D, K)
    got = host_pass(Y, C, la0, lA, want=True)
    keys = ('z0sum', 'xisum', 'T', 'logZ', 'ge', 'gamma', 'z0', 'zz')
    assert compare(got, Y, C, la0, lA, keys, label=str((B, T, D, K))) == []
    off = host_pass(Y, C, la0, lA)
    for k in ('z0sum', 'xisum', 'T', 'logZ', 'ge'):
        np.testing.assert_array_equal(off[k], got[k])
    # the prior pass and fixed labels
    assert compare(host_pass(Y, None, la0, lA), Y, None, la0, lA) == []
    lab = np.random.RandomState(0).randint(K, size=(B, T))
    r = host_pass(Y, C, la0, lA, labels=lab, want=True)
    onehot = np.eye(K)[lab]
    np.testing.assert_array_equal(r['gamma'], onehot)
    np.testing.assert_array_equal(r['z0sum'], onehot[:, 0].sum(0))
    np.testing.assert_array_equal(r['xisum'], np.einsum('bti,btj->ij', onehot[:, :-1], onehot[:, 1:]))
    np.testing.assert_allclose(r['T'][:, 1:1 + D], np.einsum('btk,btd->kd', onehot, Y), rtol=1e-13,
                               atol=1e-13)
    assert r['logZ'] == 0 and r['ge'] == 0


def test_host_build_edge_cases():
    from hmm_fused_host import host_pass
    Y, C, la0, lA = pass_inputs(4, 6, 2, 3)
    z = host_pass(Y[:0], C, la0, lA)
    assert not np.any(z['z0sum']) and not np.any(z['xisum']) and not np.any(z['T']) and z['logZ'] == 0
    la0[1] = -np.inf
    lA[:, 1] = -np.inf
    r = host_pass(Y, C, la0, lA, want=True)
    assert np.all(r['gamma'][..., 1] == 0) and np.all(r['zz'][..., 1] == 0)
    np.testing.assert_allclose(r['gamma'].sum(-1), 1.0, rtol=1e-13)
    r = host_pass(Y, C, la0, np.full((3, 3), -np.inf), want=True)
    assert np.all(np.isnan(r['zz'])) and np.isnan(r['logZ'])


# -- the C ABI -----------------------------------------------------------------------------------------
def test_cabi_declares_the_entry_points():
    """Fails without the feature: the library has no such symbols."""
    from bayespy_amd import _lib
    from hmm_fused_host import hmmf_host
    lib = _lib.load()
    for name in ('vmp_hmm_fused_limits', 'vmp_hmm_fused_plan', 'vmp_hmm_fused_pass'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    mk, md = ctypes.c_int32(), ctypes.c_int32()
    assert lib.vmp_hmm_fused_limits(ctypes.byref(mk), ctypes.byref(md)) == _lib.VMP_OK
    from bayespy_amd.inference.plans.hmm import hmm_limits
    assert (mk.value, md.value) == hmm_limits() == (64, 8)
    assert lib.vmp_hmm_fused_limits(None, None) == _lib.VMP_ERR_INVALID
    host = hmmf_host()
    c, w = ctypes.c_int64(), ctypes.c_int64()
    for B, T, D, K in ((0, 2, 1, 1), (1000, 70, 3, 5), (20000, 1000, 2, 8), (10 ** 6, 10, 8, 64)):
        assert lib.vmp_hmm_fused_plan(B, T, D, K, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_OK
        assert c.value == host.hmmf_chains_per_wg(B, T, D, K)
        assert w.value == host.hmmf_workspace_doubles(B, T, D, K)
        assert c.value % (64 // host.hmmf_kpad(K)) == 0 and host.hmmf_wgs(B, T, D, K) <= 4096
    U, I = _lib.VMP_ERR_UNSUPPORTED, _lib.VMP_ERR_INVALID
    assert lib.vmp_hmm_fused_plan(10, 4, 2, 65, ctypes.byref(c), ctypes.byref(w)) == U
    assert lib.vmp_hmm_fused_plan(10, 4, 9, 4, ctypes.byref(c), ctypes.byref(w)) == U
    assert lib.vmp_hmm_fused_plan(-1, 4, 2, 4, ctypes.byref(c), ctypes.byref(w)) == I
    assert lib.vmp_hmm_fused_plan(10, 1, 2, 4, ctypes.byref(c), ctypes.byref(w)) == I
    assert lib.vmp_hmm_fused_plan(10, 4, 2, 4, None, None) == I


def test_cabi_pass_checks_its_arguments():
    """Without a context nothing is launched: the shape is judged first, then the pointers."""
    from bayespy_amd import _lib
    lib = _lib.load()
    U, I = _lib.VMP_ERR_UNSUPPORTED, _lib.VMP_ERR_INVALID
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=4, T=3, D=2, K=3, ctx=None, C=p, ldc=6, a0=p, A=p, ws=p, z0sum=p, xisum=p, Ts=p,
             scal=p, Y=p):
        return lib.vmp_hmm_fused_pass(ctx, B, T, D, K, Y, C, ldc, a0, A, None, ws, z0sum, xisum, Ts,
                                      scal, None, None, None)
    assert call() == I                                  # a null context
    for kw in (dict(B=-1), dict(T=1), dict(T=-3), dict(D=0), dict(K=0), dict(K=-2)):
        assert call(**kw) == I, kw
    assert call(K=65) == U and call(D=9) == U
    assert call(ldc=5) == I                             # below the 6 features of D = 2
    assert call(C=None, ldc=0) == I                     # fine but for the context
