"""CPU: the fused hidden-Markov-model block with categorical emissions without a device -- the
matcher and its declining reasons, the registration through ``plans.OPT_IN_EMISSIONS``, the plan's
host logic on the kernel double tests/hmm_cat_host.py (CPUCatHMMKernels) against every fixture of
tests/golden/hmm_cat.npz (live reference, tools/make_golden_hmm_cat.py), the g++ build of the
device header csrc/vmp_hmm_fused_dev.h against a long-double restatement, masks and words out of
range, persistence, the host source under the address and undefined-behaviour sanitizers as a
stand-alone program, and the C ABI."""
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

L_RTOL = 1e-9                               # those of the Gaussian block's fixtures
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
    from hmm_cat_host import CPUCatHMMKernels
    plan = Q.plans[0]
    assert type(plan).__name__ == 'CategoricalHMMPlan' and len(Q.plans) == 1
    rt = Runtime(device='cpu')
    plan._rt, plan._kernels = rt, CPUCatHMMKernels(rt)


def _golden():
    g = np.load(os.path.join(GOLDEN, 'hmm_cat.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


def _model(tag, **kw):
    from hmm_cat_models import build
    return build(_mods(), _golden()[1], tag, **kw)


def _nodes(m):
    from bayespy_amd.nodes.node import Node
    return [m['Y'], m['Z']] + [m[k] for k in ('P', 'A', 'a0') if isinstance(m[k], Node)]


# -- the matcher and the registration ----------------------------------------------------------------
def test_matcher_accepts_every_form_and_the_gaussian_block_still_declines():
    from hmm_cat_models import CASES
    from bayespy_amd.inference.plans.hmm import HMMPlan
    from bayespy_amd.inference.plans.hmm_cat import CategoricalHMMPlan
    for tag, case in CASES.items():
        for observe in (True, False):
            m = _model(tag, observe=observe)
            why = []
            r = CategoricalHMMPlan.match(_nodes(m), why)
            assert r is not None and why == [], (tag, why)
            assert r['Y'] is m['Y'] and r['Z'] is m['Z']
            assert sorted(k for k in r if k in ('a0', 'A', 'P')) == sorted(case[4])
            assert all(r[k] is m[k] for k in case[4])
            why = []
            assert HMMPlan.match(_nodes(m), why) is None
            assert len(why) == 1 and 'Categorical, not Gaussian' in why[0]


def test_registration_leaves_the_pinned_lists_alone():
    from bayespy_amd.inference import plans
    from bayespy_amd.inference.plans.hmm_cat import CategoricalHMMPlan
    assert [P.__name__ for P in plans.OPT_IN_TYPES] == ['BernoulliMixturePlan', 'HMMPlan']
    assert [P.__name__ for P in plans.PLAN_TYPES] == ['PCAPlan', 'MaskedPCAPlan', 'GMMPlan',
                                                     'LSSMPlan', 'MaskedLSSMPlan', 'LDAPlan']
    assert plans.OPT_IN_EMISSIONS == {plans.HMMPlan: [CategoricalHMMPlan]}
    names = [P.__name__ for P in plans.opt_in_types()]
    assert names == ['BernoulliMixturePlan', 'HMMPlan', 'CategoricalHMMPlan']


def test_block_is_opt_in():
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.generic import GenericPlan
    from bayespy_amd.inference.plans.hmm_cat import CategoricalHMMPlan
    import host_generic
    host_generic.install()
    try:
        for tag in ('i', 'iii'):
            m = _model(tag)
            with warnings.catch_warnings():
                warnings.simplefilter('error')          # the default engine: no new warning
                got = compile_model(_nodes(m))
            assert len(got) == 1 and isinstance(got[0], GenericPlan)
            fused = compile_model(_nodes(m), engine='fused')
            assert len(fused) == 1 and isinstance(fused[0], CategoricalHMMPlan)
            assert compile_model(_nodes(m), engine='fused')[0] is fused[0]
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                again = compile_model(_nodes(m))
            assert isinstance(again[0], GenericPlan)    # an opt-in plan is kept only when asked for
    finally:
        host_generic.uninstall()


def test_matcher_declines_with_one_reason_each():
    from bayespy_amd import nodes as N_
    from bayespy_amd.inference.plans.hmm_cat import CategoricalHMMPlan, hmm_cat_limits
    B, T, K, M = 4, 6, 3, 5
    y = np.random.RandomState(0).randint(M, size=(B, T))

    def reason(m):
        why = []
        assert CategoricalHMMPlan.match(_nodes(m), why) is None and len(why) == 1, why
        assert why[0].startswith('fused hidden-Markov-model block with categorical emissions')
        return why[0]

    def build(a0=None, A=None, P=None, K=K, M=M, Zkw={}):
        a0 = N_.Dirichlet(np.ones(K), name='a0') if a0 is None else a0
        A = N_.Dirichlet(np.ones((K, K)), name='A') if A is None else A
        P = N_.Dirichlet(np.ones((K, M)), name='P') if P is None else P
        Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z', **Zkw)
        Y = N_.Mixture(Z, N_.Categorical, P, name='Y')
        return dict(a0=a0, A=A, P=P, Z=Z, Y=Y)
    assert CategoricalHMMPlan.match(_nodes(build())) is not None
    # plates_multiplier, a sharded plate
    assert 'plates_multiplier' in reason(build(Zkw=dict(plates_multiplier=(2.5,))))
    m = build()
    m['Z'].shard(0)
    assert 'sharded' in reason(m)
    # a scalar mask, a mask that broadcasts over a plate
    m = build()
    m['Y'].observe(y, mask=False)
    assert 'mask of shape ()' in reason(m)
    m = build()
    m['Y'].observe(y, mask=(np.arange(T) % 2 == 0))
    assert 'mask of shape (6,)' in reason(m)
    # a Concentration parent, on each role
    for nm, shape in (('a0', ()), ('A', (K,)), ('P', (K,))):
        c = N_.DirichletConcentration(M if nm == 'P' else K, plates=shape, name='c')
        assert 'concentration of %s is a node' % nm in reason(
            build(**{nm: N_.Dirichlet(c, name=nm)}))
    # other children on a role
    m = build()
    N_.CategoricalMarkovChain(m['a0'], np.full((K, K), 1.0 / K), states=3, name='other')
    assert 'other children' in reason(m)
    m = build()
    N_.Categorical(m['P'], name='other')
    assert 'other children' in reason(m)
    m = build()
    N_.CategoricalMarkovChain(np.full(K, 1.0 / K), m['A'], states=3, name='other')
    assert 'other children' in reason(m)
    m = build()                                     # a second mixture on the chain: Z / Zc
    N_.Mixture(m['Z'], N_.Categorical, np.full((K, M), 1.0 / M), name='other')
    assert 'other children' in reason(m)
    # the limits
    max_K, max_M = hmm_cat_limits()
    assert (max_K, max_M) == (64, 128)
    assert 'exceed the limits' in reason(build(K=max_K + 1))
    assert 'exceed the limits' in reason(build(M=max_M + 1))
    assert CategoricalHMMPlan.match(_nodes(build(K=max_K, M=max_M))) is not None
    # a zero in a constant P
    P0 = np.full((K, M), 1.0 / (M - 1))
    P0[1, 2] = 0.0
    assert '0 log 0' in reason(build(P=P0))
    # observed or initialised parents, a time plate on A, plates on a0
    m = build()
    m['P'].initialize_from_value(np.full((K, M), 1.0 / M))
    assert 'P is initialised by value' in reason(m)
    m = build()
    m['A'].observe(np.full((K, K), 1.0 / K))
    assert 'is observed' in reason(m)
    assert 'A has plates' in reason(build(A=N_.Dirichlet(np.ones((T - 1, K, K)), name='A')))
    assert 'a0 has plates' in reason(build(a0=N_.Dirichlet(np.ones(K), plates=(B,), name='a0')))
    assert 'constant A' in reason(build(A=np.full((T - 1, K, K), 1.0 / K)))
    m = build()
    m['Z'].states = 1
    assert 'T = 1 < 2' in reason(m)


def test_a_gaussian_hmm_gets_no_reason_from_this_block():
    from hmm_models import build_hmm
    from test_hmm_fused_host import _golden as golden_gauss
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.plans.hmm_cat import CategoricalHMMPlan
    gin = golden_gauss()[1]
    m = build_hmm(_mods(), gin['a_y'], gin['a_mu'], gin['a_Lambda'])
    why = []
    assert CategoricalHMMPlan.match([m['Y'], m['Z'], m['A'], m['a0']], why) is None and why == []
    # declined by its own block: one block's reason, not two
    m['Y'].observe(gin['a_y'], mask=False)
    with pytest.raises(NotImplementedError) as exc:
        VB(m['Y'], m['Z'], m['A'], m['a0'], engine='fused')
    assert 'categorical emissions' not in str(exc.value) and 'mask' in str(exc.value)


def test_engine_fused_builds_the_block_and_declined_models_raise():
    """Fails without the feature: engine='fused' raises "Categorical, not Gaussian"."""
    from bayespy_amd.inference import VB
    m = _model('i')
    Q = VB(m['Y'], m['Z'], engine='fused')
    assert type(Q.plans[0]).__name__ == 'CategoricalHMMPlan'
    m = _model('ii')
    m['Y'].observe(_golden()[1]['ii_y'], mask=False)
    with pytest.raises(NotImplementedError, match='categorical emissions.*mask'):
        VB(*_nodes(m), engine='fused')
    assert all(n._plan is None for n in _nodes(m))


# -- the plan on the kernel double ---------------------------------------------------------------------
def check_fixtures(res, g):
    from hmm_cat_models import n_fixture_arrays
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan') or k.endswith('_model'):
            continue
        tag = k.split('_')[0]
        want = g[k]
        if k.endswith('_mask'):
            np.testing.assert_array_equal(v, want, err_msg=k)
        elif '_Z_u' in k and tag + '_Z_mask' in g.files:
            ob = g[tag + '_Z_mask']
            assert ob.sum() == 5                    # one chain without an observed step
            np.testing.assert_allclose(v[ob], want[ob], err_msg=k, **MOM_TOL)
        elif '_u' in k:
            np.testing.assert_allclose(v, want, err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(v, want, err_msg=k, rtol=L_RTOL, atol=1e-9)
        checked += 1
    assert checked == n_fixture_arrays()


def test_plan_reproduces_every_fixture_on_the_kernel_double():
    from hmm_cat_models import run_cases
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_cases(_mods(_on_double, engine='fused'), gin, fill=-1)
    check_fixtures(res, g)
    # hmm.rst's model: set-up pass + one update; gamma, z0 and zz only on request
    calls = res['i_plan'].plans[0].kernels.calls
    assert calls.count('pass') == 2 and calls.count('pass_out') == 1
    assert 'dirichlet' not in calls                 # three constants: no table is ever updated
    # everything learned: three tables at set-up, then one Dirichlet call per node and sweep
    calls = res['ii_plan'].plans[0].kernels.calls
    assert calls.count('pass') == 1 + 4 and calls.count('dirichlet') == 3 + 3 * 4
    calls = res['v_plan'].plans[0].kernels.calls
    assert calls.count('mpass') == 1 + 4 and calls.count('pass') == 0
    # a0 constant, A and P learned; observed twice after VB(...): one set-up pass for both
    calls = res['vi_plan'].plans[0].kernels.calls
    assert calls.count('pass') == 1 + 4 and calls.count('dirichlet') == 2 + 2 * 4


def test_hmm_rst_first_model_is_the_exact_posterior():
    """One update of Z is exact when a0, A and P are constants: the bound is log p(y), here by the
    plain forward recursion in probabilities, and a second update changes nothing."""
    from hmm_cat_models import run_cases, RST_A0, RST_A, RST_P
    g, gin = _golden()
    res = run_cases(_mods(_on_double, engine='fused'), gin, only=('i',))
    y = gin['i_y']
    al, logp = RST_A0 * RST_P[:, y[0]], 0.0
    for t in range(1, len(y)):
        logp += np.log(al.sum())
        al = (al / al.sum()) @ RST_A * RST_P[:, y[t]]
    logp += np.log(al.sum())
    np.testing.assert_allclose(res['i_L'][0], logp, rtol=1e-12)
    Q = res['i_plan']
    Q.update(verbose=False)
    np.testing.assert_allclose(Q.L[1], logp, rtol=1e-12)
    gam = res['i_model']['Y'].parents[0].get_moments()[0]
    assert gam.shape == (100, 2)
    np.testing.assert_allclose(gam.sum(-1), 1.0, rtol=1e-12)


def test_moments_of_P_and_Y_and_the_masks():
    from hmm_cat_models import run_cases
    g, gin = _golden()
    res = run_cases(_mods(_on_double, engine='fused'), gin, only=('v',), fill=-1)
    m = res['v_model']
    (elogP,) = m['P'].get_moments()
    assert elogP.shape == (3, 4) and np.all(elogP < 0)
    np.testing.assert_allclose(elogP, g['v_P_u0'], **MOM_TOL)
    (onehot,) = m['Y'].get_moments()
    assert onehot.shape == (6, 15, 4)
    np.testing.assert_array_equal(onehot.sum(-1), gin['v_mask'].astype(float))
    np.testing.assert_array_equal(onehot.argmax(-1)[gin['v_mask']], gin['v_y'][gin['v_mask']])
    np.testing.assert_array_equal(m['Y'].mask, gin['v_mask'])
    np.testing.assert_array_equal(m['Z'].mask, gin['v_mask'].any(-1))


def test_labels_and_random_initialisation():
    from bayespy_amd.inference import VB
    m = _model('iii')
    m['Z'].initialize_from_random()
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    assert Q.compute_lowerbound() == -np.inf           # a point mass
    z0, zz = m['Z'].get_moments()
    B, T, K = 5, 12, 3
    assert z0.shape == (B, K) and zz.shape == (B, T - 1, K, K)
    assert set(np.unique(zz)) <= {0.0, 1.0} and np.all(zz.sum((-1, -2)) == 1)
    Q.update(repeat=2, verbose=False)
    assert np.all(np.isfinite(Q.L[:2]))
    # fixed labels: the one-hot moments of exactly these states
    m = _model('iii')
    lab = np.random.RandomState(3).randint(K, size=(B, T))
    m['Z'].initialize_from_value(lab)
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    np.testing.assert_array_equal(m['Z'].get_moments()[0], np.eye(K)[lab[:, 0]])
    np.testing.assert_array_equal(m['Y'].parents[0].get_moments()[0], np.eye(K)[lab])


def test_an_empty_batch_through_the_plan():
    """B = 0: every sum is zero, the tables stay at their priors and every bound term is 0."""
    from bayespy_amd import nodes as N_
    from bayespy_amd.inference import VB
    K, M, T = 3, 4, 5
    a0 = N_.Dirichlet(np.ones(K), name='a0')
    A = N_.Dirichlet(np.ones((K, K)), name='A')
    P = N_.Dirichlet(np.ones((K, M)), name='P')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=(0,), name='Z')
    Y = N_.Mixture(Z, N_.Categorical, P, name='Y')
    Y.observe(np.zeros((0, T), dtype=int))
    Q = VB(Y, Z, P, A, a0, engine='fused')
    _on_double(Q)
    prior = P.get_moments()[0].copy()
    Q.update(verbose=False)
    assert Q.L[0] == 0.0
    plan = Q.plans[0]
    assert plan.B == 0 and not plan.S.numpy().any() and not plan.xisum.numpy().any()
    np.testing.assert_array_equal(P.get_moments()[0], prior)
    z0, zz = Z.get_moments()
    assert z0.shape == (0, K) and zz.shape == (0, T - 1, K, K)


def test_reobservation_keeps_the_posteriors():
    from hmm_cat_models import run_cases
    g, gin = _golden()
    res = run_cases(_mods(_on_double, engine='fused'), gin, only=('ii',))
    Q, m = res['ii_plan'], res['ii_model']
    plan = Q.plans[0]
    P_before = m['P'].get_moments()[0].copy()
    calls = plan.kernels.calls
    n = calls.count('pass')
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m['Y'].observe(gin['ii_y'][::-1].copy())
    assert m['Y']._plan is plan and plan.has_state()
    np.testing.assert_array_equal(m['P'].get_moments()[0], P_before)
    L = Q.compute_lowerbound()
    assert calls.count('pass') == n + 1 and np.isfinite(L) and L != Q.L[3]
    np.testing.assert_array_equal(plan.yd.numpy().reshape(-1), gin['ii_y'][::-1])


def test_words_out_of_range_raise_from_the_plan():
    import torch
    from bayespy_amd.inference import VB
    gin = _golden()[1]
    for tag, bad in (('ii', 5), ('ii', -1), ('v', 4)):
        for as_tensor in (False, True):
            m = _model(tag, observe=False)
            y = gin[tag + '_y'].copy()
            mask = gin[tag + '_mask'] if tag == 'v' else np.ones(y.shape, dtype=bool)
            y[~mask] = -1                                   # fine: never used
            pos = tuple(np.argwhere(mask)[3])
            y[pos] = bad
            data = torch.from_numpy(y) if as_tensor else y
            m['Y'].observe(data, **(dict(mask=mask) if tag == 'v' else {}))
            Q = VB(*_nodes(m), engine='fused')
            _on_double(Q)
            with pytest.raises(ValueError, match='Invalid category index'):
                Q.update(verbose=False)
    m = _model('ii', observe=False)
    m['Y'].observe(gin['ii_y'] + 0.5)
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    with pytest.raises(ValueError, match='Values must be integers'):
        Q.update(verbose=False)


def test_save_load_round_trip_and_the_other_blocks_checkpoint(tmp_path):
    from hmm_cat_models import run_cases
    from hmm_models import run_hmm_cases
    import test_hmm_fused_host as gauss
    g, gin = _golden()
    for tag in ('v', 'vi'):
        Q = run_cases(_mods(_on_double, engine='fused'), gin, only=(tag,), fill=-1)[tag + '_plan']
        fn = str(tmp_path / ('hmm_cat_%s.ckpt' % tag))
        Q.save(filename=fn)
        L4 = Q.L[:4].copy()
        Q.update(repeat=2, verbose=False)
        L6 = Q.L[:6].copy()
        Q.load(filename=fn)
        assert Q.iter == 4
        np.testing.assert_array_equal(Q.L[:4], L4)
        Q.update(repeat=2, verbose=False)
        np.testing.assert_array_equal(Q.L[:6], L6)
    # the Gaussian block's checkpoint is refused here, and this block's there
    Qg = run_hmm_cases(gauss._mods(gauss._on_double, engine='fused'), gauss._golden()[1],
                       only=('a',))['a_plan']
    fg = str(tmp_path / 'hmm_gauss.ckpt')
    Qg.save(filename=fg)
    with pytest.raises(Exception, match='categorical emissions: it holds that of the block with '
                                        'Gaussian emissions'):
        Q.load(filename=fg)
    with pytest.raises(Exception, match='Gaussian emissions: it holds that of the block with '
                                        'categorical emissions'):
        Qg.load(filename=fn)
    # another shape of the same block
    Q2 = run_cases(_mods(_on_double, engine='fused'), gin, only=('iii',))['iii_plan']
    with pytest.raises(ValueError, match=r'\(B, T, M, K, learned P, constant a0, constant A\)'):
        Q2.load(filename=fn)


# -- the device header on the host ---------------------------------------------------------------------
HOST_SHAPES = [(1, 2, 1, 1), (3, 2, 3, 2), (5, 3, 4, 3), (65, 7, 3, 2), (9, 65, 16, 5), (4, 5, 128, 17),
               (3, 4, 3, 33), (2, 3, 128, 64)]


@pytest.mark.parametrize('B,T,M,K', HOST_SHAPES)
def test_host_build_of_the_device_header_against_long_double(B, T, M, K):
    """The rule of DESIGN 4.14: 8 times the deviation of the float64 evaluation of the reference
    formulas from long double, floor 4 ulp of the quantity's magnitude."""
    from hmm_cat_host import host_pass, compare, pass_inputs, ALL, SUMS
    y, Pt, la0, lA = pass_inputs(B, T, M, K)
    got = host_pass(y, Pt, la0, lA, want=True)
    assert compare(got, y, Pt, la0, lA, ALL, label=str((B, T, M, K))) == []
    off = host_pass(y, Pt, la0, lA)
    for k in SUMS:
        np.testing.assert_array_equal(off[k], got[k])
    np.testing.assert_allclose(got['S'].sum(), B * T, rtol=1e-12)
    # the prior pass and fixed labels
    assert compare(host_pass(y, M, la0, lA), y, M, la0, lA) == []
    lab = np.random.RandomState(0).randint(K, size=(B, T))
    r = host_pass(y, Pt, la0, lA, labels=lab, want=True)
    onehot = np.eye(K)[lab]
    np.testing.assert_array_equal(r['gamma'], onehot)
    np.testing.assert_array_equal(r['z0sum'], onehot[:, 0].sum(0))
    np.testing.assert_array_equal(r['xisum'], np.einsum('bti,btj->ij', onehot[:, :-1], onehot[:, 1:]))
    np.testing.assert_array_equal(r['S'], np.einsum('btm,btk->mk', np.eye(M)[y], onehot))
    assert r['logZ'] == 0 and r['ge'] == 0


@pytest.mark.parametrize('B,T,M,K', [(7, 6, 4, 3), (35, 5, 3, 2), (3, 4, 128, 64)])
def test_masks_on_the_host_build(B, T, M, K):
    from hmm_cat_host import host_pass, compare, pass_inputs, ALL, SUMS
    from hmm_fused_host import mixed_mask
    y, Pt, la0, lA = pass_inputs(B, T, M, K)
    plain = host_pass(y, Pt, la0, lA, want=True)
    ones = host_pass(y, Pt, la0, lA, want=True, mask=np.ones((B, T)))
    for k in ALL:                                   # a mask of ones: the bits of the unmasked pass
        np.testing.assert_array_equal(ones[k], plain[k], err_msg=k)
    mask = mixed_mask(B, T, np.random.RandomState(B))
    ref = host_pass(np.where(mask, y, 0), Pt, la0, lA, want=True, mask=mask)
    assert compare(ref, y, Pt, la0, lA, ALL, label='masked ' + str((B, T, M, K)), mask=mask) == []
    for fill in (-1, M - 1, M, 2 ** 31 - 1, -2 ** 31):  # what stands at a masked position: never used
        got = host_pass(np.where(mask, y, fill), Pt, la0, lA, want=True, mask=mask)
        for k in ALL:
            np.testing.assert_array_equal(got[k], ref[k], err_msg='%s fill %d' % (k, fill))
    # a word out of range at an observed position counts as a masked step (the plan reports it)
    pos = tuple(np.argwhere(mask)[len(np.argwhere(mask)) // 2])
    hole = mask.copy()
    hole[pos] = False
    if hole[pos[0]].any():                          # the chain weight is taken from the mask alone
        want = host_pass(y, Pt, la0, lA, want=True, mask=hole)
        for bad in (M, -1, -7, 10 ** 9):
            yb = y.copy()
            yb[pos] = bad
            got = host_pass(yb, Pt, la0, lA, want=True, mask=mask)
            for k in ALL:
                np.testing.assert_array_equal(got[k], want[k], err_msg='%s word %d' % (k, bad))


def test_host_build_edge_cases():
    from hmm_cat_host import host_pass, pass_inputs
    y, Pt, la0, lA = pass_inputs(4, 6, 5, 3)
    z = host_pass(y[:0], Pt, la0, lA)                   # B = 0
    assert not np.any(z['z0sum']) and not np.any(z['xisum']) and not np.any(z['S']) and z['logZ'] == 0
    la0[1] = -np.inf
    lA[:, 1] = -np.inf
    r = host_pass(y, Pt, la0, lA, want=True)
    assert np.all(r['gamma'][..., 1] == 0) and np.all(r['zz'][..., 1] == 0) and np.all(r['S'][:, 1] == 0)
    np.testing.assert_allclose(r['gamma'].sum(-1), 1.0, rtol=1e-13)


def test_host_source_under_the_sanitizers_as_a_program_of_its_own():
    """tests/host/hmm_cat_host_main.cpp: the host source on two shapes (a padded bucket with a
    mask, -1 at masked positions and a word out of range; K = 64, M = 128), built with
    -fsanitize=address,undefined and run as a program, never loaded into python."""
    from hmm_cat_host import build_sanitized_program
    exe = build_sanitized_program()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count('sum S') == 3 and 'ERROR' not in r.stdout and 'runtime error' not in r.stdout


# -- the C ABI -----------------------------------------------------------------------------------------
def test_cabi_declares_the_entry_points():
    """Fails without the feature: the library has no such symbols."""
    from bayespy_amd import _lib
    from hmm_cat_host import hmmc_host
    lib = _lib.load()
    for name in ('vmp_hmm_fused_cat_limits', 'vmp_hmm_fused_cat_plan',
                 'vmp_hmm_fused_pass_categorical'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    mk, mm = ctypes.c_int32(), ctypes.c_int32()
    assert lib.vmp_hmm_fused_cat_limits(ctypes.byref(mk), ctypes.byref(mm)) == _lib.VMP_OK
    from bayespy_amd.inference.plans.hmm_cat import hmm_cat_limits
    host = hmmc_host()
    assert (mk.value, mm.value) == hmm_cat_limits() == (64, 128) == (host.hmmc_max_k(),
                                                                   host.hmmc_max_m())
    assert lib.vmp_hmm_fused_cat_limits(None, None) == _lib.VMP_ERR_INVALID
    c, w = ctypes.c_int64(), ctypes.c_int64()
    for B, T, M, K in ((0, 2, 1, 1), (1000, 70, 3, 5), (20000, 1000, 16, 8), (10 ** 6, 10, 128, 64)):
        assert lib.vmp_hmm_fused_cat_plan(B, T, M, K, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_OK
        assert c.value == host.hmmc_chains_per_wg(B, M, K)
        assert w.value == host.hmmc_workspace_doubles(B, T, M, K)
        nw = host.hmmc_wgs(B, M, K)
        assert c.value % (64 // max(2, 1 << (K - 1).bit_length())) == 0 and nw <= 4096
        assert nw * host.hmmc_partial_doubles(M, K) <= 2 ** 24
    U, I = _lib.VMP_ERR_UNSUPPORTED, _lib.VMP_ERR_INVALID
    assert lib.vmp_hmm_fused_cat_plan(10, 4, 2, 65, ctypes.byref(c), ctypes.byref(w)) == U
    assert lib.vmp_hmm_fused_cat_plan(10, 4, 129, 4, ctypes.byref(c), ctypes.byref(w)) == U
    assert lib.vmp_hmm_fused_cat_plan(-1, 4, 2, 4, ctypes.byref(c), ctypes.byref(w)) == I
    assert lib.vmp_hmm_fused_cat_plan(10, 1, 2, 4, ctypes.byref(c), ctypes.byref(w)) == I
    assert lib.vmp_hmm_fused_cat_plan(10, 4, 0, 4, ctypes.byref(c), ctypes.byref(w)) == I
    assert lib.vmp_hmm_fused_cat_plan(10, 4, 2, 4, None, None) == I


def test_cabi_pass_checks_its_arguments():
    """Without a context nothing is launched: the shape is judged first, then the pointers."""
    from bayespy_amd import _lib
    lib = _lib.load()
    U, I = _lib.VMP_ERR_UNSUPPORTED, _lib.VMP_ERR_INVALID
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(B=4, T=3, M=2, K=3, ctx=None, y=p, Pt=p, a0=p, A=p, ws=p, z0sum=p, xisum=p, S=p,
             scal=p):
        return lib.vmp_hmm_fused_pass_categorical(ctx, B, T, M, K, y, Pt, a0, A, None, None, ws,
                                                  z0sum, xisum, S, scal, None, None, None)
    assert call() == I                                  # a null context
    for kw in (dict(B=-1), dict(T=1), dict(T=-3), dict(M=0), dict(K=0), dict(K=-2)):
        assert call(**kw) == I, kw
    assert call(K=65) == U and call(M=129) == U
    assert call(Pt=None) == I                           # fine but for the context
