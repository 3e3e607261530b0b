"""CPU: masks on the fused hidden-Markov-model block without a device -- the matcher (full-shape
masks accepted, scalar and broadcasting masks declined), the plan's host logic on the kernel double
tests/hmm_fused_host.py (CPUHMMKernels) against every fixture of tests/golden/hmm_masked.npz
(live reference, tools/make_golden_hmm.py masked), ``Z.mask`` / ``Y.mask``, re-observation, save /
load, the g++ build of the device header's masked pass against a long-double restatement, and the
C ABI of ``vmp_hmm_fused_pass_masked``."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

L_RTOL = 1e-9                               # tests/test_hmm_fused_host.py
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
    g = np.load(os.path.join(GOLDEN, 'hmm_masked.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


def _device_mask(m):
    """A ``DeviceMask`` as ``observe`` builds it from a boolean tensor in HBM (here: on the host)."""
    import torch
    from bayespy_amd.nodes.node import DeviceMask
    return DeviceMask(torch.from_numpy(np.ascontiguousarray(m)))


def _model(tag, mask, learned=False):
    from hmm_models import build_hmm
    gin = _golden()[1]
    m = build_hmm(_mods(), gin[tag + '_y'], gin[tag + '_mu'], gin[tag + '_Lambda'], observe=False,
                  learned=learned)
    m['Y'].observe(gin[tag + '_y'], mask=mask)
    return m


def _nodes(m):
    from test_hmm_fused_host import _nodes as nodes
    return nodes(m)


# -- the matcher -----------------------------------------------------------------------------------------
def test_fixture_file_is_as_the_cases_demand():
    g, gin = _golden()
    for tag in 'abcdef':
        m = gin[tag + '_mask']
        assert np.all(np.isnan(gin[tag + '_y'][~m])) and np.all(np.isfinite(gin[tag + '_y'][m]))
        zm = np.atleast_1d(g[tag + '_Z_mask'])
        np.testing.assert_array_equal(zm, np.atleast_1d(m.any(axis=-1)))
        assert np.sum(~zm) <= 1 and (m.ndim == 1 or np.sum(zm) >= 2)
    assert not gin['a_mask'][0] and 0.6 < gin['a_mask'].mean() < 0.8
    np.testing.assert_array_equal(gin['b_mask'].sum(1), (12, 9, 5, 1, 0, 12, 7))
    np.testing.assert_array_equal(gin['c_mask'], [[1, 0], [0, 1], [0, 0]])
    assert np.any(gin['d_mask0'] != gin['d_mask'])
    assert os.path.getsize(os.path.join(GOLDEN, 'hmm_masked.npz')) < 2 ** 20


def test_matcher_accepts_full_shape_masks():
    """Fails without the feature: every mask is declined."""
    from bayespy_amd.inference.plans.hmm import HMMPlan
    gin = _golden()[1]
    for tag in ('a', 'b', 'e', 'f'):        # one chain and a batch, both emission forms
        for wrap in (lambda m: m, _device_mask, lambda m: m.astype(np.uint8)):
            m = _model(tag, wrap(gin[tag + '_mask']), learned=tag in 'ef')
            why = []
            r = HMMPlan.match(_nodes(m), why)
            assert r is not None and why == [], why
            assert r['Y'] is m['Y'] and ('mu' in r) == (tag in 'ef')
    assert 'mask' in HMMPlan.describe()


def test_matcher_declines_scalar_and_broadcasting_masks():
    from bayespy_amd.inference.plans.hmm import HMMPlan
    gin = _golden()[1]

    def reason(m):
        why = []
        assert HMMPlan.match(_nodes(m), why) is None and len(why) == 1, why
        return why[0]
    T = gin['b_mask'].shape[1]
    for tag, mask in (('a', False), ('b', False), ('b', gin['b_mask'][0]),
                      ('b', gin['b_mask'][:, :1]), ('b', gin['b_mask'][:1]),
                      ('b', _device_mask(gin['b_mask'][0])), ('a', np.array([False]))):
        r = reason(_model(tag, mask))
        assert 'mask' in r and '(T,)' in r and '(B, T)' in r, r
    assert str((7, T)) in reason(_model('b', gin['b_mask'][0]))


def test_engine_fused_builds_the_block_with_a_mask():
    """Fails without the feature."""
    from bayespy_amd.inference import VB
    gin = _golden()[1]
    m = _model('b', gin['b_mask'])
    Q = VB(*_nodes(m), engine='fused')
    assert type(Q.plans[0]).__name__ == 'HMMPlan'
    m = _model('b', gin['b_mask'][0])
    with pytest.raises(NotImplementedError, match='fused hidden-Markov-model block.*mask'):
        VB(*_nodes(m), engine='fused')


# -- the plan on the kernel double ---------------------------------------------------------------------
def check_masked_fixtures(res, g):
    from hmm_models import CASES, LEARNED
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan'):
            continue
        tag = k.split('_')[0]
        if k.endswith('_mask'):
            np.testing.assert_array_equal(v, g[k], err_msg=k)
        elif '_Z_u' in k:
            # the moments of a chain without an observed step are not compared
            zm = g[tag + '_Z_mask']
            if zm.ndim:
                assert zm.sum() >= 2
                np.testing.assert_allclose(v[zm], g[k][zm], err_msg=k, **MOM_TOL)
            else:
                assert zm
                np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        elif '_u' in k:
            np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL, atol=1e-9)
        checked += 1
    assert checked == len(CASES) * (1 + 4 + 4 + 2) + len(LEARNED) * (1 + 6 + 8 + 2)


def test_plan_reproduces_every_fixture_on_the_kernel_double():
    """Fails without the feature: engine='fused' declines the masked models."""
    from hmm_models import run_hmm_cases
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_hmm_cases(_mods(_on_double, engine='fused'), gin)
    check_masked_fixtures(res, g)
    calls = res['a_plan'].plans[0].kernels.calls
    # set-up pass + one per sweep, all masked; gamma, z0 and zz only on request
    assert calls.count('mpass') == 1 + 4 and calls.count('mpass_out') == 1
    assert not [c for c in calls if c.startswith('pass')]
    # observed twice after VB(...), before the first update: one set-up pass
    calls = res['d_plan'].plans[0].kernels.calls
    assert calls.count('mpass') == 1 + 4


def test_fixtures_with_device_masks_on_the_kernel_double():
    from hmm_models import run_hmm_cases
    g, gin = _golden()
    res = run_hmm_cases(_mods(_on_double, engine='fused'), gin, only=('b', 'd', 'f'),
                           device_mask=_device_mask)
    for k, v in res.items():
        if k.endswith('_L') or k.endswith('_mask'):
            np.testing.assert_allclose(np.asarray(v, dtype=float), np.asarray(g[k], dtype=float),
                                       err_msg=k, rtol=L_RTOL)


def test_masks_of_the_nodes():
    from bayespy_amd.inference import VB
    gin = _golden()[1]
    m = _model('b', gin['b_mask'])
    Q = VB(*_nodes(m), engine='fused')
    _on_double(Q)
    np.testing.assert_array_equal(m['Y'].mask, gin['b_mask'])
    np.testing.assert_array_equal(m['Z'].mask, gin['b_mask'].any(axis=1))
    assert m['Z'].mask.shape == (7,) and not m['Z'].mask[4]
    for nm in ('a0', 'A'):
        assert np.all(m[nm].mask) and np.ndim(m[nm].mask) == 0
    m = _model('e', gin['e_mask'], learned=True)
    VB(*_nodes(m), engine='fused')
    assert np.all(m['mu'].mask) and np.all(m['Lambda'].mask)
    m = _model('a', gin['a_mask'])
    VB(*_nodes(m), engine='fused')
    assert m['Z'].mask.shape == () and bool(m['Z'].mask)
    np.testing.assert_array_equal(m['Y'].mask, gin['a_mask'])
    m = _model('a', True)
    VB(*_nodes(m), engine='fused')
    assert np.all(m['Y'].mask) and np.all(m['Z'].mask)


def test_values_at_masked_positions_do_not_matter():
    from hmm_models import run_hmm_cases
    g, gin = _golden()
    base = run_hmm_cases(_mods(_on_double, engine='fused'), gin, only=('b', 'e'))
    for fill in (0.0, 1e3):
        alt = dict(gin)
        for tag in 'be':
            alt[tag + '_y'] = np.where(gin[tag + '_mask'][..., None], gin[tag + '_y'], fill)
        res = run_hmm_cases(_mods(_on_double, engine='fused'), alt, only=('b', 'e'))
        for k, v in base.items():
            if not k.endswith('_plan'):
                np.testing.assert_array_equal(res[k], v, err_msg=k)


def test_reobservation_keeps_the_posteriors():
    """After updates: new data and a new full-shape mask (or none) re-form the sums only."""
    from hmm_models import run_hmm_cases
    g, gin = _golden()
    res = run_hmm_cases(_mods(_on_double, engine='fused'), gin, only=('e',))
    Q = res['e_plan']
    plan = Q.plans[0]
    Y = plan.Y
    A_before = plan.A.get_moments()[0].copy()
    mu_before = plan.mu.get_moments()[0].copy()
    m2 = ~gin['e_mask']
    m2[0] = True
    y2 = np.where(m2[..., None], np.nan_to_num(gin['e_y'], nan=0.25), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter('error')               # no "state discarded" warning
        Y.observe(y2, mask=m2)
        assert Y._plan is plan and plan.has_state()
        np.testing.assert_array_equal(plan.A.get_moments()[0], A_before)
        np.testing.assert_array_equal(plan.mu.get_moments()[0], mu_before)
        np.testing.assert_array_equal(Y.mask, m2)
        np.testing.assert_array_equal(plan.maskd.numpy(), m2.astype(np.uint8))
        from hmm_fused_host import host_pass
        L = plan.layout
        C = plan.state[L.off_C:L.off_C + int(L.KP) * int(L.F2P)].numpy().reshape(-1, int(L.F2P))[:3]
        want = host_pass(y2, C, plan.used_a0.numpy(), plan.used_A.numpy(), mask=m2)
        np.testing.assert_array_equal(plan.Tstat.numpy(), want['T'])
        np.testing.assert_array_equal(plan.xisum.numpy(), want['xisum'])
        # and without a mask: the unmasked pass again
        y3 = np.nan_to_num(gin['e_y'], nan=-0.5)
        Y.observe(y3)
        assert Y._plan is plan and plan.has_state()
        n = plan.kernels.calls.count('pass')
        assert np.isfinite(Q.compute_lowerbound())
        assert plan.maskd is None and plan.kernels.calls.count('pass') == n + 1
        np.testing.assert_array_equal(plan.A.get_moments()[0], A_before)
    # a mask the block cannot take: the existing discard-and-rematch way
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        Y.observe(y3, mask=m2[0])
    assert not plan.has_state() and Y._plan is not plan


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
    return Q, fn


@pytest.mark.parametrize('tag', ['d', 'e'])
def test_save_load_round_trip_with_a_mask(tmp_path, tag):
    Q, fn = _save_load(tmp_path, tag)
    gin = _golden()[1]
    # another mask, or none, on the model: refused with a clear message
    Y = Q.plans[0].Y
    m2 = gin[tag + '_mask'].copy()
    m2[0, 1] = ~m2[0, 1]
    Y.observe(np.nan_to_num(gin[tag + '_y']), mask=m2)
    with pytest.raises(ValueError, match='mask'):
        Q.load(filename=fn)
    Y.observe(np.nan_to_num(gin[tag + '_y']))
    with pytest.raises(ValueError, match='no mask on Y'):
        Q.load(filename=fn)


def test_checkpoint_without_a_mask_keeps_its_format(tmp_path):
    """The entries of an unmasked checkpoint are those of the format before masks (no
    ``plans/0/mask``), and a masked model refuses it."""
    from bayespy_amd.inference import VB
    from hmm_models import run_hmm_cases
    from test_hmm_fused_host import _golden as golden_unmasked
    gin = golden_unmasked()[1]
    Q = run_hmm_cases(_mods(_on_double, engine='fused'), gin, only=('d',))['d_plan']
    names = []
    Q.plans[0].save_state(lambda k, v: names.append(k), None, 0)
    assert sorted(n[len('plans/0/'):] for n in names) == sorted(
        ('delta_roles', 'kind', 'dims', 'flags', 'alpha_a0', 'elog_a0', 'alpha_A', 'elog_A',
         'used_a0', 'used_A', 'z0sum', 'xisum', 'scal', 'bnd', 'Tstat'))
    fn = str(tmp_path / 'plain.ckpt')
    Q.save(filename=fn)
    mk = np.ones(gin['d_y'].shape[:2], dtype=bool)
    mk[1, 2] = False
    Q.plans[0].Y.observe(gin['d_y'], mask=mk)
    with pytest.raises(ValueError, match='no mask on Y'):
        Q.load(filename=fn)
    names = []
    Q.plans[0].save_state(lambda k, v: names.append(k), None, 0)
    assert 'plans/0/mask' in names
    assert VB is not None


# -- the device header on the host ---------------------------------------------------------------------
HOST_SHAPES = [(3, 2, 1, 1), (7, 3, 3, 2), (13, 7, 2, 3), (67, 5, 2, 2), (9, 65, 8, 5), (13, 5, 3, 17),
               (7, 4, 2, 33), (7, 3, 8, 64)]


@pytest.mark.parametrize('B,T,D,K', HOST_SHAPES)
def test_host_build_of_the_masked_pass_against_long_double(B, T, D, K):
    """The rule of DESIGN 4.15: 8 times the deviation of the float64 evaluation of the reference
    formulas from long double, floor 4 ulp of the quantity's magnitude."""
    from hmm_fused_host import host_pass, compare, mixed_mask, nan_fill
    from test_hmm_fused_host import pass_inputs
    Y, C, la0, lA = pass_inputs(B, T, D, K)
    mask = mixed_mask(B, T, np.random.RandomState(B + T))
    Yn = nan_fill(Y, mask)
    got = host_pass(Yn, C, la0, lA, want=True, mask=mask)
    keys = ('z0sum', 'xisum', 'T', 'logZ', 'ge', 'gamma', 'z0', 'zz')
    assert compare(got, Yn, C, la0, lA, keys, label=str((B, T, D, K)), mask=mask) == []
    sums = ('z0sum', 'xisum', 'T', 'logZ', 'ge')
    # the values at masked positions, the optional outputs: the same bits
    for fill in (0.0, 1e300):
        alt = host_pass(nan_fill(Y, mask, fill), C, la0, lA, mask=mask)
        for k in sums:
            np.testing.assert_array_equal(alt[k], got[k], err_msg=k)
    # a mask of ones: the bits of mask=None
    ref = host_pass(Y, C, la0, lA, want=True)
    one = host_pass(Y, C, la0, lA, want=True, mask=np.ones((B, T), dtype=bool))
    for k in keys:
        np.testing.assert_array_equal(one[k], ref[k], err_msg=k)
    # a mask of zeros: nothing
    z = host_pass(Yn, C, la0, lA, mask=np.zeros((B, T), dtype=bool))
    assert not np.any(z['z0sum']) and not np.any(z['xisum']) and not np.any(z['T'])
    assert z['logZ'] == 0 and z['ge'] == 0
    # the prior pass
    assert compare(host_pass(Yn, None, la0, lA, mask=mask), Yn, None, la0, lA, mask=mask) == []
    # fixed labels: T over the observed steps, z0sum and xisum over the chains with one
    lab = np.random.RandomState(0).randint(K, size=(B, T))
    r = host_pass(Yn, C, la0, lA, labels=lab, want=True, mask=mask)
    check_labels(r, lab, Y, mask, K)


def check_labels(r, lab, Y, mask, K):
    D = Y.shape[-1]
    onehot = np.eye(K)[lab]
    ob = mask.any(axis=1)
    np.testing.assert_array_equal(r['gamma'][ob], onehot[ob])
    np.testing.assert_array_equal(r['z0sum'], onehot[ob, 0].sum(0))
    np.testing.assert_array_equal(r['xisum'],
                                  np.einsum('bti,btj->ij', onehot[ob, :-1], onehot[ob, 1:]))
    om = onehot * mask[..., None]
    np.testing.assert_array_equal(r['T'][:, 0], om.sum((0, 1)))
    np.testing.assert_allclose(r['T'][:, 1:1 + D],
                               np.einsum('btk,btd->kd', om, np.where(mask[..., None], Y, 0.0)),
                               rtol=1e-13, atol=1e-13)
    assert r['logZ'] == 0 and r['ge'] == 0


# -- the C ABI -----------------------------------------------------------------------------------------
def test_cabi_declares_the_masked_entry_point():
    """Fails without the feature: the library has no such symbol."""
    from bayespy_amd import _lib
    lib = _lib.load()
    name = 'vmp_hmm_fused_pass_masked'
    assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    # the arguments of vmp_hmm_fused_pass plus the mask, after the labels
    plain, masked = _lib.SIGNATURES['vmp_hmm_fused_pass'], _lib.SIGNATURES[name]
    assert masked[0] is plain[0] and len(masked[1]) == len(plain[1]) + 1
    assert list(masked[1][:11]) == list(plain[1][:11]) and list(masked[1][12:]) == list(plain[1][11:])
    # no masked limit of its own: every instance builds without scratch memory
    assert 'vmp_hmm_fused_mask_limits' not in _lib.header_symbols()
    from bayespy_amd.inference.plans.hmm import hmm_limits
    assert hmm_limits() == (64, 8)


def test_cabi_masked_pass_checks_its_arguments():
    """Without a context nothing is launched: the checks of vmp_hmm_fused_pass in its order, with
    and without a mask."""
    from bayespy_amd import _lib
    lib = _lib.load()
    U, I = _lib.VMP_ERR_UNSUPPORTED, _lib.VMP_ERR_INVALID
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    for mask in (p, None):
        def call(B=4, T=3, D=2, K=3, ctx=None, C=p, ldc=6, a0=p, A=p, ws=p, z0sum=p, xisum=p, Ts=p,
                 scal=p, Y=p):
            return lib.vmp_hmm_fused_pass_masked(ctx, B, T, D, K, Y, C, ldc, a0, A, None, mask, ws,
                                                 z0sum, xisum, Ts, scal, None, None, None)
        assert call() == I                                  # a null context
        for kw in (dict(B=-1), dict(T=1), dict(T=-3), dict(D=0), dict(K=0), dict(K=-2)):
            assert call(**kw) == I, kw
        assert call(K=65) == U and call(D=9) == U
        assert call(K=65, ldc=1) == U                       # the shape is judged first
        assert call(ldc=5) == I                             # below the 6 features of D = 2
        assert call(C=None, ldc=0) == I                     # fine but for the context
