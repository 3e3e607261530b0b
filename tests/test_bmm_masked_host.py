"""CPU: the fused Bernoulli-mixture block with missing observations, without a device -- the
matcher on full-shape, scalar and broadcasting masks, the plan's host logic on the kernel double
tests/bmm_masked_host.py (CPUBMMMaskedKernels) against every fixture of
tests/golden/bmm_masked.npz (live reference, tools/make_golden_bmm_masked.py), re-observation, a
save / load round trip, hidden entries flipped or NaN, the g++ build of the device header
csrc/vmp_bmm_dev.h against a long-double restatement, the sanitizer program and the C ABI."""
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


def _mods(after=None, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    m = dict(nodes=nodes, VB=VB, vb_kwargs=kw)
    if after is not None:
        m['after_vb'] = after
    return m


def _on_double(Q):
    from bayespy_amd.device import Runtime
    from bmm_masked_host import CPUBMMMaskedKernels
    plan = Q.plans[0]
    assert type(plan).__name__ == 'BernoulliMixturePlan'
    rt = Runtime(device='cpu')
    plan._rt, plan._kernels = rt, CPUBMMMaskedKernels(rt)


def _golden():
    g = np.load(os.path.join(GOLDEN, 'bmm_masked.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


def _model(tag='c'):
    from bmm_masked_models import build_bmm_masked
    gin = _golden()[1]
    m = build_bmm_masked(_mods(), gin[tag + '_x'], gin[tag + '_mask'], gin[tag + '_p0'].shape[1])
    m['P'].initialize_from_value(gin[tag + '_p0'])
    return m


def _nodes(m):
    return [m['Z'], m['R'], m['X'], m['P']]


def check_fixture(res, g, tags):
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan'):
            continue
        if k.endswith('_mask'):
            np.testing.assert_array_equal(np.broadcast_to(v, g[k].shape), g[k], err_msg=k)
            assert np.shape(v) == g[k].shape, k
        elif k.endswith('_u0'):
            np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        elif k.endswith('_L'):
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL)
        else:                                   # per-node terms: some are near zero
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL, atol=1e-9)
        checked += 1
    assert checked == len(tags) * (1 + 4 + 3 + 2)


# -- the matcher -------------------------------------------------------------------------------------
def test_matcher_takes_a_full_shape_mask_and_declines_the_others():
    from bayespy_amd.inference.plans.bmm import BernoulliMixturePlan
    gin = _golden()[1]
    x, mask = np.nan_to_num(gin['c_x']).astype(np.int64), gin['c_mask']
    N, D = x.shape
    m = _model()
    why = []
    assert BernoulliMixturePlan.match(_nodes(m), why) is not None and why == []
    for bad in (False, mask[:, :1], mask[:1]):
        m = _model()
        m['X'].observe(x, mask=bad)
        why = []
        assert BernoulliMixturePlan.match(_nodes(m), why) is None and len(why) == 1
        assert 'mask of shape %s' % (np.shape(bad),) in why[0]
        assert 'full shape' in why[0] and str((N, D)) in why[0]
    assert 'mask of the full shape (N, D)' in BernoulliMixturePlan.describe()


def test_engine_fused_builds_the_block_for_a_masked_model():
    """Fails without the feature: NotImplementedError, 'it has a mask'."""
    from bayespy_amd.inference import VB
    m = _model()
    Q = VB(*_nodes(m), engine='fused')
    assert type(Q.plans[0]).__name__ == 'BernoulliMixturePlan'


# -- the plan on the kernel double ---------------------------------------------------------------------
def test_plan_reproduces_every_fixture_on_the_kernel_double():
    from bmm_masked_models import run_masked_cases, CASES, N_ITER
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_masked_cases(_mods(_on_double, engine='fused'), gin)
    check_fixture(res, g, CASES)
    calls = res['a_plan'].plans[0].kernels.calls
    assert calls.count('pass_masked') == 1 + N_ITER and calls.count('pass_masked_r') == 1
    assert calls.count('pack_masked') == 1 and 'pass' not in calls and 'pack' not in calls
    # what the issue's run on the reference showed, on this plan
    plan = res['c_plan'].plans[0]
    Zm = g['c_Z_mask'][:, 0]
    assert Zm.sum() == Zm.size - 1 and not Zm[4]
    np.testing.assert_allclose(plan.Nk.numpy().sum(), Zm.size - 1, rtol=1e-12)
    z = res['c_Z_u0'][4, 0]
    assert np.all(np.isfinite(z)) and abs(z.sum() - 1) < 1e-12
    # the never-observed column keeps the prior: counts are exactly zero
    assert np.all(plan.counts.numpy().reshape(65, 3, 2)[9] == 0)


def test_a_mask_of_ones_reproduces_case_a_of_the_unmasked_fixture():
    from bmm_masked_models import run_masked_cases
    g, gin = _golden()
    f = np.load(os.path.join(GOLDEN, 'bmm_fused.npz'))
    res = run_masked_cases(_mods(_on_double, engine='fused'), gin, only=('d',), n_iter=4)
    np.testing.assert_allclose(res['d_L'], f['a_L'], rtol=L_RTOL)
    for nm in ('R', 'Z', 'P', 'X'):
        np.testing.assert_allclose(res['d_%s_Lterm' % nm], f['a_%s_Lterm' % nm], rtol=L_RTOL,
                                   atol=1e-9)
    for nm in ('R', 'P', 'Z'):
        np.testing.assert_allclose(res['d_%s_u0' % nm], f['a_%s_u0' % nm], **MOM_TOL)


def test_reobserve_keeps_the_posteriors():
    from bmm_masked_models import run_masked_cases
    g, gin = _golden()
    Q = run_masked_cases(_mods(_on_double, engine='fused'), gin, only=('c',))['c_plan']
    plan = Q.plans[0]
    X, P, R = Q['X'], Q['P'], Q['R']
    p, r = P.get_moments()[0], R.get_moments()[0]
    x, mask = np.nan_to_num(gin['c_x']).astype(np.int64), gin['c_mask']
    S0, M0 = plan.S.numpy().copy(), plan.M.numpy().copy()
    perm = np.random.RandomState(0).permutation(x.shape[0])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        X.observe(x[perm].astype(bool), mask=mask[perm])
    assert Q.plans[0] is plan
    np.testing.assert_array_equal(P.get_moments()[0], p)
    np.testing.assert_array_equal(R.get_moments()[0], r)
    # the same multiset of rows: the same statistics up to the order of the additions
    np.testing.assert_allclose(plan.S.numpy(), S0, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(plan.M.numpy(), M0, rtol=1e-12, atol=1e-13)
    assert plan.kernels.calls.count('pack_masked') == 2
    np.testing.assert_array_equal(X.mask, mask[perm])
    np.testing.assert_array_equal(Q['Z'].mask, mask[perm].any(axis=1)[:, None])


def test_save_load_round_trip_and_a_changed_mask_is_refused(tmp_path):
    from bmm_masked_models import run_masked_cases
    g, gin = _golden()
    Q = run_masked_cases(_mods(_on_double, engine='fused'), gin, only=('c',), n_iter=4)['c_plan']
    fn = str(tmp_path / 'bmm_masked.ckpt')
    Q.save(filename=fn)
    L4 = Q.L[:4].copy()
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    assert Q.iter == 4
    np.testing.assert_array_equal(Q.L[:4], L4)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)
    x, mask = np.nan_to_num(gin['c_x']).astype(np.int64), gin['c_mask'].copy()
    mask[0, 0] = not mask[0, 0]
    Q['X'].observe(np.where(mask, x, 0), mask=mask)
    with pytest.raises(ValueError, match='checkpoint was saved with a mask on X with'):
        Q.load(filename=fn)


def test_hidden_entries_flipped_or_nan_leave_the_same_bits():
    from bmm_masked_models import run_masked_cases
    from bmm_masked_host import host_pack_masked
    g, gin = _golden()
    x, mask = np.nan_to_num(gin['c_x']).astype(np.int64), gin['c_mask']
    a = run_masked_cases(_mods(_on_double, engine='fused'), gin, only=('c',))
    import bmm_masked_models as models
    orig = models.build_bmm_masked
    models.build_bmm_masked = lambda *args, **kw: _flip(orig, *args, **kw)
    try:
        b = run_masked_cases(_mods(_on_double, engine='fused'), gin, only=('c',))
    finally:
        models.build_bmm_masked = orig
    for k in a:
        if not k.endswith('_plan'):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    # NaN, -1 and 7 at hidden positions: the same words and no flag; an observed 7 sets the flag
    want, flag = host_pack_masked(x.astype(np.float64), mask)
    assert flag == 0
    for v in (np.nan, -1.0, 7.0):
        got, flag = host_pack_masked(np.where(mask, x, v).astype(np.float64), mask)
        assert flag == 0
        np.testing.assert_array_equal(got, want)
    bad = x.astype(np.float64)
    i, j = np.argwhere(mask)[17]
    bad[i, j] = 7
    assert host_pack_masked(bad, mask)[1] == 1


def _flip(orig, mods, xx, mm, K, **kw):
    """The script of bmm_masked_models with the hidden entries set to one instead of zero."""
    m = orig(mods, xx, mm, K, **kw)
    m['X'].observe(np.where(mm, np.nan_to_num(xx), 1).astype(np.int64), mask=mm)
    return m


# -- the device header on the host ---------------------------------------------------------------------
@pytest.mark.parametrize('D', [63, 64, 65])
def test_pack_masked_planes(D):
    from bmm_masked_host import host_pack_masked, bmmm_host
    from bmm_host import host_unpack
    rs = np.random.RandomState(D)
    x = rs.randint(2, size=(37, D))
    m = rs.rand(37, D) < 0.7
    m[0], m[1] = False, True
    W = (D + 63) // 64
    for a in (x.astype(np.int64), x.astype(np.float64), x.astype(bool)):
        xw, flag = host_pack_masked(a, m)
        assert flag == 0 and xw.shape == (37, 2 * bmmm_host().bmmm_words(D)) == (37, 2 * W)
        np.testing.assert_array_equal(host_unpack(np.ascontiguousarray(xw[:, :W]), D), x * m)
        np.testing.assert_array_equal(host_unpack(np.ascontiguousarray(xw[:, W:]), D), m)
        if D % 64:                                                     # unused high bits are zero
            assert not np.any(xw[:, W - 1] >> np.uint64(D % 64))
            assert not np.any(xw[:, 2 * W - 1] >> np.uint64(D % 64))


@pytest.mark.parametrize('N,D,K', [(0, 5, 3), (1, 1, 1), (65, 63, 2), (300, 65, 15), (257, 64, 16),
                                   (515, 70, 17), (763, 257, 64)])
def test_host_build_of_the_masked_pass_against_long_double(N, D, K):
    """The tolerance rule of DESIGN 4.14 on r, N_k, S, M, sum lse, N_k . c and S . w + M . l0: 8
    times the deviation of the float64 NumPy evaluation from long double, floor 4 ulp."""
    from bmm_masked_host import (host_pack_masked, host_pass_masked, restate_masked, tolerances,
                                 error, mixed_mask, bmmm_host, QUANTITIES)
    rs = np.random.RandomState(N + D + K)
    assert bmmm_host().bmmm_chunk_rows(N, D, K) == 256
    x = rs.randint(2, size=(N, D)).astype(np.int64)
    m = mixed_mask(N, D, rs)
    w = rs.normal(size=(D, K))
    l0 = -rs.gamma(1.0, size=(D, K))
    c = rs.normal(size=K)
    c -= c.max()
    xw, _ = host_pack_masked(x, m)
    h = host_pass_masked(N, D, K, xw, None, w, l0, c, want_r=True)
    ld, f64 = restate_masked(x, m, w, l0, c), restate_masked(x, m, w, l0, c, np.float64)
    tol, dev = tolerances(ld, f64)
    for key in QUANTITIES:
        err = error(h[key], ld[key])
        print('%s (N, D, K) = %s: float64 deviation %.3g, host build %.3g, allowed %.3g'
              % (key, (N, D, K), dev[key], err, tol[key]))
        assert err <= tol[key], (key, err, tol[key])
    np.testing.assert_array_equal(h['counts'][:, 0], h['S'].reshape(-1))
    np.testing.assert_array_equal(h['counts'][:, 1], (h['M'] - h['S']).reshape(-1))
    # fixed labels: exact integer counts over the rows with an observed entry, lse = 0
    lab = rs.randint(K, size=N).astype(np.int32)
    h = host_pass_masked(N, D, K, xw, lab, w, l0, c, want_r=True)
    obs = m.any(axis=1)
    one = np.eye(K)[lab]
    np.testing.assert_array_equal(h['Nk'], (one * obs[:, None]).sum(0))
    np.testing.assert_array_equal(h['S'], (x * m).T @ one)
    np.testing.assert_array_equal(h['M'], m.astype(float).T @ one)
    np.testing.assert_array_equal(h['r'], one)
    assert h['sum_lse'] == 0


def test_host_source_under_the_sanitizers_as_a_program_of_its_own():
    """tests/host/bmm_masked_host_main.cpp: the host source on two shapes ((333, 70, 5): N and D no
    multiples of 64, a row and a column of nothing, NaN at hidden positions; (64, 128, 64)), built
    with -fsanitize=address,undefined and run as a program, never loaded into python."""
    from bmm_masked_host import build_sanitized_program
    exe = build_sanitized_program()
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                       timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.count('sum M') == 4 and 'ERROR' not in r.stdout \
        and 'runtime error' not in r.stdout


# -- the C ABI -----------------------------------------------------------------------------------------
def test_cabi_declares_the_masked_entry_points():
    """Fails without the feature: the library has no such symbols."""
    from bayespy_amd import _lib
    from bmm_masked_host import bmmm_host
    lib = _lib.load()
    for name in ('vmp_bmm_limits_masked', 'vmp_bmm_plan_masked', 'vmp_bmm_pack_masked',
                 'vmp_bmm_tables_masked', 'vmp_bmm_pass_masked'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    from bayespy_amd.inference.plans.bmm import (bmm_masked_limits, BMM_MASKED_MAX_K,
                                                 BMM_MASKED_MAX_D)
    host = bmmm_host()
    assert bmm_masked_limits() == (host.bmmm_max_k(), host.bmmm_max_d()) == (64, 1024) \
        == (BMM_MASKED_MAX_K, BMM_MASKED_MAX_D)
    assert lib.vmp_bmm_limits_masked(None, None) == _lib.VMP_ERR_INVALID
    c, w = ctypes.c_int64(), ctypes.c_int64()
    for N, D, K in ((0, 1, 1), (1000, 70, 5), (10 ** 7, 64, 32), (10 ** 6, 1024, 64),
                    (10 ** 9, 1024, 64)):
        assert lib.vmp_bmm_plan_masked(N, D, K, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_OK
        rows, nc = host.bmmm_chunk_rows(N, D, K), host.bmmm_chunks(N, D, K)
        assert c.value == rows and w.value == nc * host.bmmm_partial_doubles(D, K) + 1024 + 2
        assert rows % 64 == 0 and rows >= 256 and nc <= 1024 and nc * rows >= N
        assert nc * host.bmmm_partial_doubles(D, K) * 8 <= 2 ** 28
    bad = lib.vmp_bmm_plan_masked
    assert bad(10, 4, 65, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_ERR_UNSUPPORTED
    assert bad(10, 1025, 4, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_ERR_UNSUPPORTED
    assert bad(-1, 4, 4, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_ERR_INVALID
    assert bad(10, 4, 4, None, None) == _lib.VMP_ERR_INVALID
