"""GPU: the fused diagonal-Gaussian-mixture block with missing observations
(inference/plans/dgmm_masked.py, csrc/vmp_dgmm_masked.hip) -- the pack and the pass through the C
ABI against a long-double restatement at sizes that cross lane-group, column-block, tile and chunk
boundaries, an all-hidden mask, bit-identity (two calls, the r output, NaN / 1e300 / -inf at the
hidden positions of the caller's y), a mask of ones against the unmasked pass, fixed labels, the
updates of both nodes, the argument checks, and the fixtures through ``VB(..., engine='fused')``."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

MID = (300, 70, 5)
# the shapes of tests/test_dgmm_gpu.py with D on both sides of the column block of 32
SHAPES = sorted(set([(MID[0], MID[1], K) for K in (1, 2, 15, 16, 17, 64)]
                    + [(MID[0], D, MID[2]) for D in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257)]
                    + [(N, MID[1], MID[2]) for N in (0, 1, 63, 65, 257, 763)]
                    + [(763, 257, 64)]))
BITS = ('S1', 'S2', 'M', 'Nk', 'sum_lse', 'Nk_c', 'S_hqg')


def _kernels():
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.dgmm_masked import MaskedDGMMKernels
    rt = get_runtime()
    rt.sync_stream()
    return rt, MaskedDGMMKernels(rt)


def _up(rt, a, dtype=np.float64):
    return rt.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(rt.device)


def _device_pack(y, mask):
    """(packed y as a device tensor, number of observed entries)."""
    rt, k = _kernels()
    N, D = y.shape
    out = rt.empty(max(N, 1), D)
    count = rt.torch.zeros(1, dtype=rt.torch.int64, device=rt.device)
    k.pack_masked(N, D, _up(rt, y) if N else None, _up(rt, mask, np.uint8) if N else None,
                  out if N else None, count)
    rt.synchronize()
    return out[:N], int(count.cpu().numpy()[0])


def _device_tables(D, K, mu_mom, tau_mom, elog_pi):
    rt, k = _kernels()
    h, q, g, c = rt.empty(D, K), rt.empty(D, K), rt.empty(D, K), rt.empty(K)
    k.tables_masked(D, K, None if mu_mom is None else _up(rt, mu_mom),
                    None if tau_mom is None else _up(rt, tau_mom), _up(rt, elog_pi), h, q, g, c)
    rt.synchronize()
    return tuple(t.cpu().numpy() for t in (h, q, g, c))


def _device_pass(N, D, K, yp, h, q, g, c, labels=None, want_r=False):
    """dict of S1, S2, M, Nk, sum_lse, Nk_c, S_hqg and r (or None) of vmp_dgmm_pass_masked as host
    arrays; ``yp`` the packed device tensor."""
    rt, k = _kernels()
    chunk, wsd = k.plan_masked(N, D, K)
    assert chunk == 256
    S1, S2, M, Nk, scal = rt.empty(D, K), rt.empty(D, K), rt.empty(D, K), rt.empty(K), rt.zeros(8)
    ws = rt.empty(int(wsd))
    r = rt.empty(N, K) if want_r and N else None
    lab = None if labels is None else _up(rt, labels, np.int32)
    k.pass_masked(N, D, K, yp if N else None, lab, _up(rt, h), _up(rt, q), _up(rt, g), _up(rt, c),
                  ws, S1, S2, M, Nk, scal, r)
    rt.synchronize()
    s = scal.cpu().numpy()
    return dict(S1=S1.cpu().numpy(), S2=S2.cpu().numpy(), M=M.cpu().numpy(), Nk=Nk.cpu().numpy(),
                sum_lse=s[0], Nk_c=s[1], S_hqg=s[2],
                r=np.zeros((0, K)) if want_r and not N else None if r is None else r.cpu().numpy())


def _device_update(D, K, which, prior_a, prior_b, S1, S2, M, other):
    rt, k = _kernels()
    par, mom, bound = rt.empty(D * K, 2), rt.empty(D * K, 2), rt.zeros(1)
    opt = lambda a: None if a is None else _up(rt, a)     # noqa: E731
    k.update_masked(D, K, which, _up(rt, np.broadcast_to(prior_a, (D, K))),
                    _up(rt, np.broadcast_to(prior_b, (D, K))), opt(S1), opt(S2), opt(M),
                    opt(other), par, mom, bound)
    rt.synchronize()
    return par.cpu().numpy(), mom.cpu().numpy(), float(bound.cpu().numpy()[0])


def _inputs(N, D, K):
    from dgmm_host import make_inputs
    from dgmm_masked_host import host_tables_masked, mixed_mask
    g = make_inputs(N, D, K)
    m = mixed_mask(N, D)
    return g, m, host_tables_masked(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_pass_against_long_double_restatement(N, D, K):
    from dgmm_host import tolerances, error
    from dgmm_masked_host import (host_pack_masked, host_pass_masked, restate_masked_pass,
                                  junk_at_hidden, dgmmm_host, PASS_QUANTITIES)
    # 763 rows: three chunks of 256 with a ragged last one
    assert dgmmm_host().dgmmm_chunks(N, D, K) == (N + 255) // 256
    g, m, (hh, hq, hg, hc) = _inputs(N, D, K)
    h, q, gt, c = _device_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])
    for a, b in ((h, hh), (q, hq), (gt, hg), (c, hc)):
        np.testing.assert_allclose(a, b, rtol=1e-14, atol=1e-13)
    assert c.max() == 0
    y = junk_at_hidden(g['y'], m, np.nan)
    yp, count = _device_pack(y, m)
    hyp, hcount = host_pack_masked(y, m)
    assert count == hcount == m.sum()
    np.testing.assert_array_equal(yp.cpu().numpy().view(np.uint64), hyp.view(np.uint64))
    got = _device_pass(N, D, K, yp, h, q, gt, c, want_r=True)
    host = host_pass_masked(N, D, K, hyp, None, h, q, gt, c, want_r=True)
    ld = restate_masked_pass(g['y'], m, h, q, gt, c)
    f64 = restate_masked_pass(g['y'], m, h, q, gt, c, np.float64)
    tol, dev = tolerances(ld, f64, PASS_QUANTITIES)
    for key in PASS_QUANTITIES:
        err, herr = error(got[key], ld[key]), error(host[key], ld[key])
        print('%s (N, D, K) = %s: float64 deviation %.3g, kernel %.3g, host build %.3g, allowed '
              '%.3g' % (key, (N, D, K), dev[key], err, herr, tol[key]))
        assert err <= tol[key], (key, err, tol[key])
        assert herr <= tol[key], ('host', key, herr, tol[key])
    if N > 2:                                       # the row of nothing: softmax(c), in no sum
        assert not m[2].any()
        soft = np.exp(c.astype(np.longdouble))
        assert error(got['r'][2], soft / soft.sum()) <= max(tol['r'], 4 * np.spacing(1.0))
    if D > 2:                                       # the column of nothing: exact zeros
        assert not got['M'][1].any() and not got['S1'][1].any() and not got['S2'][1].any()


def test_an_all_hidden_mask_gives_zeros_and_softmax_rows():
    N, D, K = 65, 17, 5
    g, _, (h, q, gt, c) = _inputs(N, D, K)
    yp, count = _device_pack(g['y'], np.zeros((N, D), dtype=bool))
    got = _device_pass(N, D, K, yp, h, q, gt, c, want_r=True)
    assert count == 0 and got['sum_lse'] == 0 and got['Nk_c'] == 0 and got['S_hqg'] == 0
    for key in ('S1', 'S2', 'M', 'Nk'):
        assert not got[key].any(), key
    soft = np.exp(c) / np.exp(c).sum()
    np.testing.assert_allclose(got['r'], np.broadcast_to(soft, (N, K)), rtol=1e-14)
    assert np.all(got['r'] == got['r'][0])


@pytest.mark.parametrize('N,D,K', [MID, (763, 257, 64), (257, 64, 16)])
def test_two_calls_the_r_output_and_junk_at_hidden_entries_leave_the_same_bits(N, D, K):
    from dgmm_masked_host import junk_at_hidden
    g, m, (h, q, gt, c) = _inputs(N, D, K)
    yp, _ = _device_pack(junk_at_hidden(g['y'], m, 0.0), m)
    a = _device_pass(N, D, K, yp, h, q, gt, c, want_r=True)
    b = _device_pass(N, D, K, yp, h, q, gt, c, want_r=True)
    n = _device_pass(N, D, K, yp, h, q, gt, c, want_r=False)
    for key in BITS + ('r',):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    for key in BITS:
        np.testing.assert_array_equal(a[key], n[key], err_msg=key)
    assert np.all(np.isfinite(a['r'])) and all(np.all(np.isfinite(a[key])) for key in BITS)
    for junk in (np.nan, 1e300, -np.inf):
        yj, _ = _device_pack(junk_at_hidden(g['y'], m, junk), m)
        np.testing.assert_array_equal(yj.cpu().numpy().view(np.uint64),
                                      yp.cpu().numpy().view(np.uint64))
        j = _device_pass(N, D, K, yj, h, q, gt, c, want_r=True)
        for key in BITS + ('r',):
            np.testing.assert_array_equal(a[key], j[key], err_msg='%s with %r' % (key, junk))


@pytest.mark.parametrize('N,D,K', [MID, (257, 64, 16)])
def test_a_mask_of_ones_against_the_unmasked_pass(N, D, K):
    """Each pass within its own allowance of the common long-double value (not bit for bit: c is
    formed differently, sum_d g is inside it there and a product here)."""
    from dgmm_host import host_tables, restate_pass, tolerances, error
    from dgmm_masked_host import restate_masked_pass
    from test_dgmm_gpu import _device_pass as plain_pass
    g, _, (h, q, gt, c) = _inputs(N, D, K)
    ones = np.ones((N, D), dtype=bool)
    yp, count = _device_pack(g['y'], ones)
    assert count == N * D
    np.testing.assert_array_equal(yp.cpu().numpy(), g['y'])
    got = _device_pass(N, D, K, yp, h, q, gt, c, want_r=True)
    ph, pq, pc, _ = host_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])
    plain = plain_pass(N, D, K, g['y'], ph, pq, pc, want_r=True)
    ld = restate_masked_pass(g['y'], ones, h, q, gt, c)
    f64 = restate_masked_pass(g['y'], ones, h, q, gt, c, np.float64)
    keys = ('r', 'Nk', 'S1', 'S2')
    tol, _ = tolerances(ld, f64, keys)
    pld, pf64 = restate_pass(g['y'], ph, pq, pc), restate_pass(g['y'], ph, pq, pc, np.float64)
    ptol, _ = tolerances(pld, pf64, keys)
    for key in keys:
        assert error(got[key], ld[key]) <= tol[key], key
        assert error(plain[key], pld[key]) <= ptol[key], key
        # the two long-double values are one value up to the constant taken out of c
        assert error(np.asarray(pld[key], dtype=np.float64), ld[key]) <= tol[key] + ptol[key], key
    np.testing.assert_array_equal(got['M'], np.broadcast_to(got['M'][:1], (D, K)))
    assert error(got['M'][0], ld['Nk']) <= tol['Nk']


@pytest.mark.parametrize('N,D,K', [(763, 70, 17), (300, 257, 5)])
def test_fixed_labels_give_one_hot_rows_and_integer_counts(N, D, K):
    from dgmm_host import tolerances, error
    g, m, (h, q, gt, c) = _inputs(N, D, K)
    yp, _ = _device_pack(g['y'], m)
    got = _device_pass(N, D, K, yp, h, q, gt, c, labels=g['labels'], want_r=True)
    one = np.eye(K)[g['labels']]
    np.testing.assert_array_equal(got['r'], one)
    assert not m[2].any()
    np.testing.assert_array_equal(got['Nk'], (one * m.any(axis=1)[:, None]).sum(0))
    np.testing.assert_array_equal(got['M'], m.astype(float).T @ one)
    assert got['sum_lse'] == 0
    yt = np.where(m, g['y'], 0.0)
    ld = dict(S1=yt.astype(np.longdouble).T @ one, S2=(yt.astype(np.longdouble) ** 2).T @ one)
    f64 = dict(S1=yt.T @ one, S2=(yt * yt).T @ one)
    tol, _ = tolerances(ld, f64, ('S1', 'S2'))
    for key in ('S1', 'S2'):
        assert error(got[key], ld[key]) <= tol[key], key


@pytest.mark.parametrize('N,D,K', [MID, (300, 70, 17), (65, 1, 5)])
def test_updates_of_both_nodes_against_the_restatement(N, D, K):
    from dgmm_host import tolerances, error
    from dgmm_masked_host import (host_pack_masked, host_pass_masked, restate_masked_update,
                                  UPDATE_QUANTITIES)
    g, m, (h, q, gt, c) = _inputs(N, D, K)
    o = host_pass_masked(N, D, K, host_pack_masked(g['y'], m)[0], None, h, q, gt, c)
    args = (g['m0'], g['beta0'], g['a0'], g['b0'], o['S1'], o['S2'], o['M'], g['mu_mom'],
            g['tau_mom'])
    ld, f64 = restate_masked_update(*args), restate_masked_update(*args, dtype=np.float64)
    tol, dev = tolerances(ld, f64, UPDATE_QUANTITIES)
    pm, mm, bm = _device_update(D, K, 0, g['m0'], g['beta0'], o['S1'], o['S2'], o['M'],
                                g['tau_mom'])
    pt, mt, bt = _device_update(D, K, 1, g['a0'], g['b0'], o['S1'], o['S2'], o['M'], g['mu_mom'])
    got = dict(mu_mom=mm, mu_bound=bm, tau_mom=mt, tau_bound=bt, mu_par=pm, tau_par=pt)
    for key in UPDATE_QUANTITIES:
        err = error(got[key], ld[key])
        print('%s (N, D, K) = %s: float64 deviation %.3g, kernel %.3g, allowed %.3g'
              % (key, (N, D, K), dev[key], err, tol[key]))
        assert err <= tol[key], (key, err, tol[key])
    # null statistics: the prior, bound exactly zero
    par, mom, bound = _device_update(D, K, 1, g['a0'], g['b0'], None, None, None, None)
    np.testing.assert_array_equal(par.reshape(D, K, 2)[..., 0], g['a0'])
    assert bound == 0


# -- end to end ------------------------------------------------------------------------------------------
def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    return dict(nodes=nodes, VB=VB, vb_kwargs=kw)


def test_fixtures_on_the_fused_block(golden_dir):
    """Fails without the feature: NotImplementedError ('it has a mask') from
    VB(..., engine='fused')."""
    from dgmm_masked_models import run_masked_cases, CASES
    from test_dgmm_masked_host import check_fixture
    from bayespy_amd.inference.plans.dgmm_masked import MaskedDiagGaussianMixturePlan
    g = np.load(os.path.join(golden_dir, 'dgmm_masked.npz'))
    gin = {k[3:]: g[k] for k in g.files if k.startswith('in_')}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_masked_cases(_mods(engine='fused'), gin)
    for tag in CASES:
        assert isinstance(res[tag + '_plan'].plans[0], MaskedDiagGaussianMixturePlan)
    check_fixture(res, g, CASES)


def test_the_example():
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import diag_gaussian_mixture_missing
    out = diag_gaussian_mixture_missing.run(N=500, D=70, K=4, sweeps=8, verbose=False)
    assert out['plan'] == 'MaskedDiagGaussianMixturePlan' and np.all(np.diff(out['L']) > -1e-6)
    assert out['accuracy'] > 0.9


# -- argument checks: nothing is launched ------------------------------------------------------------------
def test_argument_checks_and_limits():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(16)
    p = ctypes.c_void_p(z.data_ptr())
    ok = [p] * 13                       # y, labels, h, q, g, c, ws, S1, S2, M, Nk, scal, r_out
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11):
        args = list(ok)
        args[i] = None
        assert lib.vmp_dgmm_pass_masked(ctx, 4, 4, 4, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_dgmm_pass_masked(None, 4, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_dgmm_pass_masked(ctx, -1, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_dgmm_pass_masked(ctx, 4, 0, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_dgmm_pass_masked(ctx, 4, 4, 65, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_dgmm_pass_masked(ctx, 4, 1025, 4, *ok) == _lib.VMP_ERR_UNSUPPORTED
    t = [p] * 7                                 # mu_mom, tau_mom, elog_pi, h, q, g, c
    for i in (2, 3, 4, 5, 6):
        args = list(t)
        args[i] = None
        assert lib.vmp_dgmm_tables_masked(ctx, 4, 4, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_dgmm_tables_masked(ctx, 4, 65, *t) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_dgmm_tables_masked(ctx, 1025, 4, *t) == _lib.VMP_ERR_UNSUPPORTED
    u = [p] * 9                                 # prior_a, prior_b, S1, S2, M, other, par, mom, bound
    for i in (0, 1, 6, 7, 8):
        args = list(u)
        args[i] = None
        assert lib.vmp_dgmm_update_masked(ctx, 4, 4, 0, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_dgmm_update_masked(ctx, 4, 4, 2, *u) == _lib.VMP_ERR_INVALID
    assert lib.vmp_dgmm_update_masked(ctx, 4, 65, 0, *u) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_dgmm_update_masked(ctx, 1025, 4, 1, *u) == _lib.VMP_ERR_UNSUPPORTED
    k4 = [p] * 4                                # y, mask, y_packed, n_observed
    for i in range(4):
        args = list(k4)
        args[i] = None
        assert lib.vmp_dgmm_pack_masked(ctx, 2, 2, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_dgmm_pack_masked(ctx, -1, 2, *k4) == _lib.VMP_ERR_INVALID
    assert lib.vmp_dgmm_pack_masked(ctx, 2, 1025, *k4) == _lib.VMP_ERR_UNSUPPORTED
    k, d = ctypes.c_int32(), ctypes.c_int32()
    assert lib.vmp_dgmm_limits_masked(ctypes.byref(k), ctypes.byref(d)) == _lib.VMP_OK
    assert (k.value, d.value) == (64, 1024)
