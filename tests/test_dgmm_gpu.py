"""GPU: the fused diagonal-Gaussian-mixture block (inference/plans/dgmm.py, csrc/vmp_dgmm.hip) --
the pass through the C ABI against a long-double restatement at sizes that cross lane-group,
column-block, tile and chunk boundaries, bit-identity, fixed labels, the updates of both nodes,
the argument checks, and the fixtures through ``VB(..., engine='fused')``."""
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
# one dimension at a time around MID; D = 63 and 65: one value on each side of the column block
SHAPES = sorted(set([(MID[0], MID[1], K) for K in (1, 2, 15, 16, 17, 64)]
                    + [(MID[0], D, MID[2]) for D in (1, 15, 16, 17, 63, 64, 65, 257)]
                    + [(N, MID[1], MID[2]) for N in (0, 1, 63, 65, 257, 763)]
                    + [(763, 257, 64)]))
BITS = ('S1', 'S2', 'Nk', 'sum_lse', 'Nk_c', 'S_hq')


def _kernels():
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.dgmm import DGMMKernels
    rt = get_runtime()
    rt.sync_stream()
    return rt, DGMMKernels(rt)


def _up(rt, a, dtype=np.float64):
    return rt.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(rt.device)


def _device_tables(D, K, mu_mom, tau_mom, elog_pi):
    rt, k = _kernels()
    h, q, c, gsum = rt.empty(D, K), rt.empty(D, K), rt.empty(K), rt.empty(K)
    k.tables(D, K, None if mu_mom is None else _up(rt, mu_mom),
             None if tau_mom is None else _up(rt, tau_mom), _up(rt, elog_pi), h, q, c, gsum)
    rt.synchronize()
    return tuple(t.cpu().numpy() for t in (h, q, c, gsum))


def _device_pass(N, D, K, y, h, q, c, labels=None, want_r=False):
    """dict of S1, S2, Nk, sum_lse, Nk_c, S_hq and r (or None) of vmp_dgmm_pass as host arrays."""
    rt, k = _kernels()
    chunk, wsd = k.plan(N, D, K)
    assert chunk == 256
    S1, S2, Nk, scal = rt.empty(D, K), rt.empty(D, K), rt.empty(K), rt.zeros(8)
    ws = rt.empty(int(wsd))
    r = rt.empty(N, K) if want_r and N else None
    lab = None if labels is None else _up(rt, labels, np.int32)
    k.pass_(N, D, K, _up(rt, y) if N else None, lab, _up(rt, h), _up(rt, q), _up(rt, c), ws, S1, S2,
            Nk, scal, r)
    rt.synchronize()
    s = scal.cpu().numpy()
    return dict(S1=S1.cpu().numpy(), S2=S2.cpu().numpy(), Nk=Nk.cpu().numpy(), sum_lse=s[0],
                Nk_c=s[1], S_hq=s[2],
                r=np.zeros((0, K)) if want_r and not N else None if r is None else r.cpu().numpy())


def _device_update(D, K, which, prior_a, prior_b, S1, S2, Nk, other):
    rt, k = _kernels()
    par, mom, bound = rt.empty(D * K, 2), rt.empty(D * K, 2), rt.zeros(1)
    opt = lambda a: None if a is None else _up(rt, a)     # noqa: E731
    k.update(D, K, which, _up(rt, np.broadcast_to(prior_a, (D, K))),
             _up(rt, np.broadcast_to(prior_b, (D, K))), opt(S1), opt(S2), opt(Nk), opt(other), par,
             mom, bound)
    rt.synchronize()
    return par.cpu().numpy(), mom.cpu().numpy(), float(bound.cpu().numpy()[0])


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_pass_against_long_double_restatement(N, D, K):
    from dgmm_host import (make_inputs, host_tables, host_pass, restate_pass, tolerances, error,
                           dgmm_host, PASS_QUANTITIES)
    # 763 rows: three chunks of 256 with a ragged last one
    assert dgmm_host().dgmm_chunks(N, D, K) == (N + 255) // 256
    assert dgmm_host().dgmm_chunks(763, D, K) == 3 and 763 % 256 == 251
    g = make_inputs(N, D, K)
    h, q, c, gsum = _device_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])
    hh, hq, hc, hg = host_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])
    for a, b in ((h, hh), (q, hq), (c, hc), (gsum, hg)):
        np.testing.assert_allclose(a, b, rtol=1e-14, atol=1e-13)
    assert c.max() == 0
    got = _device_pass(N, D, K, g['y'], h, q, c, want_r=True)
    host = host_pass(N, D, K, g['y'], None, h, q, c, want_r=True)
    ld, f64 = restate_pass(g['y'], h, q, c), restate_pass(g['y'], h, q, c, np.float64)
    tol, dev = tolerances(ld, f64, PASS_QUANTITIES)
    for key in PASS_QUANTITIES:
        err, herr = error(got[key], ld[key]), error(host[key], ld[key])
        print('%s (N, D, K) = %s: float64 deviation %.3g, kernel %.3g, host build %.3g, allowed '
              '%.3g' % (key, (N, D, K), dev[key], err, herr, tol[key]))
        assert err <= tol[key], (key, err, tol[key])
        assert herr <= tol[key], ('host', key, herr, tol[key])


@pytest.mark.parametrize('N,D,K', [MID, (763, 257, 64), (257, 64, 16)])
def test_two_calls_and_the_r_output_leave_the_same_bits(N, D, K):
    from dgmm_host import make_inputs, host_tables
    g = make_inputs(N, D, K)
    h, q, c, _ = host_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])
    a = _device_pass(N, D, K, g['y'], h, q, c, want_r=True)
    b = _device_pass(N, D, K, g['y'], h, q, c, want_r=True)
    n = _device_pass(N, D, K, g['y'], h, q, c, want_r=False)
    for key in BITS + ('r',):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    for key in BITS:
        np.testing.assert_array_equal(a[key], n[key], err_msg=key)


@pytest.mark.parametrize('N,D,K', [(763, 70, 17), (300, 257, 5)])
def test_fixed_labels_give_one_hot_rows_and_integer_counts(N, D, K):
    from dgmm_host import make_inputs, host_tables, restate_pass, tolerances, error
    g = make_inputs(N, D, K)
    h, q, c, _ = host_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])
    got = _device_pass(N, D, K, g['y'], h, q, c, labels=g['labels'], want_r=True)
    one = np.eye(K)[g['labels']]
    np.testing.assert_array_equal(got['r'], one)
    np.testing.assert_array_equal(got['Nk'], one.sum(0))
    assert got['sum_lse'] == 0
    # S1 and S2 of one-hot rows: sums of y and y^2 per class, under the rule of the pass
    y = g['y']
    ld = dict(S1=y.astype(np.longdouble).T @ one, S2=(y.astype(np.longdouble) ** 2).T @ one)
    f64 = dict(S1=y.T @ one, S2=(y * y).T @ one)
    tol, _ = tolerances(ld, f64, ('S1', 'S2'))
    for key in ('S1', 'S2'):
        assert error(got[key], ld[key]) <= tol[key], key


@pytest.mark.parametrize('N,D,K', [MID, (300, 70, 17), (65, 1, 5)])
def test_updates_of_both_nodes_against_the_restatement(N, D, K):
    from dgmm_host import (make_inputs, host_tables, host_pass, restate_update, tolerances, error,
                           UPDATE_QUANTITIES)
    g = make_inputs(N, D, K)
    h, q, c, _ = host_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])
    o = host_pass(N, D, K, g['y'], None, h, q, c)
    args = (g['m0'], g['beta0'], g['a0'], g['b0'], o['S1'], o['S2'], o['Nk'], g['mu_mom'],
            g['tau_mom'])
    ld, f64 = restate_update(*args), restate_update(*args, dtype=np.float64)
    keys = UPDATE_QUANTITIES + ('mu_par', 'tau_par')
    tol, dev = tolerances(ld, f64, keys)
    pm, mm, bm = _device_update(D, K, 0, g['m0'], g['beta0'], o['S1'], o['S2'], o['Nk'],
                                g['tau_mom'])
    pt, mt, bt = _device_update(D, K, 1, g['a0'], g['b0'], o['S1'], o['S2'], o['Nk'], g['mu_mom'])
    got = dict(mu_mom=mm, mu_bound=bm, tau_mom=mt, tau_bound=bt, mu_par=pm, tau_par=pt)
    for key in keys:
        err = error(got[key], ld[key])
        print('%s (N, D, K) = %s: float64 deviation %.3g, kernel %.3g, allowed %.3g'
              % (key, (N, D, K), dev[key], err, tol[key]))
        assert err <= tol[key], (key, err, tol[key])


def test_null_tables_and_null_statistics_give_the_priors():
    from dgmm_host import make_inputs
    D, K = 7, 3
    g = make_inputs(10, D, K)
    h, q, c, gsum = _device_tables(D, K, None, None, g['elog_pi'])
    assert not h.any() and not q.any() and not gsum.any()
    np.testing.assert_array_equal(c, g['elog_pi'] - g['elog_pi'].max())
    par, mom, bound = _device_update(D, K, 0, g['m0'], g['beta0'], None, None, None, None)
    np.testing.assert_array_equal(par.reshape(D, K, 2)[..., 0], g['m0'])
    np.testing.assert_array_equal(par.reshape(D, K, 2)[..., 1], g['beta0'])
    assert bound == 0
    par, mom, bound = _device_update(D, K, 1, g['a0'], g['b0'], None, None, None, None)
    np.testing.assert_array_equal(par.reshape(D, K, 2)[..., 0], g['a0'])
    np.testing.assert_array_equal(par.reshape(D, K, 2)[..., 1], g['b0'])
    assert bound == 0


# -- end to end ------------------------------------------------------------------------------------------
def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    return dict(nodes=nodes, VB=VB, vb_kwargs=kw)


def test_fixtures_on_the_fused_block(golden_dir):
    """Fails without the feature: NotImplementedError ('no fused block covers ...') from
    VB(..., engine='fused')."""
    from dgmm_models import run_cases, CASES
    from test_dgmm_host import check_fixture
    from bayespy_amd.inference.plans.dgmm import DiagGaussianMixturePlan
    g = np.load(os.path.join(golden_dir, 'dgmm.npz'))
    gin = {k[3:]: g[k] for k in g.files if k.startswith('in_')}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_cases(_mods(engine='fused'), gin)
    for tag in CASES:
        assert isinstance(res[tag + '_plan'].plans[0], DiagGaussianMixturePlan)
    check_fixture(res, g, CASES)


def test_the_example():
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import diag_gaussian_mixture
    out = diag_gaussian_mixture.run(N=500, D=70, K=4, sweeps=8, verbose=False)
    assert out['plan'] == 'DiagGaussianMixturePlan' and np.all(np.diff(out['L']) > -1e-6)
    assert out['accuracy'] > 0.9


# -- argument checks: nothing is launched ------------------------------------------------------------------
def test_argument_checks_and_limits():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(16)
    p = ctypes.c_void_p(z.data_ptr())
    ok = [p] * 11                               # y, labels, h, q, c, ws, S1, S2, Nk, scal, r_out
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9):
        args = list(ok)
        args[i] = None
        assert lib.vmp_dgmm_pass(ctx, 4, 4, 4, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_dgmm_pass(None, 4, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_dgmm_pass(ctx, -1, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_dgmm_pass(ctx, 4, 0, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_dgmm_pass(ctx, 4, 4, 65, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_dgmm_pass(ctx, 4, 1025, 4, *ok) == _lib.VMP_ERR_UNSUPPORTED
    t = [p] * 7                                 # mu_mom, tau_mom, elog_pi, h, q, c, gsum
    for i in (2, 3, 4, 5):
        args = list(t)
        args[i] = None
        assert lib.vmp_dgmm_tables(ctx, 4, 4, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_dgmm_tables(ctx, 4, 65, *t) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_dgmm_tables(ctx, 1025, 4, *t) == _lib.VMP_ERR_UNSUPPORTED
    u = [p] * 9                                 # prior_a, prior_b, S1, S2, Nk, other, par, mom, bound
    for i in (0, 1, 6, 7, 8):
        args = list(u)
        args[i] = None
        assert lib.vmp_dgmm_update(ctx, 4, 4, 0, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_dgmm_update(ctx, 4, 4, 2, *u) == _lib.VMP_ERR_INVALID
    assert lib.vmp_dgmm_update(ctx, 4, 65, 0, *u) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_dgmm_update(ctx, 1025, 4, 1, *u) == _lib.VMP_ERR_UNSUPPORTED
    k, d = ctypes.c_int32(), ctypes.c_int32()
    assert lib.vmp_dgmm_limits(ctypes.byref(k), ctypes.byref(d)) == _lib.VMP_OK
    assert (k.value, d.value) == (64, 1024)
