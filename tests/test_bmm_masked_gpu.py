"""GPU: the fused Bernoulli-mixture block with missing observations (inference/plans/bmm.py,
csrc/vmp_bmm.hip) -- the masked pass through the C ABI against a long-double restatement at sizes
that cross lane-group, word, column-block, tile and chunk boundaries, bit-identity, a mask of ones
against the unmasked pass, fixed labels, the pack flag, the fixtures and the example through
``VB(..., engine='fused')``, and the argument checks."""
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
SHAPES = sorted(set([(MID[0], MID[1], K) for K in (1, 2, 15, 16, 17, 64)]
                    + [(MID[0], D, MID[2]) for D in (1, 63, 64, 65, 257)]
                    + [(N, MID[1], MID[2]) for N in (0, 1, 63, 65, 257, 763)]
                    + [(763, 257, 64), (300, 1024, 64)]))   # the last: the full LDS tile


def _inputs(N, D, K):
    from bmm_masked_host import mixed_mask
    rs = np.random.RandomState(1000 * K + 10 * D + N)
    x = rs.randint(2, size=(N, D)).astype(np.int64)
    m = mixed_mask(N, D, rs)
    w = rs.normal(size=(D, K))
    l0 = -rs.gamma(1.0, size=(D, K))
    c = rs.normal(size=K)
    return x, m, w, l0, c - c.max()


def _device_pass(N, D, K, x, m, w, l0, c, labels=None, want_r=False):
    """dict of S, M, Nk, counts, sum_lse, Nk_c, S_w, r (or None) and the packed words of
    vmp_bmm_pack_masked + vmp_bmm_pass_masked as host arrays."""
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.bmm import BMMKernels
    rt = get_runtime()
    torch = rt.torch
    k = BMMKernels(rt)
    rt.sync_stream()
    chunk, wsd = k.plan_masked(N, D, K)
    assert chunk == 256
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)    # noqa: E731
    W = (D + 63) // 64
    xw = torch.zeros(max(N, 1) * 2 * W, dtype=torch.int64, device=rt.device)
    flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
    code = {'float64': 0, 'int64': 1}[x.dtype.name]
    k.pack_masked(N, D, code, up(x), up(m.astype(np.uint8)), xw, flag)
    assert int(flag.cpu()[0]) == 0
    S, M, Nk = rt.empty(D, K), rt.empty(D, K), rt.empty(K)
    counts, scal = rt.empty(D * K, 2), rt.zeros(8)
    ws = rt.empty(int(wsd))
    r = rt.empty(N, K) if want_r else None
    lab = None if labels is None else up(labels.astype(np.int32))
    k.pass_masked(N, D, K, xw, lab, up(w), up(l0), up(c), ws, S, M, Nk, counts, scal,
                  r if N else None)
    rt.synchronize()
    s = scal.cpu().numpy()
    return dict(S=S.cpu().numpy(), M=M.cpu().numpy(), Nk=Nk.cpu().numpy(),
                counts=counts.cpu().numpy(), sum_lse=s[0], Nk_c=s[1], S_w=s[2],
                r=None if r is None else r.cpu().numpy(), xw=xw.cpu().numpy())


BITS = ('S', 'M', 'Nk', 'counts', 'sum_lse', 'Nk_c', 'S_w')


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_masked_pass_against_long_double_restatement(N, D, K):
    from bmm_masked_host import (restate_masked, host_pack_masked, host_pass_masked, tolerances,
                                 error, QUANTITIES)
    x, m, w, l0, c = _inputs(N, D, K)
    got = _device_pass(N, D, K, x, m, w, l0, c, want_r=True)
    if not N:
        got['r'] = np.zeros((0, K))
    ld, f64 = restate_masked(x, m, w, l0, c), restate_masked(x, m, w, l0, c, np.float64)
    tol, dev = tolerances(ld, f64)
    hw, _ = host_pack_masked(x, m)
    np.testing.assert_array_equal(hw.reshape(-1).view(np.int64), got['xw'][:hw.size])
    host = host_pass_masked(N, D, K, hw, None, w, l0, c, want_r=True)
    for key in QUANTITIES:
        err, herr = error(got[key], ld[key]), error(host[key], ld[key])
        print('%s (N, D, K) = %s: float64 deviation %.3g, kernel %.3g, host build %.3g, allowed '
              '%.3g' % (key, (N, D, K), dev[key], err, herr, tol[key]))
        assert err <= tol[key], (key, err, tol[key])
        assert herr <= tol[key], ('host', key, herr, tol[key])
    np.testing.assert_array_equal(got['counts'][:, 0], got['S'].reshape(-1))
    np.testing.assert_array_equal(got['counts'][:, 1], (got['M'] - got['S']).reshape(-1))
    if N > 2:
        # the row of nothing: r = softmax(c); a column of nothing: exact zeros
        np.testing.assert_allclose(got['r'][2], np.exp(c) / np.exp(c).sum(), rtol=1e-13)
    if D > 2:
        assert np.all(got['S'][1] == 0) and np.all(got['M'][1] == 0)


@pytest.mark.parametrize('N,D,K', [MID, (763, 257, 64), (257, 64, 16)])
def test_two_calls_the_r_output_and_hidden_entries_leave_the_same_bits(N, D, K):
    x, m, w, l0, c = _inputs(N, D, K)
    a = _device_pass(N, D, K, x, m, w, l0, c, want_r=True)
    b = _device_pass(N, D, K, x, m, w, l0, c, want_r=True)
    n = _device_pass(N, D, K, x, m, w, l0, c, want_r=False)
    flipped = _device_pass(N, D, K, np.where(m, x, 1 - x), m, w, l0, c, want_r=True)
    nan = _device_pass(N, D, K, np.where(m, x, np.nan).astype(np.float64), m, w, l0, c,
                       want_r=True)
    for key in BITS + ('r', 'xw'):
        for other in (b, flipped, nan):
            np.testing.assert_array_equal(a[key], other[key], err_msg=key)
    for key in BITS:
        np.testing.assert_array_equal(a[key], n[key], err_msg=key)


@pytest.mark.parametrize('N,D,K', [MID, (763, 257, 64)])
def test_a_mask_of_ones_matches_the_unmasked_pass(N, D, K):
    """Not bit for bit: c is formed differently (sum_d l0 inside c and the maximum taken out
    there, added through the second plane here, where the logits carry sum_d l0 and are rounded at
    that size).  Each pass is within its own allowance of the common exact value (the rule of
    DESIGN 4.14 on its own restatement), so the two differ by at most the sum of the two.
    Compared one by one: r, N_k and S.  Sum lse, N_k . c and S . w + M . l0 are not: the constants
    stand elsewhere in the two passes (sum_d l0 and the maximum taken out of c), so only their
    combination sum lse - N_k . c - (S . w + M . l0), the entropy, is the same number; it is
    compared at the fixtures' rtol of 1e-9.  With every entry observed M[d, k] is the sum of the
    same r_nk as N_k in another order of additions (tiles, not slots): rtol 1e-12, above
    the worst case 2 (N - 1) 2^-53 = 1.7e-13 of two sums of 763 terms that are not negative."""
    from bmm_host import restate
    from bmm_masked_host import error, restate_masked, tolerances
    from test_bmm_gpu import _device_pass as unmasked_pass, _tolerances
    x, _, w, l0, cpi = _inputs(N, D, K)
    ones = np.ones((N, D), dtype=bool)
    got = _device_pass(N, D, K, x, ones, w, l0, cpi, want_r=True)
    c = cpi + l0.sum(axis=0)
    shift = c.max()
    S, Nk, counts, scal, r, _ = unmasked_pass(N, D, K, x, w, c - shift, want_r=True)
    ld, f64 = restate(x, w, c - shift), restate(x, w, c - shift, np.float64)
    tol, dev = _tolerances(ld, f64)
    tolm, _ = tolerances(restate_masked(x, ones, w, l0, cpi),
                         restate_masked(x, ones, w, l0, cpi, np.float64))
    for key, val, ref in (('r', got['r'], r), ('Nk', got['Nk'], Nk), ('S', got['S'], S)):
        err = error(val, ref)
        print('%s (N, D, K) = %s: masked against unmasked %.3g, allowed %.3g + %.3g'
              % (key, (N, D, K), err, tolm[key], tol[key]))
        assert err <= tolm[key] + tol[key], (key, err)
    np.testing.assert_allclose(got['M'], np.broadcast_to(got['Nk'], (D, K)), rtol=1e-12)
    # the entropy, which does not depend on where the constants stand
    ent_m = got['sum_lse'] - got['Nk_c'] - got['S_w']
    ent_u = scal[0] - scal[1] - scal[2]
    np.testing.assert_allclose(ent_m, ent_u, rtol=1e-9)


def test_fixed_labels_give_exact_integer_counts():
    N, D, K = 763, 70, 17
    x, m, w, l0, c = _inputs(N, D, K)
    lab = np.random.RandomState(5).randint(K, size=N)
    got = _device_pass(N, D, K, x, m, w, l0, c, labels=lab, want_r=True)
    one = np.eye(K)[lab]
    obs = m.any(axis=1)
    assert not obs.all()
    np.testing.assert_array_equal(got['Nk'], (one * obs[:, None]).sum(0))
    np.testing.assert_array_equal(got['S'], (x * m).T @ one)
    np.testing.assert_array_equal(got['M'], m.astype(float).T @ one)
    np.testing.assert_array_equal(got['r'], one)
    assert got['sum_lse'] == 0


def test_pack_dtypes_and_the_flag_on_observed_values_only():
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.bmm import BMMKernels
    from bmm_masked_host import host_pack_masked
    rt = get_runtime()
    torch = rt.torch
    k = BMMKernels(rt)
    rt.sync_stream()
    for D in (63, 64, 65):
        rs = np.random.RandomState(D)
        x = rs.randint(2, size=(37, D))
        m = rs.rand(37, D) < 0.7
        m[5, D - 1], m[6, D - 1] = True, False
        md = torch.from_numpy(m.astype(np.uint8)).to(rt.device)
        want = host_pack_masked(x.astype(np.int64), m)[0].reshape(-1).view(np.int64)
        xw = torch.zeros(want.size, dtype=torch.int64, device=rt.device)
        flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
        for code, a in ((0, x.astype(np.float64)), (1, x.astype(np.int64)), (2, x.astype(bool))):
            xw.zero_()
            k.pack_masked(37, D, code, torch.from_numpy(a).to(rt.device), md, xw, flag)
            np.testing.assert_array_equal(xw.cpu().numpy(), want)
            assert int(flag.cpu()[0]) == 0
        for v in (np.nan, -1.0, 7.0, 0.5):
            hidden = x.astype(np.float64)
            hidden[6, D - 1] = v
            k.pack_masked(37, D, 0, torch.from_numpy(hidden).to(rt.device), md, xw, flag)
            np.testing.assert_array_equal(xw.cpu().numpy(), want)
            assert int(flag.cpu()[0]) == 0
        bad = x.astype(np.float64)
        bad[5, D - 1] = 0.5
        k.pack_masked(37, D, 0, torch.from_numpy(bad).to(rt.device), md, xw, flag)
        assert int(flag.cpu()[0]) == 1


# -- end to end ------------------------------------------------------------------------------------------
def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    return dict(nodes=nodes, VB=VB, vb_kwargs=kw)


def test_fixtures_on_the_fused_block(golden_dir):
    """Fails without the feature: NotImplementedError from VB(..., engine='fused')."""
    from bmm_masked_models import run_masked_cases, CASES
    from test_bmm_masked_host import check_fixture
    from bayespy_amd.inference.plans.bmm import BernoulliMixturePlan
    g = np.load(os.path.join(golden_dir, 'bmm_masked.npz'))
    gin = {k[3:]: g[k] for k in g.files if k.startswith('in_')}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_masked_cases(_mods(engine='fused'), gin)
    for tag in CASES:
        assert isinstance(res[tag + '_plan'].plans[0], BernoulliMixturePlan)
        assert res[tag + '_plan'].plans[0].maskd is not None
    check_fixture(res, g, CASES)
    f = np.load(os.path.join(golden_dir, 'bmm_fused.npz'))
    np.testing.assert_allclose(res['d_L'][:4], f['a_L'], rtol=1e-9)


def test_device_mask_and_the_example(golden_dir):
    import torch
    from bayespy_amd.nodes import Categorical, Dirichlet, Beta, Mixture, Bernoulli
    from bayespy_amd.inference import VB
    g = np.load(os.path.join(golden_dir, 'bmm_masked.npz'))
    x, mask = np.nan_to_num(g['in_c_x']).astype(np.int64), g['in_c_mask']
    N, D = x.shape
    K = 3
    R = Dirichlet(K * [1e-5], name='R')
    Z = Categorical(R, plates=(N, 1), name='Z')
    P = Beta([0.5, 0.5], plates=(D, K), name='P')
    X = Mixture(Z, Bernoulli, P, name='X')
    X.observe(x, mask=torch.from_numpy(mask).to('cuda'))
    P.initialize_from_value(g['in_c_p0'])
    Q = VB(Z, R, X, P, engine='fused')
    Q.ignore_bound_checks = True
    Q.update(repeat=5, verbose=False)
    assert type(Q.plans[0]).__name__ == 'BernoulliMixturePlan'
    np.testing.assert_allclose(Q.L[:5], g['c_L'], rtol=1e-9)
    np.testing.assert_array_equal(Z.mask, g['c_Z_mask'])
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import bernoulli_mixture_missing
    out = bernoulli_mixture_missing.run(N=500, D=40, K=4, sweeps=8, verbose=False)
    assert out['plan'] == 'BernoulliMixturePlan' and np.all(np.diff(out['L']) > -1e-6)
    assert out['held_out_accuracy'] > 0.6


# -- argument checks: nothing is launched ------------------------------------------------------------------
def test_argument_checks():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(16)
    p = ctypes.c_void_p(z.data_ptr())
    ok = [p] * 12                               # every call below has a bad argument
    for i in (0, 2, 3, 4, 5, 6, 7, 8, 9, 10):   # xw, w, l0, c, ws, S, M, Nk, counts, scal
        args = list(ok)
        args[i] = None
        assert lib.vmp_bmm_pass_masked(ctx, 4, 4, 4, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_bmm_pass_masked(None, 4, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_pass_masked(ctx, -1, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_pass_masked(ctx, 4, 4, 65, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_bmm_pass_masked(ctx, 4, 1025, 4, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_bmm_tables_masked(ctx, 4, 4, p, None, p, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_tables_masked(ctx, 4, 4, p, p, p, None, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_tables_masked(ctx, 4, 65, p, p, p, p, p) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_bmm_tables_masked(ctx, 1025, 4, p, p, p, p, p) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_bmm_pack_masked(ctx, 4, 4, 0, p, p, p, None) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_pack_masked(ctx, 4, 4, 0, p, None, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_pack_masked(ctx, 4, 4, 3, p, p, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_pack_masked(ctx, 4, 1025, 0, p, p, p, p) == _lib.VMP_ERR_UNSUPPORTED
