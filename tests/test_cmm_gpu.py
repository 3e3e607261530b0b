"""GPU: the fused categorical-mixture block (inference/plans/cmm.py, csrc/vmp_cmm.hip) -- every
fixture of tests/golden/cmm.npz through ``VB(..., engine='fused')``, each entry point alone through
the C ABI against the long-double restatement of tests/cmm_host.py at sizes that cross lane-group,
column-group, tile and chunk boundaries and the cap of the LDS count table, fixed labels, masks,
bit-identity, the pack flag and the argument checks."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

L_RTOL = 1e-9                               # tests/test_bmm_gpu.py
MOM_TOL = dict(rtol=1e-6, atol=1e-9)

MID = (300, 7, 5, 5)                        # (N, D, K, M)
CAP = (300, 7, 64, 32)                      # the count table exactly at its cap
SHAPES = sorted(set([(MID[0], MID[1], K, MID[3]) for K in (1, 2, 15, 16, 17, 33, 64)]
                    + [(MID[0], MID[1], MID[2], M) for M in (2, 3, 32)]
                    + [(MID[0], D, MID[2], MID[3]) for D in (1, 3, 4, 5, 17)]
                    + [(N, MID[1], MID[2], MID[3]) for N in (0, 1, 63, 64, 65, 257)]
                    + [MID, CAP]))


def _kernels():
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.cmm import CMMKernels
    rt = get_runtime()
    rt.sync_stream()
    return rt, CMMKernels(rt)


def _device_pass(N, D, K, M, x, mask, L, c, labels=None, want_r=False, expect_flag=0):
    """dict of S (M, D, K), Nk, sum_lse, Nk_c, S_L, r (or None) and the packed bytes of
    vmp_cmm_pack + vmp_cmm_pass as host arrays."""
    from cmm_host import DTYPES
    rt, k = _kernels()
    torch = rt.torch
    chunk, wsd = k.plan(N, D, K, M)
    assert chunk == 256
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)    # noqa: E731
    xb = torch.zeros(max(N * D, 8), dtype=torch.uint8, device=rt.device)
    flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
    md = None if mask is None else up(np.asarray(mask).astype(np.uint8))
    k.pack(N, D, M, DTYPES[x.dtype.name], up(x) if N else rt.zeros(1), md, xb, flag)
    assert int(flag.cpu()[0]) == expect_flag
    S, Nk, scal = rt.empty(M, D * K), rt.empty(K), rt.zeros(8)
    ws = rt.empty(int(wsd))
    r = rt.empty(N, K) if want_r and N else None
    lab = None if labels is None else up(labels.astype(np.int32))
    k.pass_(N, D, K, M, xb, lab, up(L), up(c), ws, S, Nk, scal, r)
    rt.synchronize()
    s = scal.cpu().numpy()
    return dict(S=S.cpu().numpy().reshape(M, D, K), Nk=Nk.cpu().numpy(), sum_lse=s[0], Nk_c=s[1],
                S_L=s[2], r=np.zeros((0, K)) if want_r and not N else
                (None if r is None else r.cpu().numpy()), xb=xb.cpu().numpy()[:N * D].reshape(N, D))


BITS = ('S', 'Nk', 'sum_lse', 'Nk_c', 'S_L')


@pytest.mark.parametrize('N,D,K,M', SHAPES)
def test_pass_against_long_double_restatement(N, D, K, M):
    """Per quantity 8 times the deviation of the plain float64 evaluation from long double, floor
    4 ulp of the magnitude; without a mask, with the mask of fixture (f) and with
    fixed labels."""
    from cmm_host import (restate, host_pack, host_pass, tolerances, error, mixed_mask,
                          pass_inputs, QUANTITIES)
    x, L, c, rs = pass_inputs(N, D, K, M)
    for mask in (None, mixed_mask(N, D, rs)):
        got = _device_pass(N, D, K, M, x, mask, L, c, want_r=True)
        ld, f64 = restate(x, mask, L, c), restate(x, mask, L, c, np.float64)
        tol, dev = tolerances(ld, f64)
        hb, _ = host_pack(x, M, mask)
        np.testing.assert_array_equal(hb, got['xb'])
        host = host_pass(N, D, K, M, hb, None, L, c, want_r=True)
        for key in QUANTITIES:
            err, herr = error(got[key], ld[key]), error(host[key], ld[key])
            print('%s (N, D, K, M) = %s mask=%s: float64 deviation %.3g, kernel %.3g, host build '
                  '%.3g, allowed %.3g' % (key, (N, D, K, M), mask is not None, dev[key], err, herr,
                                          tol[key]))
            assert err <= tol[key], (key, err, tol[key])
        if N and K > 1:
            assert got['r'].max() < 0.999                    # soft rows
        if mask is not None and N > 2:
            # the row of nothing: r = softmax(c); a column of nothing: exact zeros
            np.testing.assert_allclose(got['r'][2], np.exp(c) / np.exp(c).sum(), rtol=1e-13)
        if mask is not None and D > 2:
            assert np.all(got['S'][:, 1] == 0)
        # fixed labels: exact integer counts, lse = 0
        lab = rs.randint(K, size=N)
        got = _device_pass(N, D, K, M, x, mask, L, c, labels=lab, want_r=True)
        m = np.ones((N, D), dtype=bool) if mask is None else mask
        one = np.eye(K)[lab]
        np.testing.assert_array_equal(got['r'], one)
        one = one * m.any(axis=1)[:, None]
        np.testing.assert_array_equal(got['Nk'], one.sum(0))
        onehot = ((x[:, :, None] == np.arange(M)) & m[:, :, None]).astype(float)
        np.testing.assert_array_equal(got['S'], np.einsum('ndm,nk->mdk', onehot, one))
        assert got['sum_lse'] == 0


def test_one_step_above_the_cap_is_refused_without_a_launch():
    from bayespy_amd import _lib
    rt, k = _kernels()
    N, D, K, M = CAP
    from bayespy_amd.inference.plans.cmm import cmm_limits
    assert D * M * 64 == cmm_limits()[3]
    c, w = ctypes.c_int64(), ctypes.c_int64()
    assert rt.lib.vmp_cmm_plan(N, D + 1, K, M, ctypes.byref(c), ctypes.byref(w)) \
        == _lib.VMP_ERR_UNSUPPORTED
    z = rt.zeros(16)
    z.fill_(7.0)
    p = ctypes.c_void_p(z.data_ptr())
    assert rt.lib.vmp_cmm_pass(rt.ctx, N, D + 1, K, M, *[p] * 9) == _lib.VMP_ERR_UNSUPPORTED
    assert rt.lib.vmp_cmm_tables(rt.ctx, D + 1, K, M, p, p, p, p) == _lib.VMP_ERR_UNSUPPORTED
    rt.synchronize()
    assert np.all(z.cpu().numpy() == 7.0)                   # nothing was launched


@pytest.mark.parametrize('N,D,K,M', [MID, CAP, (257, 17, 16, 5), (65, 4, 33, 3)])
def test_bit_identity(N, D, K, M):
    """Two calls, with and without r_out, different junk at hidden positions, a mask of ones
    against no mask: the same bits."""
    from cmm_host import mixed_mask, pass_inputs
    x, L, c, rs = pass_inputs(N, D, K, M)
    m = mixed_mask(N, D, rs)
    a = _device_pass(N, D, K, M, x, m, L, c, want_r=True)
    b = _device_pass(N, D, K, M, x, m, L, c, want_r=True)
    n = _device_pass(N, D, K, M, x, m, L, c, want_r=False)
    junk1 = np.where(m, x, np.nan).astype(np.float64)
    junk2 = junk1.copy()
    junk2[~m] = np.resize([-1.0, 1e300, np.nan, 0.5, 3.0], int((~m).sum()))
    j1 = _device_pass(N, D, K, M, junk1, m, L, c, want_r=True)
    j2 = _device_pass(N, D, K, M, junk2, m, L, c, want_r=True)
    for key in BITS + ('r', 'xb'):
        for other in (b, j1, j2):
            np.testing.assert_array_equal(a[key], other[key], err_msg=key)
    for key in BITS:
        np.testing.assert_array_equal(a[key], n[key], err_msg=key)
    u = _device_pass(N, D, K, M, x, None, L, c, want_r=True)
    o = _device_pass(N, D, K, M, x, np.ones((N, D), dtype=bool), L, c, want_r=True)
    for key in BITS + ('r', 'xb'):
        np.testing.assert_array_equal(u[key], o[key], err_msg=key)


def test_pack_dtypes_and_an_out_of_range_value_is_flagged_and_treated_as_hidden():
    """On outputs only: vmp_cmm_pack followed by vmp_cmm_pass on a buffer with a bad observed
    value gives what the same data gives with that entry masked out."""
    from cmm_host import host_pack, pass_inputs, HIDDEN
    N, D, K, M = MID
    x, L, c, rs = pass_inputs(N, D, K, M)
    mask = rs.rand(N, D) < 0.7
    want = host_pack(x, M, mask)[0]
    for a in (x.astype(np.float64), x.astype(np.int64), x.astype(np.int32), x.astype(np.uint8)):
        got = _device_pass(N, D, K, M, a, mask, L, c)
        np.testing.assert_array_equal(got['xb'], want)
    mask[5, 6] = True
    hidden = mask.copy()
    hidden[5, 6] = False
    ref = _device_pass(N, D, K, M, x, hidden, L, c, want_r=True)
    for v in (float(M), -1.0, 0.5, np.nan, 1e300):
        bad = x.astype(np.float64)
        bad[5, 6] = v
        got = _device_pass(N, D, K, M, bad, mask, L, c, want_r=True, expect_flag=1)
        assert got['xb'][5, 6] == HIDDEN
        for key in BITS + ('r', 'xb'):
            np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
    for v in (M, -1, 2 ** 40):
        bad = x.copy()
        bad[5, 6] = v
        got = _device_pass(N, D, K, M, bad, mask, L, c, want_r=True, expect_flag=1)
        for key in BITS + ('r', 'xb'):
            np.testing.assert_array_equal(got[key], ref[key], err_msg=key)


def test_tables():
    from cmm_host import restate_tables, pass_inputs
    rt, k = _kernels()
    N, D, K, M = MID
    _, L, _, rs = pass_inputs(N, D, K, M)
    elog_pi = rs.normal(size=K) - 1e5
    up = lambda a: rt.torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)    # noqa: E731
    for ep in (None, L):
        Ld, cd = rt.empty(M, D * K), rt.empty(K)
        k.tables(D, K, M, None if ep is None else up(ep), up(elog_pi), Ld, cd)
        Lr, cr = restate_tables(ep, elog_pi, (M, D * K))
        np.testing.assert_array_equal(Ld.cpu().numpy(), Lr)
        np.testing.assert_array_equal(cd.cpu().numpy(), cr)


# -- end to end ------------------------------------------------------------------------------------------
def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    return dict(nodes=nodes, VB=VB, vb_kwargs=kw)


def test_fixtures_on_the_fused_block():
    """Fails without the feature: NotImplementedError from VB(..., engine='fused')."""
    from cmm_models import run_cmm_cases, CASES
    from test_cmm_host import check_fixture, _golden
    from bayespy_amd.inference.plans.cmm import CategoricalMixturePlan
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_cmm_cases(_mods(engine='fused'), gin)
    for tag in CASES:
        assert isinstance(res[tag + '_plan'].plans[0], CategoricalMixturePlan)
    assert check_fixture(res, g, CASES) == len(CASES) * (1 + 4 + 3 + 2)
    for k in ('L', 'Z_u0', 'P_u0', 'R_u0'):
        np.testing.assert_array_equal(res['g_' + k], res['a_' + k], err_msg=k)


def test_the_pass_entry_point_is_exported():
    """Fails without the feature: the library has no such symbol."""
    from bayespy_amd import _lib
    assert hasattr(_lib.load(), 'vmp_cmm_pass')


def test_invalid_category_on_a_device_tensor_device_mask_and_the_example():
    import torch
    from cmm_models import build_cmm
    from test_cmm_host import _golden
    from bayespy_amd.inference import VB
    g, gin = _golden()
    x, mask, p0 = gin['a_x'], gin['f_mask'], gin['a_p0']
    m = build_cmm(_mods(), x, 3, 5, conc=gin['a_conc'], alpha=gin['a_alpha'], observe=False)
    m['X'].observe(np.where(mask, x, 0), mask=torch.from_numpy(mask).to('cuda'))
    m['P'].initialize_from_value(p0)
    Q = VB(m['Z'], m['R'], m['X'], m['P'], engine='fused')
    Q.ignore_bound_checks = True
    Q.update(repeat=4, verbose=False)
    assert type(Q.plans[0]).__name__ == 'CategoricalMixturePlan'
    np.testing.assert_allclose(Q.L[:4], g['f_L'], rtol=L_RTOL)
    np.testing.assert_array_equal(m['Z'].mask, g['f_Z_mask'])
    np.testing.assert_array_equal(m['P'].mask, g['f_P_mask'])
    bad = torch.from_numpy(np.where(mask, x, 0)).to('cuda')
    bad[5, 0] = 5
    assert mask[5, 0]
    m['X']._data = bad
    Q.plans[0].invalidate(m['X'])
    with pytest.raises(ValueError, match='Invalid category index'):
        Q.update(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import categorical_mixture
    for missing in (False, True):
        out = categorical_mixture.run(N=500, D=12, K=3, M=4, sweeps=8, missing=missing,
                                      verbose=False)
        assert out['plan'] == 'CategoricalMixturePlan' and np.all(np.diff(out['L']) > -1e-6)
        assert out['accuracy'] > 0.6


# -- argument checks: nothing is launched ------------------------------------------------------------------
def test_argument_checks():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(16)
    p = ctypes.c_void_p(z.data_ptr())
    ok = [p] * 9                                # xb, labels, L, c, ws, S, Nk, scal, r_out
    for i in (0, 2, 3, 4, 5, 6, 7):
        args = list(ok)
        args[i] = None
        assert lib.vmp_cmm_pass(ctx, 4, 4, 4, 4, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_cmm_pass(None, 4, 4, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_cmm_pass(ctx, -1, 4, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_cmm_pass(ctx, 4, 4, 65, 4, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_cmm_pass(ctx, 4, 4, 4, 33, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_cmm_pass(ctx, 4, 4, 4, 1, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_cmm_tables(ctx, 4, 4, 4, p, None, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_cmm_tables(ctx, 4, 4, 4, p, p, None, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_cmm_tables(ctx, 4, 65, 4, p, p, p, p) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_cmm_pack(ctx, 4, 4, 4, 0, p, p, p, None) == _lib.VMP_ERR_INVALID
    assert lib.vmp_cmm_pack(ctx, 4, 4, 4, 0, None, p, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_cmm_pack(ctx, 4, 4, 4, 4, p, p, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_cmm_pack(ctx, 4, 4, 33, 0, p, p, p, p) == _lib.VMP_ERR_UNSUPPORTED
