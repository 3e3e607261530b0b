"""GPU: the fused Bernoulli-mixture block (inference/plans/bmm.py, csrc/vmp_bmm.hip) -- the pass
through the C ABI against a long-double restatement at sizes that cross lane-group, word, column
block, tile and chunk boundaries, bit-identity, the host build, golden cases and the bmm.rst
doctest through ``VB(..., engine='fused')``, and the argument checks."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

L_RTOL = 1e-9                               # tests/test_generic_engine_gpu.py on the same data
MOM_TOL = dict(rtol=1e-6, atol=1e-9)

MID = (300, 70, 5)
SHAPES = sorted(set([(MID[0], MID[1], K) for K in (1, 2, 15, 16, 17, 64)]
                    + [(MID[0], D, MID[2]) for D in (1, 63, 64, 65, 257)]
                    + [(N, MID[1], MID[2]) for N in (0, 1, 63, 65, 257, 763)]
                    + [(763, 257, 64)]))     # chunk = 256 at all of these: chunk + 1, 3 chunk - 5


def _inputs(N, D, K):
    rs = np.random.RandomState(1000 * K + 10 * D + N)
    x = rs.randint(2, size=(N, D)).astype(np.int64)
    if N > 2:
        x[0], x[1] = 0, 1
    w = rs.normal(size=(D, K))
    c = rs.normal(size=K) - 0.7 * D
    return x, w, c


def _device_pass(N, D, K, x, w, c, labels=None, want_r=False):
    """(S, Nk, counts, scal[:3], r or None) of vmp_bmm_pack + vmp_bmm_pass as host arrays."""
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.bmm import BMMKernels
    rt = get_runtime()
    torch = rt.torch
    k = BMMKernels(rt)
    rt.sync_stream()
    chunk, wsd = k.plan(N, D, K)
    assert chunk == 256
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)    # noqa: E731
    W = (D + 63) // 64
    xw = torch.zeros(max(N, 1) * W, dtype=torch.int64, device=rt.device)
    flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
    k.pack(N, D, 1, up(x), xw, flag)
    assert int(flag.cpu()[0]) == 0
    S, Nk, counts, scal = rt.empty(D, K), rt.empty(K), rt.empty(D * K, 2), rt.zeros(8)
    ws = rt.empty(int(wsd))
    r = rt.empty(N, K) if want_r else None
    lab = None if labels is None else up(labels.astype(np.int32))
    k.pass_(N, D, K, xw, lab, up(w), up(c), ws, S, Nk, counts, scal, r if N else None)
    rt.synchronize()
    return (S.cpu().numpy(), Nk.cpu().numpy(), counts.cpu().numpy(), scal.cpu().numpy()[:3],
            None if r is None else r.cpu().numpy(), xw.cpu().numpy())


def _tolerances(ld, f64):
    """Per quantity 8 times the largest deviation of the float64 NumPy evaluation (the reference's
    arithmetic) from long double, with a floor of 4 ulp of the quantity's magnitude; the factor
    covers the other order of the additions over D and over the rows."""
    tol, dev = {}, {}
    for key in ('r', 'Nk', 'S', 'sum_lse', 'Nk_c', 'S_w'):
        ref = np.asarray(ld[key], dtype=np.longdouble)
        d = float(np.max(np.abs(np.asarray(f64[key], dtype=np.longdouble) - ref))) if ref.size \
            else 0.0
        mag = float(np.max(np.abs(ref))) if ref.size else 0.0
        dev[key] = d
        tol[key] = max(8 * d, 4 * float(np.spacing(mag)))
    return tol, dev


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_pass_against_long_double_restatement(N, D, K):
    from bmm_host import restate, host_pack, host_pass
    x, w, c = _inputs(N, D, K)
    S, Nk, counts, scal, r, xw = _device_pass(N, D, K, x, w, c, want_r=True)
    ld, f64 = restate(x, w, c), restate(x, w, c, np.float64)
    tol, dev = _tolerances(ld, f64)
    got = dict(r=r if N else np.zeros((0, K)), Nk=Nk, S=S, sum_lse=scal[0], Nk_c=scal[1],
               S_w=scal[2])
    # the host build, within the same tolerance (device exp is not glibc's: no bit-identity)
    hw, _ = host_pack(x)
    np.testing.assert_array_equal(hw.reshape(-1).view(np.int64), xw[:hw.size])
    hS, hNk, _, hsl, hr = host_pass(N, D, K, hw, None, w, c, want_r=True)
    host = dict(r=hr, Nk=hNk, S=hS, sum_lse=hsl, Nk_c=float(np.sum(hNk * c)),
                S_w=float(np.sum(hS * w)))
    for key, val in got.items():
        ref = np.asarray(ld[key], dtype=np.longdouble)
        err = float(np.max(np.abs(np.asarray(val) - ref))) if ref.size else 0.0
        herr = float(np.max(np.abs(np.asarray(host[key]) - ref))) if ref.size else 0.0
        print('%s (N, D, K) = %s: float64 deviation %.3g, kernel %.3g, host build %.3g, allowed '
              '%.3g' % (key, (N, D, K), dev[key], err, herr, tol[key]))
        assert err <= tol[key], (key, err, tol[key])
        assert herr <= tol[key], ('host', key, herr, tol[key])
    np.testing.assert_array_equal(counts[:, 0], S.reshape(-1))
    np.testing.assert_array_equal(counts[:, 1], (Nk[None, :] - S).reshape(-1))


@pytest.mark.parametrize('N,D,K', [MID, (763, 257, 64), (257, 64, 16)])
def test_two_calls_and_the_r_output_leave_the_same_bits(N, D, K):
    x, w, c = _inputs(N, D, K)
    a = _device_pass(N, D, K, x, w, c, want_r=True)
    b = _device_pass(N, D, K, x, w, c, want_r=True)
    n = _device_pass(N, D, K, x, w, c, want_r=False)
    for i in (0, 1, 2, 3, 4):
        np.testing.assert_array_equal(a[i], b[i])
    for i in (0, 1, 2, 3):
        np.testing.assert_array_equal(a[i], n[i])


def test_fixed_labels_give_one_hot_statistics():
    N, D, K = 763, 70, 17
    x, w, c = _inputs(N, D, K)
    lab = np.random.RandomState(5).randint(K, size=N)
    S, Nk, counts, scal, r, _ = _device_pass(N, D, K, x, w, c, labels=lab, want_r=True)
    np.testing.assert_array_equal(Nk, np.bincount(lab, minlength=K))
    np.testing.assert_array_equal(S, x.T @ np.eye(K)[lab])
    np.testing.assert_array_equal(r, np.eye(K)[lab])
    assert scal[0] == 0


def test_pack_dtypes_and_flag():
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.bmm import BMMKernels
    from bmm_host import host_pack
    rt = get_runtime()
    torch = rt.torch
    k = BMMKernels(rt)
    rt.sync_stream()
    for D in (63, 64, 65):
        x = np.random.RandomState(D).randint(2, size=(37, D))
        want = host_pack(x.astype(np.int64))[0].reshape(-1).view(np.int64)
        for code, a in ((0, x.astype(np.float64)), (1, x.astype(np.int64)), (2, x.astype(bool))):
            xw = torch.zeros(want.size, dtype=torch.int64, device=rt.device)
            flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
            k.pack(37, D, code, torch.from_numpy(a).to(rt.device), xw, flag)
            np.testing.assert_array_equal(xw.cpu().numpy(), want)
            assert int(flag.cpu()[0]) == 0
        bad = x.astype(np.float64)
        bad[5, D - 1] = 0.5
        k.pack(37, D, 0, torch.from_numpy(bad).to(rt.device), xw, flag)
        assert int(flag.cpu()[0]) == 1


# -- end to end ------------------------------------------------------------------------------------------
def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    return dict(nodes=nodes, VB=VB, vb_kwargs=kw)


def test_golden_cases_a_and_b_on_the_fused_block(golden_dir):
    from bmm_models import run_bmm_cases
    from bayespy_amd.inference.plans.bmm import BernoulliMixturePlan
    g = np.load(os.path.join(golden_dir, 'bmm_fused.npz'))
    gin = {k[3:]: g[k] for k in g.files if k.startswith('in_')}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_bmm_cases(_mods(engine='fused'), gin, only=('a', 'b'))
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan'):
            assert isinstance(v.plans[0], BernoulliMixturePlan)
            continue
        if k.endswith('_u0'):
            np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL, atol=1e-9)
        checked += 1
    assert checked == 2 * 8


def test_doctest_known_answer_on_the_fused_block(golden_dir):
    """doc/source/examples/bmm.rst: "Iteration 1: loglike=-6.872145e+02 ... Iteration 17:
    loglike=-5.236921e+02" with engine='fused'."""
    from bayespy_amd.nodes import Categorical, Dirichlet, Beta, Mixture, Bernoulli
    from bayespy_amd.inference import VB
    g = np.load(os.path.join(golden_dir, 'bmm_doctest.npz'))
    N, D, K = 100, 10, 10
    R = Dirichlet(K * [1e-5], name='R')
    Z = Categorical(R, plates=(N, 1), name='Z')
    P = Beta([0.5, 0.5], plates=(D, K), name='P')
    X = Mixture(Z, Bernoulli, P)
    Q = VB(Z, R, X, P, engine='fused')
    P.initialize_from_value(g['p_init'])
    X.observe(g['x'])
    Q.update(repeat=1000, verbose=False)
    assert type(Q.plans[0]).__name__ == 'BernoulliMixturePlan'
    L = Q.L[:Q.iter]
    assert '%e' % L[0] == '-6.872145e+02'
    assert Q.iter == 17 and '%e' % L[-1] == '-5.236921e+02'
    np.testing.assert_allclose(L, g['L'], rtol=L_RTOL)
    np.testing.assert_allclose(R.u[0], g['R_u0'], rtol=1e-6)
    np.testing.assert_allclose(P.u[0], g['P_u0'], rtol=1e-6, atol=1e-9)
    assert Z.u[0].shape == (N, 1, K)
    np.testing.assert_allclose(Z.u[0].sum(-1), 1.0, rtol=1e-12)


# -- argument checks: nothing is launched ------------------------------------------------------------------
def test_argument_checks():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(16)
    p = ctypes.c_void_p(z.data_ptr())
    ok = [p] * 10                               # every call below has a bad argument
    for i in (0, 2, 3, 4, 5, 6, 7, 8):          # xw, w, c, ws, S, Nk, counts, scal
        args = list(ok)
        args[i] = None
        assert lib.vmp_bmm_pass(ctx, 4, 4, 4, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_bmm_pass(None, 4, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_pass(ctx, -1, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_pass(ctx, 4, 4, 65, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_bmm_pass(ctx, 4, 1025, 4, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_bmm_tables(ctx, 4, 4, p, None, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_tables(ctx, 4, 65, p, p, p, p) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_bmm_tables(ctx, 1025, 4, p, p, p, p) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_bmm_pack(ctx, 4, 4, 0, p, p, None) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_pack(ctx, 4, 4, 3, p, p, p) == _lib.VMP_ERR_INVALID
    assert lib.vmp_bmm_pack(ctx, 4, 1025, 0, p, p, p) == _lib.VMP_ERR_UNSUPPORTED
