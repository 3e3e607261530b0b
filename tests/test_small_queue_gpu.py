"""
The queue of small operations at its limits (include/vmp_hip.h: vmp_queue_*; csrc/vmp_generic.hip:
small_ops_kernel, queue_place).  Inside a plan operation small formulas, small plate sums and small
SPD inverses are records that one interpreter launch runs later; outside an operation (or with the
queue's tune off) the same calls launch stand-alone kernels.  Every case runs the ways its kind
allows and asserts WHICH path it took from the queue statistics (``operations`` grows only for
records), so that a moved threshold cannot turn a queue test into a stand-alone test unnoticed.

References are computed on the host in extended precision (np.longdouble; scipy for the special
functions, whose fp64 accuracy the library documents as 2e-14, tests/test_cabi.py).  Tolerances
follow from error bounds, with u = 2^-53 the unit round-off of fp64:

* sums:      |err| <= (h + nin) u sum|terms|, h the height of the kernel's addition tree (its
             longest chain of additions); h = nred for a chain, so this holds for any order
* inverses:  ||X - A^-1||_F / ||A^-1||_F <= 8 n kappa u   (Gauss-Jordan on an SPD matrix without
             pivoting: backward stable, forward error <= c n kappa u)
* logdet:    |err| <= 4 n u (n kappa + sum|log lambda_i|)   (every pivot to n kappa u relative; the
             logarithms of up to n partial products summed one after the other)
* formulas:  relative error <= 4 nops u for the elementary words on data without cancellation

At kappa = 1 every one of them is below 1e-12 relative.
"""
import ctypes

import numpy as np
import pytest
from scipy import special

pytestmark = pytest.mark.gpu

U64 = 2.0 ** -53
SMALL_SM_KEEP, SMALL_SM_WORK, SMALL_EW_MAX = 2048, 32768, 2048


# ---- runtime helpers -------------------------------------------------------------------------------
def _rt():
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    with rt.operation():         # the first operation sets the queue's tunes from the environment
        pass
    if not rt._tune_sm:
        pytest.skip('sums and inverses are kept out of the queue (BAYESPY_AMD_SMALL_QUEUE=ew)')
    return rt


def _ops(rt):
    """Records run so far (after flushing what is collected)."""
    rt.flush_small()
    return rt.queue_stats()['operations']


class _Tune:
    """Set a tune key for a block; the runtime's own value is restored after."""

    def __init__(self, rt, key, value, restore):
        self.rt, self.key, self.value, self.restore = rt, key, value, restore

    def __enter__(self):
        self.rt.flush_small()
        self.rt.set_tune(self.key, self.value)

    def __exit__(self, *exc):
        self.rt.flush_small()
        self.rt.set_tune(self.key, self.restore)
        return False


def _dev(rt, a):
    from bayespy_amd.darray import DArray
    return DArray(rt.to_device(a))


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


# ---- SPD references ------------------------------------------------------------------------------
def _spd(n, kappa, scale, rng, base=1.7):
    """Q diag(lambda) Q^T with lambda log-spaced over [base, base * kappa] times scale, exactly
    symmetric in fp64; returns the matrix and its lambdas."""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = base * scale * (kappa ** (np.arange(n) / max(n - 1, 1)))
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T), lam


def _swing(n, rng):
    """D S D with S a well-conditioned correlation matrix and D^2 log-spaced from 1e-150 to
    1e150: the pivots swing over 300 decades (the prod / ld split of logdet_accumulate)."""
    S, _ = _spd(n, 4.0, 1.0, rng, base=1.0)
    d = np.sqrt(S.diagonal())
    S = S / np.outer(d, d)
    D = 10.0 ** np.linspace(-75, 75, n)
    A = S * np.outer(D, D)
    return 0.5 * (A + A.T), D, S


def _gj_ref(A):
    """Inverse and log-determinant of a symmetric matrix by Gauss-Jordan sweeps in long double;
    (None, None) when a pivot is not positive."""
    M = np.array(A, dtype=np.longdouble)
    n = M.shape[0]
    ld = np.longdouble(0)
    for p in range(n):
        piv = M[p, p]
        if not piv > 0:
            return None, None
        ld += np.log(piv)
        d = 1 / piv
        ci, rj = M[:, p].copy(), M[p, :].copy()
        M -= np.outer(ci, rj) * d
        M[p, :] = rj * d
        M[:, p] = -ci * d
        M[p, p] = d
    return M, ld


def _check_inverse(X, ld, A, lam, tag):
    R, Rld = _gj_ref(A)
    assert R is not None
    n = A.shape[0]
    kappa = lam.max() / lam.min()
    err = np.sqrt(np.sum((np.asarray(X, np.longdouble) - R) ** 2)) / np.sqrt(np.sum(R ** 2))
    assert err <= 8 * n * kappa * U64, '%s: inverse rel. err %.3g' % (tag, float(err))
    tol = 4 * n * U64 * (n * kappa + np.sum(np.abs(np.log(lam))))
    assert abs(np.longdouble(ld) - Rld) <= tol, '%s: logdet err %.3g > %.3g' % (
        tag, float(abs(np.longdouble(ld) - Rld)), tol)


def _queues_spd(n, batch):
    return 8 < n <= 32 and batch <= 4


def _chol_paths(rt, A):
    """Inverse and logdet of the batch A through linalg.chol: stand-alone, queued, queue switched
    off; each with the number of records it added."""
    from bayespy_amd.utils import linalg
    out = {}
    C = _dev(rt, A)
    o0 = _ops(rt)
    U = linalg.chol(C)
    out['alone'] = (linalg.chol_inv(U).numpy(), linalg.chol_logdet(U).numpy(), _ops(rt) - o0)
    o0 = _ops(rt)
    with rt.operation():
        U = linalg.chol(C)
        X, L = linalg.chol_inv(U), linalg.chol_logdet(U)
    out['queued'] = (X.numpy(), L.numpy(), _ops(rt) - o0)
    with _Tune(rt, 'small_queue_spd', 0, 1):
        o0 = _ops(rt)
        with rt.operation():
            U = linalg.chol(C)
            X, L = linalg.chol_inv(U), linalg.chol_logdet(U)
        out['off'] = (X.numpy(), L.numpy(), _ops(rt) - o0)
    return out


SPD_N = [1, 2, 7, 8, 9, 12, 16, 17, 23, 24, 31, 32, 33, 48, 64]


@pytest.mark.parametrize('kappa', [1.0, 1e4, 1e8])
@pytest.mark.parametrize('batch', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('n', SPD_N)
def test_spd_queued_standalone_and_reference(n, batch, kappa):
    """linalg.chol / chol_inv / chol_logdet at the queue's edges (8 < n <= 32, batch <= 4): the
    path taken, the long-double reference, and queued == stand-alone bit for bit (queued records
    run spd_block_body<QNT>, the stand-alone block kernel spd_block_body<NT>; n <= 8 and n > 32
    take the same stand-alone kernel on every path)."""
    rt = _rt()
    rng = np.random.default_rng(1000 * n + 10 * batch + int(np.log10(kappa)))
    mats = [_spd(n, kappa, 1.0, rng) for _ in range(batch)]
    A = np.stack([m for m, _ in mats])
    res = _chol_paths(rt, A)
    assert res['alone'][2] == 0 and res['off'][2] == 0
    assert res['queued'][2] == (1 if _queues_spd(n, batch) else 0)
    for b, (Ab, lam) in enumerate(mats):
        _check_inverse(res['queued'][0][b], res['queued'][1][b], Ab, lam, 'n=%d b=%d' % (n, b))
    for path in ('alone', 'off'):
        assert np.array_equal(res[path][0].view(np.int64), res['queued'][0].view(np.int64)), path
        assert np.array_equal(res[path][1].view(np.int64), res['queued'][1].view(np.int64)), path


@pytest.mark.parametrize('scale', [1e-150, 1e-30, 1e30, 1e150])
@pytest.mark.parametrize('n', [7, 12, 32, 48])
def test_spd_extreme_scales(n, scale):
    """Matrices of magnitude 1e-150 .. 1e150 (kappa = 10: the elimination forms c_i r_j before the
    division by the pivot, so entries beyond ~1e154 would overflow an intermediate)."""
    rt = _rt()
    rng = np.random.default_rng(n)
    mats = [_spd(n, 10.0, scale, rng) for _ in range(4)]
    A = np.stack([m for m, _ in mats])
    res = _chol_paths(rt, A)
    assert res['queued'][2] == (1 if _queues_spd(n, 4) else 0)
    for b, (Ab, lam) in enumerate(mats):
        X = res['queued'][0][b]
        assert np.all(np.isfinite(X))
        _check_inverse(X, res['queued'][1][b], Ab, lam, 'n=%d scale=%g' % (n, scale))
    assert np.array_equal(res['alone'][0].view(np.int64), res['queued'][0].view(np.int64))
    assert np.array_equal(res['alone'][1].view(np.int64), res['queued'][1].view(np.int64))


@pytest.mark.parametrize('n', [12, 16, 32, 64])
def test_spd_pivots_swinging_over_300_decades(n):
    """D S D, D^2 from 1e-150 to 1e150: scale invariance of the elimination bounds the error of
    D A^-1 D by that of S^-1; the logdet must survive the running product leaving its range."""
    rt = _rt()
    rng = np.random.default_rng(77 + n)
    A, D, S = _swing(n, rng)
    res = _chol_paths(rt, A[None])
    assert res['queued'][2] == (1 if _queues_spd(n, 1) else 0)
    R, Rld = _gj_ref(A)
    X = res['queued'][0][0]
    assert np.all(np.isfinite(X))
    lamS = np.linalg.eigvalsh(S)
    kappa = lamS.max() / lamS.min()
    Dl = np.asarray(D, np.longdouble)
    E = Dl[:, None] * (np.asarray(X, np.longdouble) - R) * Dl[None, :]
    Rs = Dl[:, None] * R * Dl[None, :]
    assert np.sqrt(np.sum(E ** 2)) / np.sqrt(np.sum(Rs ** 2)) <= 8 * n * kappa * U64
    # sum |log lambda| of A is at most sum |log d_i^2| + sum |log lambda(S)|
    tol = 4 * n * U64 * (n * kappa + np.sum(np.abs(np.log(D ** 2))) + np.sum(np.abs(np.log(lamS))))
    assert abs(np.longdouble(res['queued'][1][0]) - Rld) <= tol
    assert np.array_equal(res['alone'][0].view(np.int64), res['queued'][0].view(np.int64))
    assert np.array_equal(res['alone'][1].view(np.int64), res['queued'][1].view(np.int64))


def _bad_batch(n, which, rng):
    """A batch of four with matrix 2 not positive definite: 'first' (negative first pivot),
    'last' (L diag(1, .., 1, -1/2) L^T: only the last pivot is negative) or 'nan'."""
    mats = [_spd(n, 1e2, 1.0, rng) for _ in range(4)]
    A = np.stack([m for m, _ in mats])
    if which == 'first':
        A[2, 0, 0] = -1.0
    elif which == 'last':
        L = np.tril(rng.standard_normal((n, n)) * 0.3, -1) + np.eye(n)
        d = np.ones(n)
        d[-1] = -0.5
        B = (L * d) @ L.T
        A[2] = 0.5 * (B + B.T)
    else:
        A[2, 3, 5] = A[2, 5, 3] = np.nan
    return A, [lam for _, lam in mats]


@pytest.mark.parametrize('which', ['first', 'last', 'nan'])
@pytest.mark.parametrize('n', [12, 32])
def test_spd_indefinite_member_of_a_queued_batch(n, which):
    """Raw vmp_spd_batched, queued: info is set for the bad matrix only and the other three are
    right; through linalg the operation ends with NotPositiveDefiniteError."""
    import torch
    from bayespy_amd import _lib
    from bayespy_amd.utils import linalg
    rt = _rt()
    rng = np.random.default_rng(5 * n + len(which))
    A, lams = _bad_batch(n, which, rng)
    if which == 'last':
        R, _ = _gj_ref(A[2])
        assert R is None
    At = torch.from_numpy(A).to(rt.device)
    X = torch.full_like(At, -3.0)
    L = torch.full((4,), -3.0, dtype=torch.float64, device=rt.device)
    info = torch.full((4,), -7, dtype=torch.int32, device=rt.device)
    o0 = _ops(rt)
    with rt.operation():
        rt.check(rt.lib.vmp_spd_batched(rt.ctx, n, 4, _vp(At), _vp(X), _vp(L), _vp(info)))
    assert _ops(rt) - o0 == 1
    rt.synchronize()
    assert info.cpu().numpy().tolist() == [0, 0, 1, 0]
    Xh, Lh = X.cpu().numpy(), L.cpu().numpy()
    for b in (0, 1, 3):
        _check_inverse(Xh[b], Lh[b], A[b], lams[b], 'b=%d' % b)
    C = _dev(rt, A)
    with pytest.raises(_lib.NotPositiveDefiniteError):
        with rt.operation():
            U = linalg.chol(C)
            linalg.chol_inv(U)
    # the stand-alone kernel flags the same matrix
    info.fill_(-7)
    rt.check(rt.lib.vmp_spd_batched(rt.ctx, n, 4, _vp(At), _vp(X), _vp(L), _vp(info)))
    rt.synchronize()
    assert info.cpu().numpy().tolist() == [0, 0, 1, 0]


# ---- queued sums -------------------------------------------------------------------------------------
def _sum_ref(arrays, axis, scale):
    """Long-double sum of the products and the sum of their magnitudes."""
    prod = np.longdouble(scale)
    for a in arrays:
        prod = prod * np.asarray(a, np.longdouble)
    return np.sum(prod, axis=axis), np.sum(np.abs(prod), axis=axis)


def _chain(nkeep, nred, queued):
    """Height of the addition tree of one output (see the module docstring): the interpreter's
    (small_sum_body: a lane adds every G-th product, 8 per round, then log2(G) shuffle levels, or
    a workgroup of 512 lanes and its 8 wavefront sums); any other order is bounded by nred."""
    if not queued or nred <= 1:
        return max(nred, 1)
    if nkeep * 64 < 512 and nred > 1024:
        return -(-nred // 512) + 6 + 8
    G = 1
    while G < 64 and 2 * G * nkeep <= 512 and 2 * G <= nred:
        G *= 2
    return -(-nred // G) + int(np.log2(G))


def _check_sum(got, arrays, axis, scale, nkeep, nred, queued, tag):
    ref, mag = _sum_ref(arrays, axis, scale)
    ref, mag = np.broadcast_to(ref, got.shape), np.broadcast_to(mag, got.shape)
    h = _chain(nkeep, nred, queued) + len(arrays)
    err = np.abs(np.asarray(got, np.longdouble) - ref)
    bound = h * U64 * mag
    assert np.all(err <= bound), '%s: worst err/bound %.3g' % (tag, float(np.max(err / np.maximum(bound, 1e-300))))


def _cancelling(shape, rng):
    """Products that cancel: every value comes with its negative times (1 + small)."""
    x = rng.uniform(1.0, 2.0, size=shape) * 1e3
    sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return x * sign * (1.0 + 1e-6 * rng.standard_normal(shape))


def _sum_paths(rt, fn, queued_expected, tune=None):
    """fn() -> DArray, run stand-alone, queued and with the queue's tunes off; the results and the
    records added by each."""
    out = {}
    o0 = _ops(rt)
    r = fn()
    out['alone'] = (r.numpy(), _ops(rt) - o0)
    o0 = _ops(rt)
    with rt.operation():
        r = fn()
    out['queued'] = (r.numpy(), _ops(rt) - o0)
    # (formulas off too: without the queue a sum of three operands may form a product first)
    with _Tune(rt, 'small_queue_sm', 0, 1), _Tune(rt, 'small_queue_ew', 0, 1):
        o0 = _ops(rt)
        with rt.operation():
            r = fn()
        out['off'] = (r.numpy(), _ops(rt) - o0)
    assert out['alone'][1] == 0 and out['off'][1] == 0
    assert out['queued'][1] == (1 if queued_expected else 0)
    return out


SUM_SHAPES = [
    # (nkeep, nred): output counts around SMALL_SM_KEEP, product counts around SMALL_SM_WORK
    (1, 1), (1, 7), (2047, 16), (2048, 16), (2049, 16), (2048, 1),
    (1, 32768), (1, 32769), (8, 4096), (8, 4097), (3, 10922), (3, 10923), (64, 512), (2, 1025),
]


@pytest.mark.parametrize('cancel', [False, True])
@pytest.mark.parametrize('nkeep,nred', SUM_SHAPES)
def test_sum_limits_two_operands(nkeep, nred, cancel):
    """sum_j A[k, j] x[j] * s at the limits: queued exactly when nkeep <= 2048 and
    nkeep * nred <= 32768; every path within the bound of its addition tree."""
    from bayespy_amd.utils import misc
    rt = _rt()
    rng = np.random.default_rng(nkeep * 7 + nred)
    A = _cancelling((nkeep, nred), rng) if cancel else rng.uniform(0.5, 1.5, (nkeep, nred))
    x = rng.uniform(0.5, 1.5, nred)
    Ad, xd = _dev(rt, A), _dev(rt, x)
    q = nkeep <= SMALL_SM_KEEP and nkeep * nred <= SMALL_SM_WORK
    res = _sum_paths(rt, lambda: misc.sum_multiply(Ad, xd, 0.37, axis=-1), q)
    for path, (got, _) in res.items():
        _check_sum(got, [A, x], -1, 0.37, nkeep, nred, path == 'queued' and q, path)


def test_sum_work_limit_follows_the_tune():
    """small_queue_sm_work lowered to 1024: 4 x 256 products are a record, 4 x 257 are not."""
    from bayespy_amd.utils import misc
    rt = _rt()
    rng = np.random.default_rng(3)
    with _Tune(rt, 'small_queue_sm_work', 1024, SMALL_SM_WORK):
        for nred, q in ((256, True), (257, False)):
            A, x = rng.standard_normal((4, nred)), rng.standard_normal(nred)
            Ad, xd = _dev(rt, A), _dev(rt, x)
            res = _sum_paths(rt, lambda: misc.sum_multiply(Ad, xd, axis=-1), q)
            for path, (got, _) in res.items():
                _check_sum(got, [A, x], -1, 1.0, 4, nred, path == 'queued' and q, path)


SUM_FORMS = {
    # name: (operand shapes, axis to sum, nkeep, nred)
    'one operand': ([(16, 128)], (1,), 16, 128),
    # (every operand varies along a summed axis: none is hoisted out of the sum as a formula)
    'three operands': ([(16, 128), (1, 128), (16, 128)], (1,), 16, 128),
    'broadcast stride 0': ([(32, 1), (32, 64)], (0,), 64, 32),
    'non-adjacent axes': ([(6, 5, 7, 3)], (0, 2), 15, 42),
    'non-adjacent, three operands': ([(6, 5, 7, 3), (6, 1, 7, 1), (6, 5, 7, 1)], (0, 2), 15, 42),
    'all axes': ([(40, 50), (40, 50)], (0, 1), 1, 2000),
}


@pytest.mark.parametrize('name', sorted(SUM_FORMS))
def test_sum_operand_forms(name):
    from bayespy_amd.utils import misc
    rt = _rt()
    shapes, axis, nkeep, nred = SUM_FORMS[name]
    rng = np.random.default_rng(len(name))
    arrs = [_cancelling(s, rng) for s in shapes]
    devs = [_dev(rt, a) for a in arrs]
    res = _sum_paths(rt, lambda: misc.sum_multiply(*devs, -1.25, axis=axis), True)
    ref_shape = np.sum(np.broadcast_arrays(*arrs)[0], axis=axis).shape
    for path, (got, _) in res.items():
        assert got.shape == ref_shape
        _check_sum(got, arrs, axis, -1.25, nkeep, nred, path == 'queued', path)


def test_sum_over_an_empty_axis_is_zero():
    """A reduced axis of extent 0: every output 0 on every path (raw vmp_sum_multiply: the
    Python wrapper never hands an empty reduction to the library)."""
    import torch
    from bayespy_amd.utils.misc import _workspace
    rt = _rt()
    K = 5
    a = torch.ones(1, dtype=torch.float64, device=rt.device)
    ws = _workspace(rt)

    def run():
        out = torch.full((K,), 9.0, dtype=torch.float64, device=rt.device)
        shape = (ctypes.c_int64 * 2)(0, K)
        ins = (ctypes.c_void_p * 1)(a.data_ptr())
        st = (ctypes.c_int64 * 2)(0, 0)
        ost = (ctypes.c_int64 * 2)(0, 1)
        rt.check(rt.lib.vmp_sum_multiply(rt.ctx, 2, shape, 1, ins, st, ost, ctypes.c_uint32(1), 2.0,
                                         _vp(out), _vp(ws), ws.numel() * 8))
        return out

    o0 = _ops(rt)
    with rt.operation():
        out = run()
    assert _ops(rt) - o0 == 1
    assert out.cpu().numpy().tolist() == [0.0] * K
    o0 = _ops(rt)
    out = run()
    rt.synchronize()
    assert _ops(rt) - o0 == 0
    assert out.cpu().numpy().tolist() == [0.0] * K


# ---- queued formulas -------------------------------------------------------------------------------
def _factor(size, ndim):
    """size as ndim extents >= 2 (None when impossible)."""
    if ndim == 1:
        return (size,)
    for f in range(2, int(np.sqrt(size)) + 1):
        if size % f == 0:
            rest = _factor(size // f, ndim - 1)
            if rest is not None:
                return (f,) + rest
    return None


def _formula_operands(shape, rng):
    """x dense, y broadcast on every second axis: no two axes of the formula merge, so the
    kernels see all len(shape) of them."""
    x = rng.uniform(0.5, 2.0, shape)
    yshape = tuple(1 if d % 2 else s for d, s in enumerate(shape))
    y = rng.uniform(0.5, 2.0, yshape)
    return x, y


def _ew_paths(rt, fn, queued_expected):
    out = {}
    o0 = _ops(rt)
    r = fn()
    out['alone'] = (r.numpy(), _ops(rt) - o0)
    o0 = _ops(rt)
    with rt.operation():
        r = fn()
    out['queued'] = (r.numpy(), _ops(rt) - o0)
    with _Tune(rt, 'small_queue_ew', 0, 1):
        o0 = _ops(rt)
        with rt.operation():
            r = fn()
        out['off'] = (r.numpy(), _ops(rt) - o0)
    assert out['alone'][1] == 0 and out['off'][1] == 0
    assert out['queued'][1] == (1 if queued_expected else 0)
    return out


EW_CASES = [(s, nd, m) for s, m in [(1, None), (2047, None), (2048, None), (2049, None),
                                     (2048, 8192), (8192, 8192), (8193, 8192)]
            for nd in range(1, 6) if _factor(s, nd) is not None]


@pytest.mark.parametrize('size,ndim,ew_max', EW_CASES)
def test_formula_limits_and_dims(size, ndim, ew_max):
    """(x + y) * c + x / y at sizes around small_queue_ew_max (2048, and 8192 set through the
    tune), ndim 1 .. 5 (at 5 the stand-alone side is the generic ewise_kernel): queued ==
    stand-alone bit for bit, both within 4 nops u of the reference."""
    from bayespy_amd.darray import fuse
    rt = _rt()
    shape = _factor(size, ndim)
    rng = np.random.default_rng(size + ndim)
    x, y = _formula_operands(shape, rng)
    xd, yd = _dev(rt, x), _dev(rt, y)
    limit = ew_max or SMALL_EW_MAX

    def run():
        return fuse(lambda a, b: (a + b) * 1.5 + a / b, xd, yd)

    if ew_max is None:
        res = _ew_paths(rt, run, size <= limit)
    else:
        restore = rt._queue_max_out
        with _Tune(rt, 'small_queue_ew_max', ew_max, restore):
            res = _ew_paths(rt, run, size <= limit)
    xl, yl = np.asarray(x, np.longdouble), np.asarray(y, np.longdouble)
    ref = (xl + yl) * np.longdouble(1.5) + xl / yl
    got = res['queued'][0]
    assert got.shape == shape
    assert np.all(np.abs(got - ref) <= 4 * 9 * U64 * ref)        # 9 words, positive terms
    for path in ('alone', 'off'):
        assert np.array_equal(res[path][0].view(np.int64), got.view(np.int64)), path


def _program(*words):
    return list(words)


def _raw_ewise(rt, shape, ins, ops, consts, out):
    nd = len(shape)
    c_shape = (ctypes.c_int64 * max(nd, 1))(*shape)
    c_in = (ctypes.c_void_p * len(ins))(*[t.data_ptr() for t in ins])
    flat = []
    for t in ins:
        flat += [0 if t.shape[d] == 1 else t.stride(d) for d in range(nd)]
    c_str = (ctypes.c_int64 * len(flat))(*flat)
    c_ops = (ctypes.c_int32 * len(ops))(*ops)
    c_consts = (ctypes.c_double * max(len(consts), 1))(*consts)
    rt.check(rt.lib.vmp_ewise(rt.ctx, nd, c_shape, len(ins), c_in, c_str, len(ops), c_ops,
                              len(consts), c_consts, _vp(out)))


def _opcode_programs():
    from bayespy_amd import darray as D

    def w(op, arg=0):
        return op | (arg << 8)
    L = np.longdouble
    return {
        # name: (ops, consts, operand ranges, long-double / scipy reference, rel. tolerance)
        'arith': ([w(D.OP_IN, 0), w(D.OP_IN, 1), D.OP_ADD, w(D.OP_CONST, 0), D.OP_MUL, w(D.OP_IN, 0),
                   w(D.OP_IN, 1), D.OP_DIV, D.OP_ADD], [3.0], [(0.5, 2), (0.5, 2)],
                  lambda x, y: (L(x) + L(y)) * 3 + L(x) / L(y), 4 * 9 * U64),
        'unary': ([w(D.OP_IN, 0), D.OP_SQRT, w(D.OP_IN, 1), D.OP_NEG, D.OP_EXP, D.OP_MUL, w(D.OP_IN, 0),
                   D.OP_LOG, D.OP_SQR, D.OP_ADD, D.OP_RECIP], [], [(1.5, 4), (0.1, 3)],
                  lambda x, y: 1 / (np.sqrt(L(x)) * np.exp(-L(y)) + np.log(L(x)) ** 2), 4 * 11 * U64),
        'dup swap': ([w(D.OP_IN, 0), D.OP_DUP, D.OP_MUL, w(D.OP_IN, 1), D.OP_SWAP, D.OP_SUB], [],
                     [(0.5, 1), (2, 3)], lambda x, y: L(y) - L(x) * L(x), 4 * 6 * U64),
        'max min where': ([w(D.OP_IN, 0), w(D.OP_IN, 1), D.OP_MAX, w(D.OP_IN, 2), w(D.OP_IN, 3),
                           D.OP_WHERE_NZ, w(D.OP_IN, 0), w(D.OP_IN, 1), D.OP_MIN, D.OP_MUL, D.OP_ADD],
                          [], None, None, 4 * 11 * U64),
        'digamma': ([w(D.OP_IN, 0), D.OP_DIGAMMA, w(D.OP_IN, 1), D.OP_MUL], [], [(2, 40), (0.5, 2)],
                    lambda x, y: special.digamma(x) * L(y), 2e-14 + 8 * U64),
        'lgamma': ([w(D.OP_IN, 0), D.OP_LGAMMA, w(D.OP_IN, 1), D.OP_ADD], [], [(3, 40), (0.5, 2)],
                   lambda x, y: special.gammaln(x) + L(y), 2e-14 + 8 * U64),
        'trigamma': ([w(D.OP_IN, 0), D.OP_TRIGAMMA, w(D.OP_IN, 1), D.OP_SUB], [], [(0.2, 40), (-2, -0.5)],
                     lambda x, y: special.polygamma(1, x) - L(y), 2e-14 + 8 * U64),
    }


@pytest.mark.parametrize('size', [7, 2048])
@pytest.mark.parametrize('name', ['arith', 'unary', 'dup swap', 'max min where', 'digamma', 'lgamma',
                                  'trigamma'])
def test_every_opcode_queued_and_standalone(name, size):
    """Every VMP_OP_* word (raw vmp_ewise: DUP is never emitted by the tracer) queued and
    stand-alone: bit for bit the same, and within the bound of the reference."""
    import torch
    rt = _rt()
    ops, consts, ranges, ref_fn, rtol = _opcode_programs()[name]
    rng = np.random.default_rng(len(name) + size)
    if name == 'max min where':
        x, y = rng.standard_normal(size), rng.standard_normal(size)
        u = np.where(rng.random(size) < 0.4, 0.0, rng.uniform(0.5, 2, size))
        v = np.where(u == 0, -np.inf, rng.uniform(0.5, 2, size))
        host = [x, y, u, v]
        m, wv = np.maximum(x, y), np.where(u != 0, v, 0.0)
        ref = np.asarray(m, np.longdouble) + np.asarray(wv, np.longdouble) * np.minimum(x, y)
        mag = np.abs(m) + np.abs(wv * np.minimum(x, y))     # the sum may cancel: bound by magnitudes
    else:
        host = [rng.uniform(lo, hi, size) for lo, hi in ranges]
        ref = np.asarray(ref_fn(*host), np.longdouble)
        mag = np.abs(ref)
    ins = [torch.from_numpy(h).to(rt.device) for h in host]

    def run():
        out = torch.full((size,), np.nan, dtype=torch.float64, device=rt.device)
        _raw_ewise(rt, (size,), ins, ops, consts, out)
        return out

    o0 = _ops(rt)
    with rt.operation():
        q = run()
    assert _ops(rt) - o0 == 1
    q = q.cpu().numpy()
    o0 = _ops(rt)
    s = run()
    rt.synchronize()
    assert _ops(rt) - o0 == 0
    s = s.cpu().numpy()
    assert np.array_equal(q.view(np.int64), s.view(np.int64))
    assert np.all(np.isfinite(q))
    err = np.abs(np.asarray(q, np.longdouble) - ref)
    assert np.all(err <= rtol * mag), float(np.max(err / mag))


# ---- operand lifetime ------------------------------------------------------------------------------
def _alive_ptrs(rt):
    ptrs = set()
    for arrays, out in rt._queue_alive:
        for a in list(arrays) + list(out if isinstance(out, (tuple, list)) else (out,)):
            t = getattr(a, 't', a)
            if hasattr(t, 'data_ptr'):
                ptrs.add(t.untyped_storage().data_ptr())
    return ptrs


def _reuse_block(rt, ptr, numel):
    """Allocate same-sized tensors filled with 1e300 until one lands on `ptr` (or give up); the
    tensors are returned so that they stay allocated."""
    import torch
    held = []
    for _ in range(64):
        t = torch.full((numel,), 1e300, dtype=torch.float64, device=rt.device)
        held.append(t)
        if t.data_ptr() == ptr:
            break
    return held


@pytest.mark.parametrize('n,batch', [(23, 4), (24, 4), (32, 3), (32, 4)])
def test_spd_operand_outlives_its_queued_record(n, batch):
    """C is a temporary: once every Python reference to it and to the factor is gone while the
    inverse is still a record, its block must not be handed out again (a fill of 1e300 would be
    what the record inverts)."""
    from bayespy_amd.darray import DArray
    from bayespy_amd.utils import linalg
    rt = _rt()
    rng = np.random.default_rng(n * batch)
    mats = [_spd(n, 1e2, 1.0, rng) for _ in range(batch)]
    A = np.stack([m for m, _ in mats])
    host = rt.torch.from_numpy(A)
    o0 = _ops(rt)
    with rt.operation():
        C = DArray(host.to(rt.device))           # a temporary made on the device, no flush
        U = linalg.chol(C)
        X, L = linalg.chol_inv(U), linalg.chol_logdet(U)
        ptr = C.t.data_ptr()
        retained = ptr in _alive_ptrs(rt)
        del C, U
        held = _reuse_block(rt, ptr, n * n * batch)
        reused = any(t.data_ptr() == ptr for t in held)
        assert reused != retained            # the block is either kept or handed out again
    assert _ops(rt) - o0 == 1
    Xh, Lh = X.numpy(), L.numpy()
    for b, (Ab, lam) in enumerate(mats):
        _check_inverse(Xh[b], Lh[b], Ab, lam, 'n=%d batch=%d b=%d' % (n, batch, b))
    # control: once the operation is over the block IS free, and the same allocation sequence
    # receives it -- so a record that had not retained C above would have read the fill
    del held
    C2 = DArray(host.to(rt.device))
    ptr2 = C2.t.data_ptr()
    del C2
    assert any(t.data_ptr() == ptr2 for t in _reuse_block(rt, ptr2, n * n * batch))


@pytest.mark.parametrize('kind', ['sum', 'formula', 'formula 8192'])
def test_operands_of_the_largest_queued_sum_and_formula_outlive_the_record(kind):
    from bayespy_amd.darray import DArray, fuse
    from bayespy_amd.utils import misc
    rt = _rt()
    rng = np.random.default_rng(len(kind))
    if kind == 'sum':
        A, x = rng.uniform(0.5, 1.5, (SMALL_SM_KEEP, 16)), rng.uniform(0.5, 1.5, 16)
    else:
        size = 8192 if kind == 'formula 8192' else SMALL_EW_MAX
        A, x = rng.uniform(0.5, 1.5, size), rng.uniform(0.5, 1.5, size)
    xd = _dev(rt, x)
    host = rt.torch.from_numpy(A)
    restore = rt._queue_max_out
    rt.set_tune('small_queue_ew_max', 8192 if kind == 'formula 8192' else restore)
    try:
        o0 = _ops(rt)
        with rt.operation():
            T = DArray(host.to(rt.device))
            r = misc.sum_multiply(T, xd, axis=-1) if kind == 'sum' else fuse(lambda a, b: a * b + a, T, xd)
            ptr = T.t.data_ptr()
            retained = ptr in _alive_ptrs(rt)
            del T
            held = _reuse_block(rt, ptr, A.size)
            reused = any(t.data_ptr() == ptr for t in held)
            assert reused != retained
        assert _ops(rt) - o0 == 1
    finally:
        rt.set_tune('small_queue_ew_max', restore)
    got = r.numpy()
    if kind == 'sum':
        _check_sum(got, [A, x], -1, 1.0, SMALL_SM_KEEP, 16, True, kind)
    else:
        Al, xl = np.asarray(A, np.longdouble), np.asarray(x, np.longdouble)
        ref = Al * xl + Al
        assert np.all(np.abs(got - ref) <= 4 * 5 * U64 * ref)


# ---- the retention rule agrees with the library ------------------------------------------------------
def _retention_cases():
    cases = [('spd', n, b) for n in (8, 9, 16, 22, 23, 24, 32, 33) for b in (1, 2, 3, 4, 5)]
    cases += [('sum', k, r) for k, r in ((1, 32768), (1, 32769), (2048, 16), (2049, 1), (2048, 1),
                                         (16, 2048), (16, 2049), (1024, 32))]
    cases += [('ew', s, m) for s in (1, 2048, 2049, 8192, 8193) for m in (2048, 8192)]
    return cases


def test_retention_rule_covers_every_queued_call():
    """For shapes straddling every threshold: whenever the library queued a call (the record count
    after the flush), the runtime kept that call's arrays alive (rt._queue_alive grew)."""
    from bayespy_amd.darray import fuse
    from bayespy_amd.utils import linalg, misc
    rt = _rt()
    rng = np.random.default_rng(11)
    restore = rt._queue_max_out
    bad = []
    try:
        for kind, p, q in _retention_cases():
            if kind == 'spd':
                A = np.stack([_spd(p, 10.0, 1.0, rng)[0] for _ in range(q)])
                args = (_dev(rt, A),)
                fn = lambda C: linalg.chol(C)
            elif kind == 'sum':
                args = (_dev(rt, rng.standard_normal((p, q))), _dev(rt, rng.standard_normal(q)))
                fn = lambda a, b: misc.sum_multiply(a, b, axis=-1)
            else:
                rt.set_tune('small_queue_ew_max', q)
                args = (_dev(rt, rng.standard_normal(p)),)
                fn = lambda a: fuse(lambda v: v * v + 1.0, a)
            o0 = _ops(rt)
            with rt.operation():
                n0 = len(rt._queue_alive)
                r = fn(*args)
                grew = len(rt._queue_alive) > n0
            queued = _ops(rt) - o0
            if queued and not grew:
                bad.append((kind, p, q))
            del r
    finally:
        rt.set_tune('small_queue_ew_max', restore)
    assert not bad, 'queued by the library but not kept alive: %s' % bad


# ---- non-dense outputs of queued sums (raw C ABI) ----------------------------------------------------
def _raw_sum_rows(rt, A, x, out_ptr, out_stride):
    """out[k * out_stride] = sum_j A[k, j] x[j] (raw vmp_sum_multiply, out_ptr an address)."""
    from bayespy_amd.utils.misc import _workspace
    K, J = A.shape
    ws = _workspace(rt)
    shape = (ctypes.c_int64 * 2)(K, J)
    ins = (ctypes.c_void_p * 2)(A.data_ptr(), x.data_ptr())
    st = (ctypes.c_int64 * 4)(J, 1, 0, 1)
    ost = (ctypes.c_int64 * 2)(out_stride, 0)
    rt.check(rt.lib.vmp_sum_multiply(rt.ctx, 2, shape, 2, ins, st, ost, ctypes.c_uint32(2), 1.0,
                                     ctypes.c_void_p(out_ptr), _vp(ws), ws.numel() * 8))


def _scale_formula(rt, src, n, out, c):
    from bayespy_amd import darray as D
    view = src[:n]
    _raw_ewise(rt, (n,), [view], [D.OP_IN, D.OP_CONST, D.OP_MUL], [c], out)


@pytest.mark.parametrize('K', [64, 300])
def test_queued_sum_written_backwards_then_read(K):
    """A sum writes r in reverse (out = &r[K-1], stride -1); a formula of the same launch reads
    r[0:K/2].  It must see the sum's values, not what r held before the launch."""
    import torch
    rt = _rt()
    rng = np.random.default_rng(K)
    A = torch.from_numpy(rng.standard_normal((K, 9))).to(rt.device)
    x = torch.from_numpy(rng.standard_normal(9)).to(rt.device)
    r = torch.full((K,), -7.0, dtype=torch.float64, device=rt.device)
    half = K // 2
    y = torch.full((half,), np.nan, dtype=torch.float64, device=rt.device)
    o0 = _ops(rt)
    with rt.operation():
        _raw_sum_rows(rt, A, x, r.data_ptr() + 8 * (K - 1), -1)
        _scale_formula(rt, r, half, y, 3.0)
    assert _ops(rt) - o0 == 2
    rt.synchronize()
    s = (A.cpu().numpy() @ x.cpu().numpy())[::-1]
    np.testing.assert_allclose(r.cpu().numpy(), s, rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(y.cpu().numpy(), 3.0 * r.cpu().numpy()[:half])


@pytest.mark.parametrize('K', [64, 300])
def test_queued_sum_written_with_gaps_then_read(K):
    """r holds known values at the odd indices; a sum writes the even ones (stride 2); a formula
    of the same launch reads all 2K - 1.  The odd elements must be what r held."""
    import torch
    rt = _rt()
    rng = np.random.default_rng(K + 1)
    A = torch.from_numpy(rng.standard_normal((K, 9))).to(rt.device)
    x = torch.from_numpy(rng.standard_normal(9)).to(rt.device)
    r0 = np.full(2 * K - 1, np.nan)
    r0[1::2] = 1000.0 + np.arange(K - 1)
    r = torch.from_numpy(r0).to(rt.device)
    y = torch.full((2 * K - 1,), np.nan, dtype=torch.float64, device=rt.device)
    o0 = _ops(rt)
    with rt.operation():
        _raw_sum_rows(rt, A, x, r.data_ptr(), 2)
        _scale_formula(rt, r, 2 * K - 1, y, 3.0)
    assert _ops(rt) - o0 == 2
    rt.synchronize()
    expect = r0.copy()
    expect[0::2] = A.cpu().numpy() @ x.cpu().numpy()
    got = r.cpu().numpy()
    np.testing.assert_array_equal(got[1::2], r0[1::2])
    np.testing.assert_allclose(got[0::2], expect[0::2], rtol=1e-13, atol=1e-13)
    np.testing.assert_array_equal(y.cpu().numpy(), 3.0 * got)
