"""GPU: every kernel of the fused full-covariance Gaussian-mixture block (csrc/vmp_gmm.hip,
vmp_gmm_wide.hip) alone through the C ABI against the long-double restatement of
tests/gmm_pass_host.py.  A test builds a state with ``init_state``, writes exactly the fields the
kernel under test reads at the offsets of ``layout()`` (for the pass: the coefficients C, written
by the test), runs ONE kernel and reads back what it wrote.  The allowance of every comparison is
``dgmm_host.tolerances`` (8 times the deviation of the float64 evaluation from long double, floor
4 ulp) -- measured from the float64 reference, never from the kernel."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gmm_pass_host as H                                           # noqa: E402

LD, F64 = np.longdouble, np.float64
EPS = 2.0 ** -52
SENTINEL, ZS_SENTINEL = -7.5, 123456.75

# one dimension at a time
D_SWEEP = [(300, D, 5) for D in (1, 4, 5, 8, 9, 12, 16, 17, 21, 22, 32)]
K_SWEEP = [(300, D, K) for D in (3, 8, 13, 16, 24, 32) for K in (1, 16, 17, 32, 33, 64)]
N_SWEEP = [(N, D, K) for D, K in ((8, 64), (16, 64), (24, 33))
           for N in (0, 1, 15, 16, 17, 127, 128, 129)]
PASS_SHAPES = sorted(set(D_SWEEP + K_SWEEP + N_SWEEP))
# 282 tiles over two workgroups of at most eight tiles in flight: 18 trips or more per wavefront
STRIDE_SHAPES = [(8, 64), (16, 64), (12, 20), (32, 64), (20, 5)]
STRIDE_N, STRIDE_CAP = 4500, 2
LABEL_SHAPES = [(763, 8, 17), (300, 16, 64), (300, 32, 33)]
CLUSTER_SHAPES = [(1, 1), (8, 4), (8, 5), (9, 5), (16, 64), (17, 3), (32, 64)]


# -- plumbing -------------------------------------------------------------------------------------
def _kernels():
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.gmm import GMMKernels
    rt = get_runtime()
    rt.sync_stream()
    return rt, GMMKernels(rt)


def _up(rt, a, dtype=np.float64):
    return rt.torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(rt.device)


class _State:
    """A packed state from init_state; fields written and read at the offsets of layout()."""

    def __init__(self, D, K, priors=None):
        self.rt, self.k = _kernels()
        self.D, self.K = D, K
        self.L = self.k.layout(D, K)
        self.KP, self.F2P, self.FS = int(self.L.KP), int(self.L.F2P), int(self.L.FS)
        p = priors or dict(alpha0=np.ones(K), beta0=0.7, n0=D + 2.0, V0=np.identity(D))
        self.priors = p
        self.st = self.rt.zeros(int(self.L.total))
        self.k.init_state(D, K, p['alpha0'], p['beta0'], p['n0'], p['V0'], self.st)

    def write(self, off, a):
        a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        self.st[int(off):int(off) + a.size] = _up(self.rt, a)

    def write_T(self, R, S1, S2):
        K, D = self.K, self.D
        T = np.zeros((self.KP, self.FS))
        T[:K, 0], T[:K, 1:1 + D], T[:K, 1 + D:] = R, S1, np.reshape(S2, (K, D * D))
        self.write(self.L.off_T, T)

    def read(self):
        self.rt.synchronize()
        return self.st.cpu().numpy()

    def fields(self):
        s, L, K, D, KP = self.read(), self.L, self.K, self.D, self.KP

        def blk(off, shape):
            return s[int(off):int(off) + int(np.prod(shape))].reshape(shape).copy()
        T = blk(L.off_T, (KP, self.FS))
        return dict(T=T, R=T[:K, 0].copy(), S1=T[:K, 1:1 + D].copy(),
                    S2=T[:K, 1 + D:].reshape(K, D, D).copy(), zs=blk(L.off_zs, (8,)),
                    alpha=blk(L.off_alpha, (K,)), logpi=blk(L.off_alpha + KP, (K,)),
                    mu=blk(L.off_mu, (K, D)), Cmu=blk(L.off_Cmu, (K, D, D)),
                    logdetLmu=blk(L.off_logdetLmu, (K,)), nk=blk(L.off_nk, (K,)),
                    Vk=blk(L.off_Vk, (K, D, D)), Lam=blk(L.off_Lam, (K, D, D)),
                    logdetLam=blk(L.off_logdetLam, (K,)), logdetV=blk(L.off_logdetV, (K,)),
                    C=blk(L.off_C, (KP, self.F2P)), logdetV0=blk(L.off_prior + KP + 2, (1,)),
                    status=float(s[int(L.off_scal) + 3]), bound=blk(L.off_L, (6,)))


def _run_pass(D, K, y, C, labels=None, cap=0):
    """One vmp_gmm_pass (or vmp_gmm_stats_from_labels) over y with the coefficients C (KP, F2P)
    written by the caller; R has 16 sentinel rows behind row N; N = 0: one-row buffers."""
    S = _State(D, K)
    rt, k, L = S.rt, S.k, S.L
    N = len(y)
    S.write(L.off_C, C)
    S.write(L.off_zs, [ZS_SENTINEL, ZS_SENTINEL])
    Y = _up(rt, y if N else np.zeros((1, D)))
    R = rt.torch.full((max(N, 1) + 16, K), SENTINEL, dtype=rt.torch.float64, device=rt.device)
    ws = rt.empty(int(k.workspace_doubles(D, K)))
    try:
        rt.set_tune('gmm_grid_cap', cap)
        if labels is None:
            k.pass_(Y, N, D, K, R, S.st, ws)
        else:
            k.stats_from_labels(Y, N, D, K, _up(rt, labels, np.int64), R, S.st, ws)
    finally:
        rt.set_tune('gmm_grid_cap', 0)
    f = S.fields()
    Rh = R.cpu().numpy()
    f.update(r=Rh[:N].copy(), tail=Rh[N:N + 16].copy(), sum_lse=f['zs'][0], rphi=f['zs'][1])
    return f


@functools.lru_cache(None)
def _case(N, D, K):
    """Inputs and both restatements of a pass shape, computed once and left unchanged."""
    _, k = _kernels()
    L = k.layout(D, K)
    g = H.make_inputs(N, D, K)
    C = H.restate_C(g['Lam'], g['mu'], g['Cmu'], g['logdetLam'], g['logpi'], int(L.KP), int(L.F2P),
                    dtype=F64)
    ld, f64 = H.restate_pass(g['y'], C[:K]), H.restate_pass(g['y'], C[:K], dtype=F64)
    tol, dev = H.pass_tolerances(ld, f64)
    return g, C, ld, tol, dev


def _check_accuracy(got, ld, tol, dev, shape, keys=H.PASS_QUANTITIES, what='kernel'):
    for key in keys:
        err = H.error(got[key], ld[key])
        print('%s (N, D, K) = %s: float64 deviation %.3g, %s %.3g, allowed %.3g'
              % (key, shape, dev[key], what, err, tol[key]))
    if 'rphi' in keys:
        print('rphi (N, D, K) = %s: sum |C T| = %.6g, |rphi| = %.6g, cancellation factor %.3g'
              % (shape, float(ld['rphi_mag']), abs(float(ld['rphi'])),
                 float(ld['rphi_mag']) / max(abs(float(ld['rphi'])), 1e-300)))
    for key in keys:
        err = H.error(got[key], ld[key])
        assert err <= tol[key], (key, err, tol[key])


def _check_structure(got, N, D, K):
    r = got['r']
    assert r.shape == (N, K) and np.all(r >= 0)
    if N:
        assert np.max(np.abs(r.astype(LD).sum(axis=1) - 1)) <= 4 * EPS
    assert abs(float(got['R'].astype(LD).sum()) - N) <= 4 * np.spacing(float(N))
    np.testing.assert_array_equal(got['S2'], np.swapaxes(got['S2'], 1, 2))
    assert not got['T'][K:].any()
    np.testing.assert_array_equal(got['tail'], SENTINEL)


def _same_bits(a, b, keys=('r', 'T', 'zs')):
    for key in keys:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# -- the pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,D,K', PASS_SHAPES)
def test_pass_against_long_double_restatement(N, D, K):
    """Accuracy of r, R, S1, S2, sum lse and <C, T>; rows of r sum to one, S2 symmetric bit for
    bit, padded clusters and the rows of r behind N untouched; two calls leave the same bits; a
    row's r depends on that row alone (the rows rolled by five)."""
    g, C, ld, tol, dev = _case(N, D, K)
    got = _run_pass(D, K, g['y'], C)
    _check_accuracy(got, ld, tol, dev, (N, D, K))
    _check_structure(got, N, D, K)
    if N == 0:
        assert not got['T'].any() and got['zs'][0] == 0 and got['zs'][1] == 0
    _same_bits(got, _run_pass(D, K, g['y'], C))
    if N > 1:
        rolled = _run_pass(D, K, np.roll(g['y'], 5, axis=0), C)
        np.testing.assert_array_equal(rolled['r'], np.roll(got['r'], 5, axis=0))


@pytest.mark.parametrize('D,K', STRIDE_SHAPES)
def test_pass_grid_stride_loop(D, K):
    """gmm_grid_cap = 2 at N = 4500: every wavefront walks 18 tiles or more (the flush of the
    running product of sum lse and its residual, accumulators carried across tiles, the constant
    slots of the y tile written again after the r tile, ragged last trips, the surplus empty trips
    of the pair-split and wide forms, the prefetch one stride past the end)."""
    N = STRIDE_N
    assert (N + 15) // 16 >= 17 * 8 * STRIDE_CAP
    g, C, ld, tol, dev = _case(N, D, K)
    free = _run_pass(D, K, g['y'], C)
    capped = _run_pass(D, K, g['y'], C, cap=STRIDE_CAP)
    _check_accuracy(capped, ld, tol, dev, (N, D, K), what='capped kernel')
    _check_accuracy(free, ld, tol, dev, (N, D, K))
    _check_structure(capped, N, D, K)
    _check_structure(free, N, D, K)
    np.testing.assert_array_equal(capped['r'], free['r'])
    for key in ('R', 'S1', 'S2', 'sum_lse', 'rphi'):
        assert H.error(capped[key], np.asarray(free[key], dtype=LD)) <= tol[key], key
    _same_bits(capped, _run_pass(D, K, g['y'], C, cap=STRIDE_CAP))


@pytest.mark.parametrize('D,K', H.EDGE_SHAPES)
def test_pass_edge_columns(D, K):
    """An impossible cluster, two clusters with identical coefficients (one in each half of the
    pair-split form), a row whose phi spread over k exceeds 800 and an all-zero row; inputs on
    which the reference recipe yields no NaN (tests/test_gmm_pass_host.py)."""
    S = _State(D, K)
    y, C = H.edge_inputs(D, K, S.KP, S.F2P)
    N = len(y)
    ld, f64 = H.restate_pass(y, C[:K]), H.restate_pass(y, C[:K], dtype=F64)
    tol, dev = H.pass_tolerances(ld, f64)
    got = _run_pass(D, K, y, C)
    assert np.isfinite(got['rphi']) and np.isfinite(got['sum_lse']) and np.isfinite(got['T']).all()
    assert not got['r'][:, H.EDGE_DEAD].any() and not got['T'][H.EDGE_DEAD].any()
    a, b = H.EDGE_TWINS
    np.testing.assert_array_equal(got['r'][:, a], got['r'][:, b])
    phi = H.features(y, S.F2P)[H.EDGE_FAR_ROW] @ np.asarray(C[:K], dtype=LD).T
    lost = phi - phi[np.isfinite(phi)].max() < -801
    assert lost.sum() >= 2
    assert not got['r'][H.EDGE_FAR_ROW, lost].any() and not f64['r'][H.EDGE_FAR_ROW, lost].any()
    _check_accuracy(got, ld, tol, dev, (N, D, K))
    _check_structure(got, N, D, K)


@pytest.mark.parametrize('N,D,K', LABEL_SHAPES)
def test_labelled_pass(N, D, K):
    g, C, _, _, _ = _case(N, D, K)
    got = _run_pass(D, K, g['y'], C, labels=g['labels'])
    one = np.eye(K)[g['labels']]
    np.testing.assert_array_equal(got['r'], one)
    np.testing.assert_array_equal(got['R'], np.bincount(g['labels'], minlength=K))
    ld = H.restate_pass(g['y'], C[:K], labels=g['labels'])
    f64 = H.restate_pass(g['y'], C[:K], labels=g['labels'], dtype=F64)
    tol, dev = H.tolerances(ld, f64, ('S1', 'S2'))
    _check_accuracy(got, ld, tol, dev, (N, D, K), keys=('S1', 'S2'))
    np.testing.assert_array_equal(got['S2'], np.swapaxes(got['S2'], 1, 2))
    assert not got['T'][K:].any()
    np.testing.assert_array_equal(got['tail'], SENTINEL)
    np.testing.assert_array_equal(got['zs'][:2], ZS_SENTINEL)


# -- the coefficient matrix ------------------------------------------------------------------------
@pytest.mark.parametrize('prior_only', [False, True])
@pytest.mark.parametrize('D,K', [(D, K) for D in (4, 8, 9, 16, 17, 32) for K in (5, 64)])
def test_prepare_z(D, K, prior_only):
    g = H.make_inputs(64, D, K)
    S = _State(D, K)
    L, KP, F2P = S.L, S.KP, S.F2P
    for off, key in ((L.off_mu, 'mu'), (L.off_Cmu, 'Cmu'), (L.off_Lam, 'Lam'),
                     (L.off_logdetLam, 'logdetLam'), (L.off_alpha + KP, 'logpi')):
        S.write(off, g[key])
    S.write(L.off_C, np.full(KP * F2P, SENTINEL))
    S.k.prepare_z(D, K, prior_only, S.st)
    C = S.fields()['C']
    args = (g['Lam'], g['mu'], g['Cmu'], g['logdetLam'], g['logpi'], KP, F2P, prior_only)
    ld, f64 = H.restate_C(*args), H.restate_C(*args, dtype=F64)
    npair, F2 = H.n_pairs(D), H.n_features(D)
    cols = dict(C_pairs=slice(0, npair), C_linear=slice(npair, npair + D),
                C_constant=slice(npair + D, F2))
    tol, dev = H.tolerances({k: ld[:K, s] for k, s in cols.items()},
                            {k: f64[:K, s] for k, s in cols.items()}, tuple(cols))
    _check_accuracy({k: C[:K, s] for k, s in cols.items()}, {k: ld[:K, s] for k, s in cols.items()},
                    tol, dev, (64, D, K), keys=tuple(cols))
    np.testing.assert_array_equal(C[K:], f64[K:])            # 0, and -inf in the constant column
    assert np.all(np.isneginf(C[K:, F2 - 1])) and not C[K:, :F2 - 1].any()
    assert not C[:, F2:].any()


# -- the per-cluster kernels -----------------------------------------------------------------------
@functools.lru_cache(None)
def _cluster_case(D, K):
    """Soft statistics (a long-double pass, rounded), priors with a V0 of condition 1e3, and a
    consistent float64 state after one update of every node."""
    N = 300
    g = dict(H.make_inputs(N, D, K))
    C = H.restate_C(g['Lam'], g['mu'], g['Cmu'], g['logdetLam'], g['logpi'], K, H.n_features(D),
                    dtype=F64)
    p = H.restate_pass(g['y'], C)
    g.update({k: np.asarray(p[k], dtype=F64) for k in ('R', 'S1', 'S2', 'sum_lse', 'rphi')})
    return g


def _cluster_state(D, K, T=True):
    g = _cluster_case(D, K)
    S = _State(D, K, {k: g[k] for k in ('alpha0', 'beta0', 'n0', 'V0')})
    if T:
        S.write_T(g['R'], g['S1'], g['S2'])
    return g, S


def _check_clusters(got, ld, f64, shape, keys, per_cluster=()):
    tol, dev = H.tolerances(ld, f64, keys)
    for key in keys:
        if key in per_cluster:
            t, d = H.cluster_tolerances(ld, f64, key)
            e = H.cluster_errors(got[key], ld[key])
            worst = int(np.argmax(e / t))
            print('%s (D, K) = %s: cluster %d float64 deviation %.3g, kernel %.3g, allowed %.3g'
                  % (key, shape, worst, d[worst], e[worst], t[worst]))
        else:
            print('%s (D, K) = %s: float64 deviation %.3g, kernel %.3g, allowed %.3g'
                  % (key, shape, dev[key], H.error(got[key], ld[key]), tol[key]))
    for key in keys:
        if key in per_cluster:
            t, _ = H.cluster_tolerances(ld, f64, key)
            e = H.cluster_errors(got[key], ld[key])
            assert np.all(e <= t), (key, e, t)
        else:
            err = H.error(got[key], ld[key])
            assert err <= tol[key], (key, err, tol[key])


@pytest.mark.parametrize('D,K', CLUSTER_SHAPES)
def test_init_state(D, K):
    g, S = _cluster_state(D, K, T=False)
    args = (g['alpha0'], g['beta0'], g['n0'], g['V0'])
    got = S.fields()
    assert got['status'] == 0
    _check_clusters(got, H.restate_init(*args), H.restate_init(*args, dtype=F64), (D, K),
                    ('alpha', 'logpi', 'nk', 'Vk', 'mu', 'Cmu', 'logdetLmu', 'Lam', 'logdetV',
                     'logdetLam', 'logdetV0'), per_cluster=('Lam', 'Cmu'))


@pytest.mark.parametrize('D,K', CLUSTER_SHAPES)
def test_update_mu(D, K):
    g, S = _cluster_state(D, K)
    S.write(S.L.off_Lam, g['Lam'])
    S.k.update_mu(D, K, S.st)
    got = S.fields()
    assert got['status'] == 0
    args = (g['R'], g['S1'], g['Lam'], g['beta0'])
    _check_clusters(got, H.restate_update_mu(*args), H.restate_update_mu(*args, dtype=F64), (D, K),
                    ('mu', 'Cmu', 'logdetLmu'), per_cluster=('mu', 'Cmu'))


@pytest.mark.parametrize('D,K', CLUSTER_SHAPES)
def test_update_lambda(D, K):
    g, S = _cluster_state(D, K)
    S.write(S.L.off_mu, g['mu'])
    S.write(S.L.off_Cmu, g['Cmu'])
    S.k.update_lambda(D, K, S.st)
    got = S.fields()
    assert got['status'] == 0
    args = (g['R'], g['S1'], g['S2'], g['mu'], g['Cmu'], g['n0'], g['V0'])
    _check_clusters(got, H.restate_update_lambda(*args),
                    H.restate_update_lambda(*args, dtype=F64), (D, K),
                    ('nk', 'Vk', 'Lam', 'logdetV', 'logdetLam'), per_cluster=('Lam',))


@pytest.mark.parametrize('D,K', [(8, 5), (9, 5), (17, 3)])
def test_update_lambda_reports_an_indefinite_cluster(D, K):
    """One V_k indefinite: the status slot holds VMP_ERR_NOT_POSDEF (a status code, no fault) and
    the other clusters -- those of the same workgroup in the four-clusters form included -- are
    as accurate as ever."""
    from bayespy_amd import _lib
    g, S = _cluster_state(D, K)
    bad = 1
    S2 = g['S2'].copy()
    S2[bad] = -1e3 * np.identity(D)
    S.write_T(g['R'], g['S1'], S2)
    S.write(S.L.off_mu, g['mu'])
    S.write(S.L.off_Cmu, g['Cmu'])
    S.k.update_lambda(D, K, S.st)
    got = S.fields()
    assert got['status'] == _lib.VMP_ERR_NOT_POSDEF
    keep = np.arange(K) != bad
    args = (g['R'][keep], g['S1'][keep], g['S2'][keep], g['mu'][keep], g['Cmu'][keep], g['n0'],
            g['V0'])
    keys = ('nk', 'Vk', 'Lam', 'logdetV', 'logdetLam')
    _check_clusters({k: got[k][keep] for k in keys}, H.restate_update_lambda(*args),
                    H.restate_update_lambda(*args, dtype=F64), (D, K), keys, per_cluster=('Lam',))


@pytest.mark.parametrize('D,K', CLUSTER_SHAPES)
def test_update_alpha(D, K):
    g, S = _cluster_state(D, K)
    S.k.update_alpha(D, K, S.st)
    _check_clusters(S.fields(), H.restate_update_alpha(g['alpha0'], g['R']),
                    H.restate_update_alpha(g['alpha0'], g['R'], dtype=F64), (D, K),
                    ('alpha', 'logpi'))


@pytest.mark.parametrize('D,K', CLUSTER_SHAPES)
def test_lower_bound(D, K):
    """The five terms and their sum from a given consistent state.  L_alpha at (32, 64) is the
    case that made the kernel form the alpha term from (value, rounding error) pairs: with plain
    vmp_lgamma and a sequential sum it was 5.06e-13 off where 4.09e-13 is allowed, 2.2 ulp of
    ln Gamma(sum alpha) = 1780.  At K = 1 the term is exactly 0."""
    g, S = _cluster_state(D, K)
    L, KP = S.L, S.KP
    s = {k: g[k] for k in ('R', 'S1', 'S2', 'sum_lse', 'rphi', 'alpha0', 'beta0', 'n0', 'V0')}
    s.update(H.restate_update_mu(g['R'], g['S1'], g['Lam'], g['beta0'], dtype=F64))
    s.update(H.restate_update_lambda(g['R'], g['S1'], g['S2'], s['mu'], s['Cmu'], g['n0'], g['V0'],
                                     dtype=F64))
    s.update(H.restate_update_alpha(g['alpha0'], g['R'], dtype=F64))
    for off, key in ((L.off_alpha, 'alpha'), (L.off_alpha + KP, 'logpi'), (L.off_mu, 'mu'),
                     (L.off_Cmu, 'Cmu'), (L.off_logdetLmu, 'logdetLmu'), (L.off_nk, 'nk'),
                     (L.off_Vk, 'Vk'), (L.off_Lam, 'Lam'), (L.off_logdetLam, 'logdetLam'),
                     (L.off_logdetV, 'logdetV')):
        S.write(off, s[key])
    S.write(L.off_zs, [s['sum_lse'], s['rphi']])
    S.k.lower_bound(D, K, S.st)
    b = S.fields()['bound']
    got = dict(zip(H.BOUND_QUANTITIES, b))
    assert got['L'] == (((b[0] + b[1]) + b[2]) + b[3]) + b[4]
    _check_clusters(got, H.restate_lower_bound(s), H.restate_lower_bound(s, dtype=F64), (D, K),
                    H.BOUND_QUANTITIES)


# -- argument checks: nothing is launched ------------------------------------------------------------
def test_argument_checks_and_limits():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(64)
    p = ctypes.c_void_p(z.data_ptr())
    INV, UNS = _lib.VMP_ERR_INVALID, _lib.VMP_ERR_UNSUPPORTED

    def pass_(c, N, D, K, Y=p, R=p, st=p, ws=p):
        return lib.vmp_gmm_pass(c, Y, N, D, K, R, st, ws)

    def labels(c, N, D, K, Y=p, lab=p, R=p, st=p, ws=p):
        return lib.vmp_gmm_stats_from_labels(c, Y, N, D, K, lab, R, st, ws)
    for fn, names in ((pass_, ('Y', 'R', 'st', 'ws')), (labels, ('Y', 'lab', 'R', 'st', 'ws'))):
        assert fn(None, 4, 4, 4) == INV
        for name in names:
            assert fn(ctx, 4, 4, 4, **{name: None}) == INV, (fn.__name__, name)
        assert fn(ctx, 4, 0, 4) == INV and fn(ctx, 4, 4, 0) == INV and fn(ctx, -1, 4, 4) == INV
        assert fn(ctx, 4, 33, 4) == UNS and fn(ctx, 4, 4, 65) == UNS
    L = _lib.GMMLayout()
    assert lib.vmp_gmm_get_layout(4, 4, None) == INV
    assert lib.vmp_gmm_get_layout(0, 4, ctypes.byref(L)) == INV
    assert lib.vmp_gmm_get_layout(4, 0, ctypes.byref(L)) == INV
    assert lib.vmp_gmm_get_layout(33, 4, ctypes.byref(L)) == UNS
    assert lib.vmp_gmm_get_layout(4, 65, ctypes.byref(L)) == UNS
    assert lib.vmp_gmm_get_layout(32, 64, ctypes.byref(L)) == _lib.VMP_OK and L.F2P == 576
    a0, V0 = np.ones(4), np.identity(4)
    ha, hv = (ctypes.c_void_p(a.ctypes.data) for a in (a0, V0))

    def init(c, D, K, beta0=1.0, n0=6.0, alpha=ha, V=hv, st=p):
        return lib.vmp_gmm_init_state(c, D, K, alpha, beta0, n0, V, st)
    assert init(None, 4, 4) == INV
    for name in ('alpha', 'V', 'st'):
        assert init(ctx, 4, 4, **{name: None}) == INV, name
    assert init(ctx, 0, 4) == INV and init(ctx, 4, 0) == INV
    assert init(ctx, 33, 4) == UNS and init(ctx, 4, 65) == UNS
    assert init(ctx, 4, 4, beta0=0.0) == INV and init(ctx, 4, 4, beta0=-1.0) == INV
    assert init(ctx, 4, 4, n0=3.0) == INV and init(ctx, 4, 4, n0=2.5) == INV
    bad = np.array([1.0, 0.0, 1.0, 1.0])
    assert init(ctx, 4, 4, alpha=ctypes.c_void_p(bad.ctypes.data)) == _lib.VMP_ERR_NOT_POSITIVE
    bad[1] = -2.0
    assert init(ctx, 4, 4, alpha=ctypes.c_void_p(bad.ctypes.data)) == _lib.VMP_ERR_NOT_POSITIVE
    rt.synchronize()
    assert not z.cpu().numpy().any()
