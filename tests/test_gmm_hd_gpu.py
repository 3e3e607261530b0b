"""GPU: the high-dimensional form of the fused Gaussian-mixture block (csrc/vmp_gmm_hd.hip,
vmp_gmm_hd_dev.h; 33 <= D <= 64): every kernel alone through the C ABI against the long-double
restatements of tests/gmm_pass_host.py, as tests/test_gmm_pass_gpu.py does for D <= 32, and the plan
end to end against oracle/gmm.py.  The allowance of every comparison is ``dgmm_host.tolerances``
(8 times the deviation of the float64 evaluation from long double, floor 4 ulp) --
measured from the float64 reference, never from the kernel."""
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
import test_gmm_pass_gpu as B                                       # noqa: E402  (its plumbing)

LD, F64 = np.longdouble, np.float64
SENTINEL, ZS_SENTINEL = B.SENTINEL, B.ZS_SENTINEL
_up, _check_accuracy, _check_structure, _same_bits = (B._up, B._check_accuracy, B._check_structure,
                                                      B._same_bits)
_check_clusters, _cluster_case = B._check_clusters, B._cluster_case

# one dimension at a time; 255 .. 257: around the 256 points of a workgroup's trip
PASS_SHAPES = sorted(set([(300, D, 5) for D in (33, 40, 48, 49, 64)]
                         + [(300, D, K) for D in (33, 64) for K in (1, 16, 17, 64)]
                         + [(N, 48, 33) for N in (0, 1, 15, 16, 17, 255, 256, 257)]))
STRIDE_N, STRIDE_CAP = 4500, 2
CLUSTER_SHAPES = [(33, 3), (48, 5), (64, 64)]


def natural_C(Cc, D, F2P):
    """A compact coefficient table (restate_C: pairs a <= b, linear, constant) in the natural order
    of the high-dimensional form: [c, h (D), A (D x D, symmetric: a pair's coefficient halved)]."""
    a, b = H.pair_index(D)
    npair = H.n_pairs(D)
    A = np.zeros((len(Cc), D, D), dtype=Cc.dtype)
    A[:, a, b] = np.where(a == b, Cc[:, :npair], Cc[:, :npair] / 2)
    A[:, b, a] = A[:, a, b]
    out = np.zeros((len(Cc), F2P), dtype=Cc.dtype)
    out[:, 0], out[:, 1:1 + D] = Cc[:, npair + D], Cc[:, npair:npair + D]
    out[:, 1 + D:1 + D + D * D] = A.reshape(len(Cc), D * D)
    return out


def _kernels(hd=True):
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.gmm import GMMKernels
    from bayespy_amd.inference.plans.gmm_hd import HighDimGMMKernels
    rt = get_runtime()
    rt.sync_stream()
    return rt, (HighDimGMMKernels if hd else GMMKernels)(rt)


class _State(B._State):
    """B._State (write, write_T, fields) on the kernels of this form (hd) or of the block."""

    def __init__(self, D, K, priors=None, hd=True):
        self.rt, self.k = _kernels(hd)
        self.D, self.K = D, K
        self.L = self.k.layout(D, K)
        self.KP, self.F2P, self.FS = int(self.L.KP), int(self.L.F2P), int(self.L.FS)
        p = priors or dict(alpha0=np.ones(K), beta0=0.7, n0=D + 2.0, V0=np.identity(D))
        self.st = self.rt.zeros(int(self.L.total))
        self.k.init_state(D, K, p['alpha0'], p['beta0'], p['n0'], p['V0'], self.st)

def _run_pass(D, K, y, Cc, labels=None, cap=0, hd=True):
    """One pass (or labelled pass) over y with the compact coefficients Cc (KP, >= F2), laid out as
    the form under test wants them; R has 16 sentinel rows behind row N."""
    S = _State(D, K, hd=hd)
    rt, k, L = S.rt, S.k, S.L
    N = len(y)
    C = natural_C(Cc, D, S.F2P) if hd else np.pad(Cc, ((0, 0), (0, S.F2P - Cc.shape[1])))
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
    KP = 16 * (1 << int(np.ceil(np.log2(max(1, (K + 15) // 16)))))
    g = H.make_inputs(N, D, K)
    C = H.restate_C(g['Lam'], g['mu'], g['Cmu'], g['logdetLam'], g['logpi'], KP, H.n_features(D),
                    dtype=F64)
    ld, f64 = H.restate_pass(g['y'], C[:K]), H.restate_pass(g['y'], C[:K], dtype=F64)
    tol, dev = H.pass_tolerances(ld, f64)
    return g, C, ld, tol, dev


# -- the pass ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,D,K', PASS_SHAPES)
def test_pass_against_long_double_restatement(N, D, K):
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


@pytest.mark.parametrize('D,K', [(33, 5), (64, 64)])
def test_pass_grid_stride_loop(D, K):
    """gmm_grid_cap = 2 at N = 4500: nine trips per workgroup of the responsibility kernel, 36 slabs
    per chunk of the second-moment kernel, ragged last ones."""
    N = STRIDE_N
    g, C, ld, tol, dev = _case(N, D, K)
    free = _run_pass(D, K, g['y'], C)
    capped = _run_pass(D, K, g['y'], C, cap=STRIDE_CAP)
    _check_accuracy(capped, ld, tol, dev, (N, D, K), what='capped kernel')
    _check_accuracy(free, ld, tol, dev, (N, D, K))
    _check_structure(capped, N, D, K)
    _check_structure(free, N, D, K)
    np.testing.assert_array_equal(capped['r'], free['r'])
    _same_bits(capped, _run_pass(D, K, g['y'], C, cap=STRIDE_CAP))


def test_pass_agrees_with_the_block_at_its_limit():
    """D = 32, K = 64: this form and vmp_gmm_pass on the same y and coefficients, each in its own
    layout, both within the allowance of the same long-double result."""
    N, D, K = 300, 32, 64
    g, C, ld, tol, dev = _case(N, D, K)
    _check_accuracy(_run_pass(D, K, g['y'], C), ld, tol, dev, (N, D, K), what='high-dim form')
    _check_accuracy(_run_pass(D, K, g['y'], C, hd=False), ld, tol, dev, (N, D, K), what='block')


@pytest.mark.parametrize('N,D,K', [(763, 40, 17), (300, 64, 33)])
def test_labelled_pass(N, D, K):
    g, C, _, _, _ = _case(N, D, K)
    got = _run_pass(D, K, g['y'], C, labels=g['labels'])
    np.testing.assert_array_equal(got['r'], np.eye(K)[g['labels']])
    np.testing.assert_array_equal(got['R'], np.bincount(g['labels'], minlength=K))
    ld = H.restate_pass(g['y'], C[:K], labels=g['labels'])
    f64 = H.restate_pass(g['y'], C[:K], labels=g['labels'], dtype=F64)
    tol, dev = H.tolerances(ld, f64, ('S1', 'S2'))
    _check_accuracy(got, ld, tol, dev, (N, D, K), keys=('S1', 'S2'))
    np.testing.assert_array_equal(got['S2'], np.swapaxes(got['S2'], 1, 2))
    assert not got['T'][K:].any()
    np.testing.assert_array_equal(got['tail'], SENTINEL)
    np.testing.assert_array_equal(got['zs'][:2], ZS_SENTINEL)


def test_pass_edge_columns():
    """An impossible cluster, twin clusters, a row whose phi spread over k exceeds 800 and an
    all-zero row (gmm_pass_host.edge_inputs) at (D, K) = (64, 64)."""
    D, K = 64, 64
    y, C = H.edge_inputs(D, K, K, H.n_features(D))
    N = len(y)
    ld, f64 = H.restate_pass(y, C[:K]), H.restate_pass(y, C[:K], dtype=F64)
    assert np.isfinite(f64['r']).all() and np.isfinite(f64['T']).all()
    tol, dev = H.pass_tolerances(ld, f64)
    got = _run_pass(D, K, y, C)
    assert np.isfinite(got['rphi']) and np.isfinite(got['sum_lse']) and np.isfinite(got['T']).all()
    assert not got['r'][:, H.EDGE_DEAD].any() and not got['T'][H.EDGE_DEAD].any()
    a, b = H.EDGE_TWINS
    np.testing.assert_array_equal(got['r'][:, a], got['r'][:, b])
    phi = H.features(y, H.n_features(D))[H.EDGE_FAR_ROW] @ np.asarray(C[:K], dtype=LD).T
    lost = phi - phi[np.isfinite(phi)].max() < -801
    assert lost.sum() >= 2 and not got['r'][H.EDGE_FAR_ROW, lost].any()
    _check_accuracy(got, ld, tol, dev, (N, D, K))
    _check_structure(got, N, D, K)


# -- the coefficient table and the per-cluster kernels ---------------------------------------------
@pytest.mark.parametrize('prior_only', [False, True])
@pytest.mark.parametrize('D,K', CLUSTER_SHAPES)
def test_prepare_z(D, K, prior_only):
    g = H.make_inputs(64, D, K)
    S = _State(D, K)
    L, KP, F2P, FS = S.L, S.KP, S.F2P, S.FS
    for off, key in ((L.off_mu, 'mu'), (L.off_Cmu, 'Cmu'), (L.off_Lam, 'Lam'),
                     (L.off_logdetLam, 'logdetLam'), (L.off_alpha + KP, 'logpi')):
        S.write(off, g[key])
    S.write(L.off_C, np.full(KP * F2P, SENTINEL))
    S.k.prepare_z(D, K, prior_only, S.st)
    C = S.fields()['C']
    args = (g['Lam'], g['mu'], g['Cmu'], g['logdetLam'], g['logpi'], KP, H.n_features(D), prior_only)
    ld, f64 = natural_C(H.restate_C(*args), D, F2P), natural_C(H.restate_C(*args, dtype=F64), D, F2P)
    cols = dict(C_constant=slice(0, 1), C_linear=slice(1, 1 + D), C_matrix=slice(1 + D, FS))
    tol, dev = H.tolerances({k: ld[:K, s] for k, s in cols.items()},
                            {k: f64[:K, s] for k, s in cols.items()}, tuple(cols))
    _check_accuracy({k: C[:K, s] for k, s in cols.items()}, {k: ld[:K, s] for k, s in cols.items()},
                    tol, dev, (64, D, K), keys=tuple(cols))
    A = C[:K, 1 + D:FS].reshape(K, D, D)
    np.testing.assert_array_equal(A, np.swapaxes(A, 1, 2))
    assert np.all(np.isneginf(C[K:, 0])) and not C[K:, 1:].any() and not C[:, FS:].any()


def _cluster_state(D, K, T=True):
    g = _cluster_case(D, K)
    S = _State(D, K, {k: g[k] for k in ('alpha0', 'beta0', 'n0', 'V0')})
    if T:
        S.write_T(g['R'], g['S1'], g['S2'])
    return g, S


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


@pytest.mark.parametrize('D,K,bad', [(D, K, None) for D, K in CLUSTER_SHAPES] + [(40, 3, 1)])
def test_update_lambda(D, K, bad):
    """bad: that cluster's V_k is indefinite -- the status word holds VMP_ERR_NOT_POSDEF (no fault)
    and the other clusters are as accurate as ever."""
    from bayespy_amd import _lib
    g, S = _cluster_state(D, K)
    S2 = g['S2'].copy()
    if bad is not None:
        S2[bad] = -1e3 * np.identity(D)
    S.write_T(g['R'], g['S1'], S2)
    S.write(S.L.off_mu, g['mu'])
    S.write(S.L.off_Cmu, g['Cmu'])
    S.k.update_lambda(D, K, S.st)
    got = S.fields()
    assert got['status'] == (0 if bad is None else _lib.VMP_ERR_NOT_POSDEF)
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
        return lib.vmp_gmm_hd_pass(c, Y, N, D, K, R, st, ws)

    def labels(c, N, D, K, Y=p, lab=p, R=p, st=p, ws=p):
        return lib.vmp_gmm_hd_stats_from_labels(c, Y, N, D, K, lab, R, st, ws)
    for fn, names in ((pass_, ('Y', 'R', 'st', 'ws')), (labels, ('Y', 'lab', 'R', 'st', 'ws'))):
        assert fn(None, 4, 40, 4) == INV
        for name in names:
            assert fn(ctx, 4, 40, 4, **{name: None}) == INV, (fn.__name__, name)
        assert fn(ctx, 4, 0, 4) == INV and fn(ctx, 4, 40, 0) == INV and fn(ctx, -1, 40, 4) == INV
        assert fn(ctx, 4, 65, 4) == UNS and fn(ctx, 4, 40, 65) == UNS
    L = _lib.GMMLayout()
    assert lib.vmp_gmm_hd_get_layout(40, 4, None) == INV
    assert lib.vmp_gmm_hd_get_layout(0, 4, ctypes.byref(L)) == INV
    assert lib.vmp_gmm_hd_get_layout(65, 4, ctypes.byref(L)) == UNS
    assert lib.vmp_gmm_hd_get_layout(40, 65, ctypes.byref(L)) == UNS
    assert lib.vmp_gmm_hd_get_layout(64, 64, ctypes.byref(L)) == _lib.VMP_OK
    assert (L.DP, L.KP, L.FS, L.F2P) == (64, 64, 4161, 4168)
    for fn in (lib.vmp_gmm_hd_update_mu, lib.vmp_gmm_hd_update_lambda, lib.vmp_gmm_hd_update_alpha,
               lib.vmp_gmm_hd_lower_bound):
        assert fn(ctx, 40, 4, None) == INV and fn(None, 40, 4, p) == INV
        assert fn(ctx, 65, 4, p) == UNS and fn(ctx, 40, 65, p) == UNS
    assert lib.vmp_gmm_hd_prepare_z(ctx, 40, 4, 0, None) == INV
    assert lib.vmp_gmm_hd_prepare_z(ctx, 65, 4, 0, p) == UNS
    a0, V0 = np.ones(4), np.identity(40)
    ha, hv = (ctypes.c_void_p(a.ctypes.data) for a in (a0, V0))
    assert lib.vmp_gmm_hd_init_state(ctx, 40, 4, None, 1.0, 42.0, hv, p) == INV
    assert lib.vmp_gmm_hd_init_state(ctx, 65, 4, ha, 1.0, 70.0, hv, p) == UNS
    assert lib.vmp_gmm_hd_init_state(ctx, 40, 4, ha, 1.0, 39.0, hv, p) == INV
    rt.synchronize()
    assert not z.cpu().numpy().any()


# -- end to end ------------------------------------------------------------------------------------
def _build(y, lab0, K, engine):
    from bayespy_amd.nodes import GaussianARD, Gaussian, Wishart, Dirichlet, Categorical, Mixture
    from bayespy_amd.inference import VB
    N, D = y.shape
    alpha = Dirichlet(1e-3 * np.ones(K), name='alpha')
    z = Categorical(alpha, plates=(N,), name='z')
    mu = GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
    Lam = Wishart(D, 0.01 * np.identity(D), plates=(K,), name='Lambda')
    Y = Mixture(z, Gaussian, mu, Lam, plates=(N,), name='Y')
    z.initialize_from_value(lab0)
    Y.observe(y)
    Q = VB(Y, mu, Lam, z, alpha, engine=engine)
    Q.ignore_bound_checks = True
    return Q


def test_fused_high_dim_gmm_vs_oracle(tmp_path):
    """D = 40, K = 4, N = 600, five sweeps from fixed labels against oracle/gmm.py at the tolerances
    of test_gmm_gpu.py::test_fused_gmm_vs_oracle; then a checkpoint round trip."""
    from oracle.gmm import GMMOracle, make_gmm_data
    N, D, K, iters = 600, 40, 4, 5
    y, lab0 = make_gmm_data(N, D, K, seed=N + D + K)
    Q = _build(y, lab0, K, 'fused+dims')
    assert type(Q.plans[0]).__name__ == 'HighDimGMMPlan'
    o = GMMOracle(y, lab0, K)
    Q.update(repeat=iters, verbose=False)
    o.iterate(iters)
    np.testing.assert_allclose(Q.L[:iters], np.array(o.L), rtol=1e-9)
    np.testing.assert_allclose(Q['z'].u[0], o.r, rtol=1e-7, atol=1e-12)
    np.testing.assert_allclose(Q['mu'].u[0], o.mu, rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(Q['Lambda'].u[0], o.Lam, rtol=1e-7,
                               atol=1e-10 + 1e-11 * np.abs(o.Lam).max())
    np.testing.assert_allclose(Q['Lambda'].u[1], o.logdetLam, rtol=1e-9)
    np.testing.assert_allclose(Q['alpha'].u[0], o.logpi, rtol=1e-9)
    fn = str(tmp_path / 'gmm_hd.ckpt')
    Q.save(filename=fn)
    Q.update(repeat=1, verbose=False)
    Q2 = _build(y, lab0, K, 'fused+dims')
    Q2.load(filename=fn)
    Q2.update(repeat=1, verbose=False)
    assert Q2.L[iters] == Q.L[iters]
