"""GPU: the fused hidden-Markov-model block on the real library -- the fixtures of
tests/golden/hmm_fused.npz and hmm.rst's known answer through engine='fused', and
``vmp_hmm_fused_pass`` alone against the long-double restatement of the reference arithmetic
(tests/hmm_fused_host.py ``restate``) at the smallest shapes that cross every lane bucket (KP = 2
... 64), D = 1 / 3 / 8, T = 2 / 3 / 65 and one, 64 / KP + 1 and enough chains for three workgroups
with a ragged last one; form (b) through the mixture block's update kernels; fixed labels, the prior pass, the optional outputs, repeatability, long
chains and transition tables far below the underflow of exp.

Measured on MI355X (float64 deviation of the reference formulas, error of the kernel, allowance;
worst over the shapes below): see DESIGN.md section 4.15."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu

SUMS = ('z0sum', 'xisum', 'T', 'logZ', 'ge')


def gpu_pass(Y, C, la0, lA, labels=None, want=False, mask=None):
    import torch
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.hmm import HMMKernels
    rt = get_runtime()
    k = HMMKernels(rt)
    B, T, D = Y.shape
    K = len(la0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(rt.device)  # noqa: E731
    _, wsd = k.plan(B, T, D, K)
    ws = rt.empty(int(wsd))
    z0sum, xisum, Ts, scal = rt.zeros(K), rt.zeros(K, K), rt.zeros(K, 1 + D + D * D), rt.zeros(8)
    g = rt.empty(B, T, K) if want else None
    z0 = rt.empty(B, K) if want else None
    zz = rt.empty(B, T - 1, K, K) if want else None
    lab = None if labels is None else torch.from_numpy(
        np.ascontiguousarray(labels, dtype=np.int32)).to(rt.device)
    md = None if mask is None else torch.from_numpy(
        np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)).to(rt.device)
    Cd = None if C is None else up(C)
    la0d, lAd = up(la0), up(lA)
    k.pass_(B, T, D, K, up(Y), Cd, 0 if C is None else C.shape[1], la0d, lAd, lab, ws, z0sum,
            xisum, Ts, scal, g, z0, zz, mask=md)
    rt.sync_stream()
    s = scal.cpu().numpy()
    out = dict(z0sum=z0sum.cpu().numpy(), xisum=xisum.cpu().numpy(), T=Ts.cpu().numpy(),
               logZ=float(s[0]), ge=float(s[1]), dots=s[2:4].copy())
    if want:
        out.update(gamma=g.cpu().numpy(), z0=z0.cpu().numpy(), zz=zz.cpu().numpy())
    return out


def _on_device(Q):
    assert type(Q.plans[0]).__name__ == 'HMMPlan'


def test_fixtures_through_the_library():
    from hmm_models import run_hmm_cases
    from test_hmm_fused_host import _mods, _golden, check_fixtures
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_hmm_cases(_mods(_on_device, engine='fused'), gin)
    check_fixtures(res, g)


def test_hmm_rst_known_answer():
    from test_hmm_fused_host import run_hmm_rst
    run_hmm_rst(_on_device)


def _shapes():
    out = []
    for K, D, T in ((1, 1, 2), (2, 3, 3), (3, 8, 65), (5, 3, 3), (16, 1, 3), (17, 3, 2), (33, 8, 3),
                    (64, 3, 65)):
        KP = 2
        while KP < K:
            KP *= 2
        G = 64 // KP
        out += [(B, T, D, K) for B in (1, G + 1, 2 * G + 1)]
    return out


@pytest.mark.parametrize('B,T,D,K', _shapes())
def test_pass_against_long_double(B, T, D, K):
    from hmm_fused_host import compare, hmmf_host
    from test_hmm_fused_host import pass_inputs
    Y, C, la0, lA = pass_inputs(B, T, D, K)
    if B > 2:
        assert hmmf_host().hmmf_wgs(B, T, D, K) in (2, 3)
    got = gpu_pass(Y, C, la0, lA, want=True)
    keys = SUMS + ('gamma', 'z0', 'zz')
    assert compare(got, Y, C, la0, lA, keys, label=str((B, T, D, K))) == []
    # the optional outputs off: the same bits; a second call: the same bits
    off, again = gpu_pass(Y, C, la0, lA), gpu_pass(Y, C, la0, lA)
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(off[k], got[k], err_msg=k)
        np.testing.assert_array_equal(again[k], off[k], err_msg=k)
    np.testing.assert_allclose(got['dots'], [np.sum(got['z0sum'] * la0), np.sum(got['xisum'] * lA)],
                               rtol=1e-12)


@pytest.mark.parametrize('B,T,D,K', [(5, 7, 2, 3), (3, 4, 8, 33)])
def test_prior_pass_and_labels(B, T, D, K):
    from hmm_fused_host import compare
    from test_hmm_fused_host import pass_inputs
    Y, C, la0, lA = pass_inputs(B, T, D, K)
    assert compare(gpu_pass(Y, None, la0, lA), Y, None, la0, lA, label='prior') == []
    lab = np.random.RandomState(1).randint(K, size=(B, T))
    r = gpu_pass(Y, C, la0, lA, labels=lab, want=True)
    onehot = np.eye(K)[lab]
    np.testing.assert_array_equal(r['gamma'], onehot)
    np.testing.assert_array_equal(r['z0'], onehot[:, 0])
    np.testing.assert_array_equal(r['zz'], onehot[:, :-1, :, None] * onehot[:, 1:, None, :])
    np.testing.assert_array_equal(r['z0sum'], onehot[:, 0].sum(0))
    np.testing.assert_array_equal(r['xisum'], np.einsum('bti,btj->ij', onehot[:, :-1], onehot[:, 1:]))
    np.testing.assert_allclose(r['T'][:, 1:1 + D], np.einsum('btk,btd->kd', onehot, Y), rtol=1e-13,
                               atol=1e-13)
    assert r['logZ'] == 0 and r['ge'] == 0
    off = gpu_pass(Y, C, la0, lA, labels=lab)
    for k in SUMS:
        np.testing.assert_array_equal(off[k], r[k])


def test_long_chain_with_separated_emissions():
    """T = 2000: log alpha reaches about -1e4 in a propagation without renormalisation."""
    from hmm_fused_host import compare
    from bayespy_amd.inference.plans.hmm import emission_tables
    rs = np.random.RandomState(7)
    K, D, T, B = 3, 2, 2000, 2
    mu = np.array([[0.0, 0.0], [30.0, 40.0], [60.0, 0.0]])
    C, _ = emission_tables(mu, np.identity(D))
    z = np.repeat(rs.randint(K, size=(B, T // 50)), 50, axis=1)
    Y = mu[z] + rs.normal(size=(B, T, D))
    la0, lA = np.log(np.full(K, 1.0 / K)), np.log(np.full((K, K), 0.1) + 0.7 * np.identity(K))
    got = gpu_pass(Y, C, la0, lA, want=True)
    assert got['logZ'] < -5e3 and np.all(np.isfinite(got['zz']))
    assert compare(got, Y, C, la0, lA, SUMS + ('gamma', 'zz'), label='T=2000') == []


def test_tables_below_the_underflow_of_exp():
    """Dirichlet(1e-3) rows: every <log A_ij> near -985 at K = 64 (exp of the table is 0: uniform xi
    is the answer), and one used row near 0 with the others near -670."""
    from scipy import special
    from hmm_fused_host import compare, restate
    from test_hmm_fused_host import pass_inputs
    from bayespy_amd.inference.plans.hmm import hmm_limits
    K = hmm_limits()[0]
    Y, _, _, _ = pass_inputs(2, 5, 2, K)
    al = np.full(K, 1e-3)
    la0 = special.digamma(al) - special.digamma(al.sum())
    lA = np.tile(la0, (K, 1))
    assert np.all(lA < -900) and np.all(np.exp(lA) == 0)
    got = gpu_pass(Y, None, la0, lA, want=True)
    np.testing.assert_allclose(got['zz'], 1.0 / K ** 2, rtol=1e-12)
    assert compare(got, Y, None, la0, lA, SUMS + ('zz',), label='flat') == []
    K = 3
    Y, C, _, _ = pass_inputs(3, 9, 2, K)
    alA = np.full((K, K), 1e-3)
    alA[1] += [40.0, 25.0, 10.0]
    lA = special.digamma(alA) - special.digamma(alA.sum(-1, keepdims=True))
    assert lA[1].max() > -2 and lA[0].max() < -600
    la0 = special.digamma(np.full(K, 1e-3)) - special.digamma(3e-3)
    got = gpu_pass(Y, C, la0, lA, want=True)
    assert np.all(np.isfinite(got['zz']))
    assert compare(got, Y, C, la0, lA, SUMS + ('gamma', 'zz'), label='one row') == []


def test_cabi_pass_checks_its_arguments_on_a_live_context():
    """Every refusal comes before a launch: null pointers, negative sizes, the limits, ldc."""
    import torch
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime, ptr
    rt = get_runtime()
    U, I = _lib.VMP_ERR_UNSUPPORTED, _lib.VMP_ERR_INVALID
    buf = rt.zeros(4096)
    p = ptr(buf)

    def call(B=4, T=3, D=2, K=3, C=p, ldc=6, a0=p, A=p, ws=p, z0sum=p, xisum=p, Ts=p, scal=p, Y=p):
        return rt.lib.vmp_hmm_fused_pass(rt.ctx, B, T, D, K, Y, C, ldc, a0, A, None, ws, z0sum,
                                         xisum, Ts, scal, None, None, None)
    for name in ('a0', 'A', 'ws', 'z0sum', 'xisum', 'Ts', 'scal', 'Y'):
        assert call(**{name: None}) == I, name
    for kw in (dict(B=-1), dict(T=1), dict(D=0), dict(K=0), dict(ldc=5)):
        assert call(**kw) == I, kw
    assert call(K=65) == U and call(D=9) == U
    assert call(B=0, Y=None) == _lib.VMP_OK            # no chains: zeros, Y is not read
    rt.sync_stream()
    assert not torch.any(buf[:64] != 0)


def test_edge_cases():
    from test_hmm_fused_host import pass_inputs
    Y, C, la0, lA = pass_inputs(4, 6, 2, 3)
    z = gpu_pass(Y[:0], C, la0, lA)
    assert not np.any(z['z0sum']) and not np.any(z['xisum']) and not np.any(z['T']) and z['logZ'] == 0
    la0[1] = -np.inf
    lA[:, 1] = -np.inf
    r = gpu_pass(Y, C, la0, lA, want=True)
    assert np.all(r['gamma'][..., 1] == 0) and np.all(r['zz'][..., 1] == 0)
    np.testing.assert_allclose(r['gamma'].sum(-1), 1.0, rtol=1e-13)
    r = gpu_pass(Y, C, la0, np.full((3, 3), -np.inf), want=True)
    assert np.all(np.isnan(r['zz'])) and np.isnan(r['logZ'])


def test_gamma_alone_and_pass_on_a_gmm_layout_table():
    """gamma and z0 without zz (the view of Z that Y asks for), and C read in place from a
    vmp_gmm_layout state (row stride F2P > NF, padded rows) as form (b) passes it."""
    import ctypes
    import torch
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.hmm import HMMKernels
    from test_hmm_fused_host import pass_inputs
    B, T, D, K = 5, 6, 3, 5
    Y, C, la0, lA = pass_inputs(B, T, D, K)
    ref = gpu_pass(Y, C, la0, lA, want=True)
    rt = get_runtime()
    k = HMMKernels(rt)
    L = _lib.GMMLayout()
    _lib.raise_for_status(rt.lib.vmp_gmm_get_layout(D, K, ctypes.byref(L)))
    F2P, KP = int(L.F2P), int(L.KP)
    assert F2P > C.shape[1] and KP > K
    wide = np.zeros((KP, F2P))
    wide[:K, :C.shape[1]] = C
    wide[K:, C.shape[1] - 1] = -np.inf
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(rt.device)  # noqa: E731
    ws = rt.empty(int(k.plan(B, T, D, K)[1]))
    z0sum, xisum, Ts, scal = rt.zeros(K), rt.zeros(K, K), rt.zeros(K, 1 + D + D * D), rt.zeros(8)
    g, z0 = rt.empty(B, T, K), rt.empty(B, K)
    k.pass_(B, T, D, K, up(Y), up(wide), F2P, up(la0), up(lA), None, ws, z0sum, xisum, Ts, scal,
            g, z0, None)
    rt.sync_stream()
    np.testing.assert_array_equal(g.cpu().numpy(), ref['gamma'])
    np.testing.assert_array_equal(z0.cpu().numpy(), ref['z0'])
    np.testing.assert_array_equal(Ts.cpu().numpy(), ref['T'])
    np.testing.assert_array_equal(xisum.cpu().numpy(), ref['xisum'])
