"""CPU only: the restatements of tests/gmm_pass_host.py (the yardstick of tests/test_gmm_pass_gpu.py)
against oracle/gmm.py -- the pass after one z half-step, the node updates and the five bound
terms after one full iteration --, the allowances they give, and the edge inputs."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gmm_pass_host as H                                           # noqa: E402

SHAPES = [(120, 3, 4), (397, 8, 17), (350, 17, 5)]
LD, F64 = np.longdouble, np.float64


def _layout_sizes(D, K):
    """(KP, F2P) as vmp_gmm_get_layout rounds them (no library on this side)."""
    kp = 16
    while kp < K:
        kp *= 2
    unit = 64 if D > 16 else 16
    return kp, (H.n_features(D) + unit - 1) // unit * unit


def _oracle(N, D, K):
    from oracle.gmm import GMMOracle
    g = H.make_inputs(N, D, K)
    lab0 = np.random.RandomState(N + D + K).randint(K, size=N)
    o = GMMOracle(g['y'], lab0, K, alpha0=g['alpha0'], beta0=g['beta0'], n0=g['n0'], V0=g['V0'])
    return g, lab0, o


def _chain(g, lab0, D, K, dtype):
    """One VB iteration (mu, Lambda, z, alpha, the bound) from the labelled start, restated."""
    KP, F2P = _layout_sizes(D, K)
    s = H.restate_init(g['alpha0'], g['beta0'], g['n0'], g['V0'], dtype)
    p0 = H.restate_pass(g['y'], np.zeros((K, F2P)), labels=lab0, dtype=dtype)
    s.update(H.restate_update_mu(p0['R'], p0['S1'], s['Lam'], g['beta0'], dtype))
    s.update(H.restate_update_lambda(p0['R'], p0['S1'], p0['S2'], s['mu'], s['Cmu'], g['n0'],
                                     g['V0'], dtype))
    C = H.restate_C(s['Lam'], s['mu'], s['Cmu'], s['logdetLam'], s['logpi'], KP, F2P, dtype=dtype)
    p = H.restate_pass(g['y'], C[:K], dtype=dtype)
    s.update({k: p[k] for k in H.PASS_QUANTITIES + ('rphi_mag',)})
    s.update(H.restate_update_alpha(g['alpha0'], p['R'], dtype))
    s.update(alpha0=g['alpha0'], beta0=g['beta0'], n0=g['n0'], V0=g['V0'], C=C)
    s.update(H.restate_lower_bound(s, dtype))
    return s


def test_feature_list_and_the_inverse():
    D = 5
    y = np.random.RandomState(0).normal(size=(3, D))
    f = H.features(y, 32, F64)
    assert H.n_features(D) == 21
    want = [y[0, a] * y[0, b] for a in range(D) for b in range(a, D)] + list(y[0]) + [1.0]
    np.testing.assert_array_equal(f[0, :21], want)
    assert not f[:, 21:].any()
    A = np.stack([H.spd(np.random.RandomState(k), 6, 1e3) for k in range(3)])
    inv, ld = H.spd_inverse(A, LD)
    np.testing.assert_allclose(inv.astype(F64), np.linalg.inv(A), rtol=1e-10)
    np.testing.assert_allclose(ld.astype(F64), np.linalg.slogdet(A)[1], rtol=1e-13)
    bad, ldb = H.spd_inverse(-A[:1], F64)
    assert np.isnan(ldb[0])


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_pass_restatement_reproduces_the_oracle_after_one_z_half_step(N, D, K):
    g, lab0, o = _oracle(N, D, K)
    KP, F2P = _layout_sizes(D, K)
    o.update_mu()
    o.update_Lambda()
    c, b = o._coefficients()
    args = (o.Lam, o.mu, o.Cmu, o.logdetLam, o.logpi, KP, F2P)
    C_ld, C = H.restate_C(*args), H.restate_C(*args, dtype=F64)
    npair = H.n_pairs(D)
    cols = dict(lin=slice(npair, npair + D), const=slice(npair + D, npair + D + 1))
    ctol, _ = H.tolerances({k: C_ld[:K, s] for k, s in cols.items()},
                           {k: C[:K, s] for k, s in cols.items()}, tuple(cols))
    assert H.error(b, C_ld[:K, cols['lin']]) <= ctol['lin']
    assert H.error((o.logpi + c)[:, None], C_ld[:K, cols['const']]) <= ctol['const']
    assert np.all(np.isneginf(C[K:, npair + D])) and not C[K:, :npair + D].any()
    assert not C[:, npair + D + 1:].any()
    # the oracle's own coefficients in the restatement's layout
    C[:K, cols['lin']], C[:K, npair + D] = b, o.logpi + c
    o.update_z()
    ld, f64 = H.restate_pass(g['y'], C[:K]), H.restate_pass(g['y'], C[:K], dtype=F64)
    tol, dev = H.pass_tolerances(ld, f64)
    got = dict(r=o.r, R=o.R, S1=o.S1, S2=o.S2, sum_lse=o.sum_lse, rphi=o.sum_rphi)
    for key in H.PASS_QUANTITIES:
        err = H.error(got[key], ld[key])
        print('%s %s: float64 deviation %.3g, oracle %.3g, allowed %.3g'
              % (key, (N, D, K), dev[key], err, tol[key]))
        assert err <= tol[key], (key, err, tol[key])


@pytest.mark.parametrize('N,D,K', SHAPES + [(300, 32, 64)])
def test_allowances_are_measured_not_the_floor(N, D, K):
    g = H.make_inputs(N, D, K)
    KP, F2P = _layout_sizes(D, K)
    C = H.restate_C(g['Lam'], g['mu'], g['Cmu'], g['logdetLam'], g['logpi'], KP, F2P, dtype=F64)
    ld, f64 = H.restate_pass(g['y'], C[:K]), H.restate_pass(g['y'], C[:K], dtype=F64)
    tol, dev = H.pass_tolerances(ld, f64)
    floor = {k: 4 * float(np.spacing(float(np.max(np.abs(ld[k]))))) for k in H.PASS_QUANTITIES}
    assert all(tol[k] > 0 for k in H.PASS_QUANTITIES)
    assert all(dev[k] > 0 for k in H.PASS_QUANTITIES), dev
    assert any(tol[k] > floor[k] for k in H.PASS_QUANTITIES), (tol, floor)
    assert np.median(f64['r'].max(axis=1)) < 0.999


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_update_restatements_reproduce_the_oracle_after_one_iteration(N, D, K):
    g, lab0, o = _oracle(N, D, K)
    o.iterate(1)
    ld, f64 = _chain(g, lab0, D, K, LD), _chain(g, lab0, D, K, F64)
    got = dict(mu=o.mu, Cmu=o.Cmu, logdetLmu=o.logdet_Lmu, nk=o.nk, Vk=o.Vk, Lam=o.Lam,
               logdetV=o.logdetV, logdetLam=o.logdetLam, alpha=o.alpha, logpi=o.logpi,
               L_Y=o.L_terms[0]['Y'], L_z=o.L_terms[0]['z'], L_alpha=o.L_terms[0]['alpha'],
               L_mu=o.L_terms[0]['mu'], L_Lambda=o.L_terms[0]['Lambda'], L=o.L[0])
    tol, dev = H.tolerances(ld, f64, tuple(got))
    for key in got:
        err = H.error(got[key], ld[key])
        print('%s %s: float64 deviation %.3g, oracle %.3g, allowed %.3g'
              % (key, (N, D, K), dev[key], err, tol[key]))
        assert err <= tol[key], (key, err, tol[key])


@pytest.mark.parametrize('D,K', H.EDGE_SHAPES)
def test_edge_inputs_stay_nan_free_in_the_reference_recipe(D, K):
    KP, F2P = _layout_sizes(D, K)
    y, C = H.edge_inputs(D, K, KP, F2P)
    for dtype in (F64, LD):
        p = H.restate_pass(y, C[:K], dtype=dtype)
        assert not np.isnan(p['r']).any()
        assert np.isfinite(p['T']).all() and np.isfinite(p['rphi']) and np.isfinite(p['sum_lse'])
        assert not p['r'][:, H.EDGE_DEAD].any() and not p['T'][H.EDGE_DEAD].any()
        a, b = H.EDGE_TWINS
        np.testing.assert_array_equal(p['r'][:, a], p['r'][:, b])
    ld = H.restate_pass(y, C[:K])
    phi = H.features(y, F2P)[H.EDGE_FAR_ROW] @ np.asarray(C[:K], dtype=LD).T
    live = np.isfinite(phi)
    assert phi[live].max() - phi[live].min() > 800
    lost = phi - phi[live].max() < -801
    assert lost.sum() >= 2 and not H.restate_pass(y, C[:K], dtype=F64)['r'][H.EDGE_FAR_ROW, lost].any()
    assert float(ld['r'][H.EDGE_FAR_ROW].sum()) == pytest.approx(1.0, abs=1e-15)
    np.testing.assert_array_equal(y[H.EDGE_ZERO_ROW], 0.0)


def test_lgamma_of_a_sum_keeps_its_rounding_errors():
    """vmp_lgamma_dd (csrc/vmp_common.h, the ln Gamma(sum alpha) of the bound's alpha term), compiled
    for the host: value + lo against 40-digit ln Gamma(x + dx).  Bound from its arithmetic: the
    logarithm is taken of a number below sqrt 2, so it is off by at most an ulp of 0.35 (5.6e-17)
    and half an ulp for the sum it enters; times x - 1/2 and against ln Gamma >= x (log x - 1)
    that is below half an ulp of the value at every x >= 10.  lo is the error of a rounded sum:
    at most half an ulp of the value."""
    import ctypes
    import subprocess
    import tempfile
    from host_build import special_functions_text
    with tempfile.TemporaryDirectory() as d:
        cpp, so = os.path.join(d, 'lg.cpp'), os.path.join(d, 'lg.so')
        with open(cpp, 'w') as f:
            f.write(special_functions_text())
            f.write('extern "C" void lg(const double *x, const double *dx, double *hi, double *lo,'
                    ' int n)\n{ for (int i = 0; i < n; i++) hi[i] = vmp_lgamma_dd(x[i], dx[i], lo + i); }\n')
        subprocess.check_call(['g++', '-O2', '-shared', '-fPIC', cpp, '-o', so])
        lib = ctypes.CDLL(so)
    rs = np.random.RandomState(5)
    x = np.concatenate([np.logspace(1, 15, 1501), np.linspace(10.0, 500.0, 1001),
                        [10.0, 16.0, 363.7, 2.0 ** 40]])
    dx = np.spacing(x) * rs.uniform(-0.5, 0.5, size=len(x))
    hi, lo = np.empty_like(x), np.empty_like(x)
    lib.lg(*(a.ctypes.data_as(ctypes.c_void_p) for a in (x, dx, hi, lo)), len(x))
    _, lgam = H._special(LD)
    ref = lgam(x.astype(LD) + dx.astype(LD))
    ulp = np.spacing(np.abs(ref.astype(F64)))
    err = np.abs((hi.astype(LD) + lo.astype(LD)) - ref).astype(F64) / ulp
    print('vmp_lgamma_dd: worst %.3f ulp at x = %.6g' % (err.max(), x[np.argmax(err)]))
    assert err.max() <= 0.5
    assert np.all(np.abs(lo) <= 0.5 * np.spacing(np.abs(hi)))
    # below 10 it is vmp_lgamma and the dx term
    xs = np.linspace(0.25, 9.75, 39)
    d0 = np.zeros_like(xs)
    h2, l2 = np.empty_like(xs), np.empty_like(xs)
    lib.lg(*(a.ctypes.data_as(ctypes.c_void_p) for a in (xs, d0, h2, l2)), len(xs))
    assert np.all(l2 == 0.0)
    assert np.max(np.abs(h2.astype(LD) - lgam(xs.astype(LD)))) < 2e-14
