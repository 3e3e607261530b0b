"""CPU: the yardstick of the generic forward-backward kernel (tests/alpha_beta_host.py) -- the
restatement against the live-reference fixtures and oracle/hmm.py, the generators of the regimes
and the preconditions that make them regimes, the sparse-table counter-example of a shift by the
joint maximum of a slice, and the NumPy double of the entry point (tests/host_generic.py)."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from alpha_beta_host import (EXP_UNDERFLOW, INF_KINDS, KEYS, SPARSE, SPARSE_G, allowances,  # noqa: E402
                             compare, emulate_joint_shift, inputs, restate)

# kind -> (B, N, K): the shapes the GPU tests use as well
SHAPES = {'random': (5, 7, 5), 'inf_p0': (9, 4, 3), 'inf_col': (9, 4, 3), 'inf_row': (9, 4, 3),
          'left_to_right': (9, 4, 3), 'sparse': (17, 3, 3), 'dirichlet_tiny': (2, 3, 64),
          'one_row': (17, 8, 3), 'long': (2, 2000, 3)}


@pytest.fixture(scope='module', params=sorted(SHAPES))
def regime(request):
    kind = request.param
    logp0, logP = inputs(kind, *SHAPES[kind], seed=3)
    return kind, logp0, logP, restate(logp0, logP, full=True)


def test_restatement_against_the_reference_fixtures(golden_dir):
    f = np.load(os.path.join(golden_dir, 'markov_chains.npz'))
    for tag in ('ab_a', 'ab_b', 'ab_c', 'ab_d', 'ab_e', 'ab_f'):
        z0, zz, g = restate(f[tag + '_logp0'], f[tag + '_logP'], np.float64)
        assert z0.dtype == zz.dtype == g.dtype == np.float64
        np.testing.assert_allclose(g, f[tag + '_g'], rtol=1e-12, atol=1e-12, err_msg=tag)
        np.testing.assert_allclose(z0, f[tag + '_z0'], rtol=1e-10, atol=1e-15, err_msg=tag)
        np.testing.assert_allclose(zz, f[tag + '_zz'], rtol=1e-10, atol=1e-15, err_msg=tag)
        assert compare(dict(zip(KEYS, (f[tag + '_z0'], f[tag + '_zz'], f[tag + '_g']))),
                       f[tag + '_logp0'], f[tag + '_logP'], label=tag) == []


def test_restatement_against_the_oracle_and_finite(regime):
    from oracle import hmm
    kind, logp0, logP, (z0, zz, g, la, lb) = regime
    assert z0.dtype == np.longdouble
    for a in (z0, zz, g):
        assert np.all(np.isfinite(a)), kind
    got = dict(zip(KEYS, hmm.alpha_beta_recursion(logp0, logP)))
    assert compare(got, logp0, logP, label='oracle ' + kind) == []
    f64 = dict(zip(KEYS, restate(logp0, logP, np.float64)))
    for k in KEYS:
        assert np.all(np.isfinite(f64[k])), (kind, k)
    np.testing.assert_allclose(np.sum(zz, axis=(-1, -2)).astype(float), 1.0, rtol=1e-15)


def test_preconditions_of_the_regimes(regime):
    kind, logp0, logP, (z0, zz, g, la, lb) = regime
    B, N, K = SHAPES[kind]
    if kind in INF_KINDS:
        assert np.all(np.isfinite(g))                        # every chain keeps a possible path
        assert np.all(np.any(zz.reshape(B, -1) == 0, axis=1))
        assert np.any(np.isinf(logp0)) or np.any(np.isinf(logP))
    elif kind == 'sparse':
        for b in range(B):
            i = int(np.argmax(la[b, 1]))                     # the best state of instance 1 ...
            v = la[b, 0][:, None] + logP[b, 0]               # the slice that forms logalpha_1
            r, c = np.unravel_index(int(np.argmax(zz[b, 1])), (K, K))
            assert r != i                                    # ... is not on the dominant path,
            assert la[b, 1, r] < la[b, 1, i] - EXP_UNDERFLOW   # whose state lies below underflow:
            assert np.max(v[:, r]) < np.max(v) - EXP_UNDERFLOW   # its whole column of that slice
            assert zz[b, 1, r, c] > 1 - 1e-9
        assert int(np.argmax(zz[0, 1])) == 1 * K + 2
    elif kind == 'dirichlet_tiny':
        assert np.max(logp0) < -900 and np.max(logP) < -900
        np.testing.assert_allclose(zz.astype(float), 1.0 / K ** 2, rtol=1e-15)
    elif kind == 'one_row':
        assert np.all(logP[:, :, 0] > -40) and np.all(logP[:, :, 1:] < -600)
        assert np.all(logP > -EXP_UNDERFLOW) and np.any(logP < -708)   # below the normal range
        rows = np.argmax(np.sum(zz[:, 0], axis=-1), axis=-1)
        assert np.all(rows[1::2] == 1) and np.all(rows[0::2] == 0)
    elif kind == 'long':
        assert np.all(np.abs(g) > 5e3)


def test_sparse_table_case_and_the_joint_shift():
    """The counter-example: with one shift for the whole slice the state that carries the only
    cheap route underflows; the per-axis log-sum-exp of the reference keeps it."""
    from oracle import hmm
    logp0, logP = SPARSE
    o0, ozz, og = hmm.alpha_beta_recursion(logp0, logP)
    assert abs(float(og) - SPARSE_G) < 5e-3
    for dtype in (np.longdouble, np.float64):
        z0, zz, g = restate(logp0, logP, dtype)
        np.testing.assert_allclose(np.asarray(g, dtype=float), og, rtol=1e-13)
        np.testing.assert_allclose(np.asarray(zz, dtype=float), ozz, rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(np.asarray(z0, dtype=float), o0, rtol=1e-10, atol=1e-15)
    assert ozz[1, 1, 2] > 1 - 1e-9
    e0, ezz, eg = emulate_joint_shift(logp0, logP)
    assert abs(eg - 903.75) < 5e-3 and ezz[1, 0, 1] > 1 - 1e-9
    assert np.max(np.abs(ezz - ozz)) > 0.999
    bad = compare(dict(z0=e0, zz=ezz, g=eg), logp0, logP, label='joint shift')
    assert {k for k, _, _ in bad} >= {'zz', 'g'}             # the rule sees it
    # on well-scaled tables the two are the same function
    p0, P = inputs('random', 1, 7, 5, seed=1)
    assert compare(dict(zip(KEYS, emulate_joint_shift(p0[0], P[0]))), p0[0], P[0],
                   label='joint shift, random') == []


def _double(logp0, p0_bs, logP, P_bs, P_ts, B, N, K, ws_bytes=None):
    from host_generic import HostGenericLib
    p = lambda a: ctypes.c_void_p(a.ctypes.data)                    # noqa: E731
    z0, zz, g = np.full((B, K), np.nan), np.full((B, N, K, K), np.nan), np.full(B, np.nan)
    ws = np.empty(max(B * N * K, 1))
    rc = HostGenericLib().vmp_alpha_beta_recursion(
        None, N, K, B, p(logp0), p0_bs, p(logP), P_bs, P_ts, p(z0), p(zz), p(g), p(ws),
        B * N * K * 8 if ws_bytes is None else ws_bytes)
    return rc, dict(z0=z0, zz=zz, g=g)


def test_double_of_the_entry_point(regime):
    kind, logp0, logP, _ = regime
    B, N, K = SHAPES[kind]
    rc, got = _double(np.ascontiguousarray(logp0), K, np.ascontiguousarray(logP), N * K * K, K * K,
                      B, N, K)
    assert rc == 0
    assert compare(got, logp0, logP, label='double ' + kind) == []


@pytest.mark.parametrize('p0_shared', [False, True])
@pytest.mark.parametrize('form', ['dense', 'shared_b', 'shared_bt', 'shared_t'])
def test_double_stride_forms(form, p0_shared):
    B, N, K = 3, 4, 5
    logp0, logP = inputs('random', B, N, K, seed=5)
    p0 = logp0[:1] if p0_shared else logp0
    P, P_bs, P_ts = {'dense': (logP, N * K * K, K * K), 'shared_b': (logP[:1], 0, K * K),
                     'shared_bt': (logP[:1, :1], 0, 0), 'shared_t': (logP[:, :1], K * K, 0)}[form]
    rc, got = _double(np.ascontiguousarray(p0), 0 if p0_shared else K, np.ascontiguousarray(P),
                      P_bs, P_ts, B, N, K)
    assert rc == 0
    assert compare(got, np.broadcast_to(p0, (B, K)), np.broadcast_to(P, (B, N, K, K)),
                   label=form) == []


def test_double_status_codes():
    from bayespy_amd import _lib
    logp0, logP = inputs('random', 2, 2, 3, seed=0)
    assert _double(logp0, 3, logP, 18, 9, 2, 2, 3, ws_bytes=2 * 2 * 3 * 8 - 8)[0] == _lib.VMP_ERR_INVALID
    rc, got = _double(logp0, 3, logP, 18, 9, 0, 2, 3)
    assert rc == _lib.VMP_OK and np.all(np.isnan(got['zz']))
    big = np.zeros(65 * 65)
    assert _double(big, 65, big, 0, 0, 1, 1, 65)[0] == _lib.VMP_ERR_UNSUPPORTED


def test_allowance_has_its_floor():
    """K = 1: every evaluation is exact, the allowance is 4 ulp of the magnitude."""
    logp0, logP = inputs('random', 2, 3, 1, seed=0)
    a = allowances(logp0, logP)
    assert a['zz'][1] == 0 and a['zz'][2] == 4 * np.spacing(1.0)
    assert a['g'][2] >= 4 * np.spacing(float(np.max(np.abs(a['g'][0]))))
