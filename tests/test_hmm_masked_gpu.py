"""GPU: masks on the fused hidden-Markov-model block on the real library -- the fixtures of
tests/golden/hmm_masked.npz and the model of examples/hmm_ragged.py through engine='fused', and
``vmp_hmm_fused_pass_masked`` alone against the long-double restatement of the reference arithmetic
(tests/hmm_fused_host.py ``restate``) at the shapes of tests/test_hmm_fused_gpu.py with three
workgroups, the last one ragged, under one mask that mixes fully observed chains, chains with
nothing observed, masked first and last steps, ragged tails and holes; a mask of ones against the
unmasked entry, the values at masked positions, a mask of zeros, fixed labels, the optional outputs,
tables below the underflow of exp and the argument checks.

Measured on MI355X: see DESIGN.md section 4.15, "Masks"."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'examples'))

pytestmark = pytest.mark.gpu

SUMS = ('z0sum', 'xisum', 'T', 'logZ', 'ge')
OUTS = ('gamma', 'z0', 'zz')


def _on_device(Q):
    assert type(Q.plans[0]).__name__ == 'HMMPlan'


def test_fixtures_through_the_library():
    from hmm_models import run_hmm_cases
    from test_hmm_masked_host import _mods, _golden, check_masked_fixtures
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_hmm_cases(_mods(_on_device, engine='fused'), gin)
    check_masked_fixtures(res, g)


def test_fixtures_with_masks_in_device_memory():
    import torch
    from hmm_models import run_hmm_cases
    from test_hmm_masked_host import _mods, _golden, L_RTOL
    g, gin = _golden()
    res = run_hmm_cases(_mods(_on_device, engine='fused'), gin, only=('b', 'f'),
                           device_mask=lambda m: torch.from_numpy(np.ascontiguousarray(m)).cuda())
    for tag in 'bf':
        np.testing.assert_allclose(res[tag + '_L'], g[tag + '_L'], rtol=L_RTOL)
        np.testing.assert_array_equal(res[tag + '_Z_mask'], g[tag + '_Z_mask'])


def test_ragged_example_at_toy_size():
    """examples/hmm_ragged.py's model: the bound rises and agrees with the kernel double's."""
    import hmm_ragged
    from test_hmm_masked_host import _on_double, L_RTOL
    y, mask, lengths = hmm_ragged.simulate(37, 11, np.random.RandomState(3))
    assert np.all(np.isnan(y[~mask])) and lengths.min() < 11
    Q, n = hmm_ragged.build(y, mask)
    _on_device(Q)
    Q.update(repeat=5, verbose=False)
    L = Q.L[:5].copy()
    assert np.all(np.isfinite(L)) and np.all(np.diff(L) > -1e-6 * np.abs(L[:-1]))
    np.testing.assert_array_equal(n['Z'].mask, mask.any(axis=1))
    Q2, _ = hmm_ragged.build(y, mask)
    _on_double(Q2)
    Q2.update(repeat=5, verbose=False)
    np.testing.assert_allclose(L, Q2.L[:5], rtol=L_RTOL)


def _shapes():
    from bayespy_amd.inference.plans.hmm import hmm_limits
    out = []
    for K, D, T in ((1, 1, 2), (2, 3, 3), (3, 8, 65), (5, 3, 3), (17, 3, 2), (33, 8, 3), (64, 3, 65)):
        K = min(K, hmm_limits()[0])
        KP = 2
        while KP < K:
            KP *= 2
        out.append((2 * (64 // KP) + 1, T, D, K))
    return out


@pytest.mark.parametrize('B,T,D,K', _shapes())
def test_masked_pass_against_long_double(B, T, D, K):
    from hmm_fused_host import hmmf_host, compare, mixed_mask, nan_fill
    from test_hmm_fused_gpu import gpu_pass
    from test_hmm_fused_host import pass_inputs
    Y, C, la0, lA = pass_inputs(B, T, D, K)
    assert hmmf_host().hmmf_wgs(B, T, D, K) == 3
    mask = mixed_mask(B, T, np.random.RandomState(B + T))
    ob = mask.any(axis=1)
    assert ob.sum() >= 2 and (~ob).sum() >= 1
    Yn = nan_fill(Y, mask)
    got = gpu_pass(Yn, C, la0, lA, want=True, mask=mask)
    assert compare(got, Yn, C, la0, lA, SUMS + OUTS, label=str((B, T, D, K)), mask=mask) == []
    # the optional outputs off, a second call, 0 and 1e300 at the masked positions: the same bits
    off, again = gpu_pass(Yn, C, la0, lA, mask=mask), gpu_pass(Yn, C, la0, lA, mask=mask)
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(off[k], got[k], err_msg=k)
        np.testing.assert_array_equal(again[k], off[k], err_msg=k)
    for fill in (0.0, 1e300):
        alt = gpu_pass(nan_fill(Y, mask, fill), C, la0, lA, want=True, mask=mask)
        for k in SUMS + ('dots',) + OUTS:
            np.testing.assert_array_equal(alt[k], got[k], err_msg='%s, fill %g' % (k, fill))
    # a mask of ones: the bits of vmp_hmm_fused_pass, sums and optional outputs
    ref = gpu_pass(Y, C, la0, lA, want=True)
    one = gpu_pass(Y, C, la0, lA, want=True, mask=np.ones((B, T), dtype=bool))
    for k in SUMS + ('dots',) + OUTS:
        np.testing.assert_array_equal(one[k], ref[k], err_msg=k)
    # a mask of zeros: nothing
    z = gpu_pass(Yn, C, la0, lA, mask=np.zeros((B, T), dtype=bool))
    for k in ('z0sum', 'xisum', 'T'):
        assert np.all(z[k] == 0), k
    assert z['logZ'] == 0 and z['ge'] == 0


@pytest.mark.parametrize('B,T,D,K', [(13, 7, 2, 3), (7, 4, 8, 33)])
def test_fixed_labels_with_a_mask(B, T, D, K):
    from hmm_fused_host import mixed_mask, nan_fill
    from test_hmm_fused_gpu import gpu_pass
    from test_hmm_fused_host import pass_inputs
    from test_hmm_masked_host import check_labels
    Y, C, la0, lA = pass_inputs(B, T, D, K)
    mask = mixed_mask(B, T, np.random.RandomState(5))
    lab = np.random.RandomState(1).randint(K, size=(B, T))
    r = gpu_pass(nan_fill(Y, mask), C, la0, lA, labels=lab, want=True, mask=mask)
    check_labels(r, lab, Y, mask, K)
    off = gpu_pass(nan_fill(Y, mask), C, la0, lA, labels=lab, mask=mask)
    for k in SUMS:
        np.testing.assert_array_equal(off[k], r[k])


def test_tables_below_the_underflow_of_exp_with_a_mask():
    """One used row of <log A> near 0, the others near -670 (Dirichlet(1e-3) rows)."""
    from scipy import special
    from hmm_fused_host import compare, mixed_mask, nan_fill
    from test_hmm_fused_gpu import gpu_pass
    from test_hmm_fused_host import pass_inputs
    K = 3
    Y, C, _, _ = pass_inputs(7, 9, 2, K)
    alA = np.full((K, K), 1e-3)
    alA[1] += [40.0, 25.0, 10.0]
    lA = special.digamma(alA) - special.digamma(alA.sum(-1, keepdims=True))
    assert lA[1].max() > -2 and lA[0].max() < -600
    la0 = special.digamma(np.full(K, 1e-3)) - special.digamma(3e-3)
    mask = mixed_mask(7, 9, np.random.RandomState(2))
    Yn = nan_fill(Y, mask)
    got = gpu_pass(Yn, C, la0, lA, want=True, mask=mask)
    assert np.all(np.isfinite(got['zz']))
    assert compare(got, Yn, C, la0, lA, SUMS + ('gamma', 'zz'), label='one row', mask=mask) == []


def test_cabi_masked_pass_checks_its_arguments_on_a_live_context():
    """Every refusal comes before a launch: null pointers, negative sizes, the limits, ldc."""
    import torch
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime, ptr
    rt = get_runtime()
    U, I = _lib.VMP_ERR_UNSUPPORTED, _lib.VMP_ERR_INVALID
    buf = rt.zeros(4096)
    p = ptr(buf)
    mk = ptr(torch.ones(64, dtype=torch.uint8, device=rt.device))

    def call(B=4, T=3, D=2, K=3, C=p, ldc=6, a0=p, A=p, ws=p, z0sum=p, xisum=p, Ts=p, scal=p, Y=p):
        return rt.lib.vmp_hmm_fused_pass_masked(rt.ctx, B, T, D, K, Y, C, ldc, a0, A, None, mk, ws,
                                                z0sum, xisum, Ts, scal, None, None, None)
    for name in ('a0', 'A', 'ws', 'z0sum', 'xisum', 'Ts', 'scal', 'Y'):
        assert call(**{name: None}) == I, name
    for kw in (dict(B=-1), dict(T=1), dict(D=0), dict(K=0), dict(ldc=5)):
        assert call(**kw) == I, kw
    assert call(K=65) == U and call(D=9) == U
    assert call(B=0, Y=None) == _lib.VMP_OK            # no chains: zeros, Y and the mask not read
    rt.sync_stream()
    assert not torch.any(buf[:64] != 0)
