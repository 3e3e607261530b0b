"""GPU: the wide-emission pass of the fused hidden-Markov-model block -- ``vmp_hmm_wide_pass`` alone
against the long-double restatement of the reference arithmetic (tests/hmm_fused_host.py
``restate`` / ``compare``: the allowance rule of DESIGN.md section 4.15; at D = 32 sum log Z and
sum gamma . e also get the feature-sum allowance of ``check`` below, derived the same way -- worst
measured on MI355X: error 7.6e-13 against 6.6e-13 of the rule alone and 2.3e-11 with it, section
4.15b), its masked twin, fixed labels and the
prior pass, agreement with the narrow pass at D <= 8, and the model of hmm.rst at D = 12 through
engine='fused+emissions' against the live-reference fixture tests/golden/hmm_wide.npz and
engine='generic'."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu

SUMS = ('z0sum', 'xisum', 'T', 'logZ', 'ge')
ALL = SUMS + ('gamma', 'z0', 'zz')
L_RTOL = 1e-9                               # tests/test_hmm_fused_host.py
MOM_TOL = dict(rtol=1e-6, atol=1e-9)


def wide_pass(Y, C, la0, lA, labels=None, want=False, mask=None, narrow=False):
    """tests/test_hmm_fused_gpu.py ``gpu_pass`` on the kernels of the wide form."""
    import test_hmm_fused_gpu as narrow_gpu
    from bayespy_amd.inference.plans import hmm, hmm_wide
    if narrow:
        return narrow_gpu.gpu_pass(Y, C, la0, lA, labels, want, mask)
    keep = hmm.HMMKernels
    hmm.HMMKernels = hmm_wide.WideHMMKernels
    try:
        return narrow_gpu.gpu_pass(Y, C, la0, lA, labels, want, mask)
    finally:
        hmm.HMMKernels = keep


def _inputs(B, T, D, K):
    from test_hmm_fused_host import pass_inputs
    return pass_inputs(B, T, D, K)


def check(got, Y, C, la0, lA, keys=SUMS, label='', mask=None):
    """``compare`` unchanged, plus the allowance of DESIGN.md section 4.15b for the two sums that
    are linear in e.  ``restate`` evaluates e = sum_f C_f phi_f once in float64, through a BLAS
    product whose order of additions is not the reference's to choose; with few rows its deviation
    from long double is one sample of a quantity that depends on that order.  The same rule is
    therefore applied to the other float64 evaluation of the same formula, the ascending sum of
    the narrow pass: d_row = max_k |e64_row,k - e_long_row,k|, and since sum log Z and
    sum gamma . e move by at most sum_rows d_row when every e moves by d_row, they are allowed
    max(the rule's allowance, 8 sum_observed_rows d_row).  Nothing here looks at the kernel."""
    from hmm_fused_host import compare, features
    bad = compare(got, Y, C, la0, lA, keys, label=label, mask=mask)
    if bad and C is not None:
        obs = np.ones(Y.shape[:2], bool) if mask is None else np.asarray(mask) != 0
        Yz = np.where(obs[..., None], Y, 0.0)
        e64 = np.cumsum(features(Yz, np.float64)[..., None, :] * C, axis=-1)[..., -1]
        eld = features(Yz, np.longdouble) @ np.asarray(C, dtype=np.longdouble).T
        extra = 8 * float(np.sum(np.max(np.abs(e64 - eld), axis=-1)[obs]))
        print('%s feature sums: allowance for logZ and ge %.3e' % (label, extra))
        bad = [b for b in bad if not (b[0] in ('logZ', 'ge') and b[1] <= extra)]
    return bad


KDT = ((1, 9, 2), (3, 16, 3), (5, 17, 65), (17, 9, 3), (33, 32, 2), (64, 32, 3), (3, 3, 3))


def _shapes(kdt):
    out = []
    for K, D, T in kdt:
        G = 64 // max(2, 1 << (K - 1).bit_length())
        out += [(B, T, D, K) for B in (1, G + 1, 2 * G + 1)]
    return out


@pytest.mark.parametrize('B,T,D,K', _shapes(KDT))
def test_pass_against_long_double(B, T, D, K):
    Y, C, la0, lA = _inputs(B, T, D, K)
    got = wide_pass(Y, C, la0, lA, want=True)
    assert check(got, Y, C, la0, lA, ALL, label=str((B, T, D, K))) == []
    # the optional outputs off: the same bits; a second call: the same bits
    off, again = wide_pass(Y, C, la0, lA), wide_pass(Y, C, la0, lA)
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(off[k], got[k], err_msg=k)
        np.testing.assert_array_equal(again[k], off[k], err_msg=k)


@pytest.mark.parametrize('B,T,D,K', [(5, 65, 17, 5), (9, 3, 9, 17), (3, 3, 32, 64)])
def test_masked_pass_against_long_double(B, T, D, K):
    from hmm_fused_host import nan_fill
    Y, C, la0, lA = _inputs(B, T, D, K)
    mask = np.random.RandomState(K).rand(B, T) < 0.6
    mask[0, 0], mask[B - 1] = True, False           # one chain fully hidden
    got = wide_pass(nan_fill(Y, mask), C, la0, lA, want=True, mask=mask)
    assert check(got, Y, C, la0, lA, ALL, label='masked ' + str((B, T, D, K)), mask=mask) == []
    ones, none = wide_pass(Y, C, la0, lA, mask=np.ones((B, T))), wide_pass(Y, C, la0, lA)
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(ones[k], none[k], err_msg=k)


@pytest.mark.parametrize('B,T,D,K', [(5, 7, 12, 3), (3, 4, 32, 33)])
def test_prior_pass_and_labels(B, T, D, K):
    from hmm_fused_host import compare
    Y, C, la0, lA = _inputs(B, T, D, K)
    assert compare(wide_pass(Y, None, la0, lA), Y, None, la0, lA, label='prior') == []
    lab = np.random.RandomState(1).randint(K, size=(B, T))
    r = wide_pass(Y, C, la0, lA, labels=lab, want=True)
    onehot = np.eye(K)[lab]
    np.testing.assert_array_equal(r['gamma'], onehot)
    np.testing.assert_array_equal(r['z0'], onehot[:, 0])
    np.testing.assert_array_equal(r['zz'], onehot[:, :-1, :, None] * onehot[:, 1:, None, :])
    np.testing.assert_array_equal(r['z0sum'], onehot[:, 0].sum(0))
    np.testing.assert_array_equal(r['xisum'], np.einsum('bti,btj->ij', onehot[:, :-1], onehot[:, 1:]))
    Yn = np.concatenate([np.ones((B, T, 1)), Y, (Y[..., :, None] * Y[..., None, :]).reshape(B, T, -1)], -1)
    np.testing.assert_allclose(r['T'], np.einsum('btk,btf->kf', onehot, Yn), rtol=1e-13, atol=1e-12)
    assert r['logZ'] == 0 and r['ge'] == 0


@pytest.mark.parametrize('B,T,D,K', [(5, 3, 3, 3), (3, 3, 8, 33)])
def test_agrees_with_the_narrow_pass(B, T, D, K):
    Y, C, la0, lA = _inputs(B, T, D, K)
    for narrow in (False, True):
        got = wide_pass(Y, C, la0, lA, want=True, narrow=narrow)
        assert check(got, Y, C, la0, lA, ALL, label='narrow' if narrow else 'wide') == []


def test_model_against_the_reference_fixture_and_the_generic_engine(tmp_path):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from hmm_wide_models import FORMS, run_cases
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'hmm_wide.npz'))
    gin = {k[3:]: g[k] for k in g.files if k.startswith('in_')}
    res = run_cases(dict(nodes=nodes, VB=VB, vb_kwargs=dict(engine='fused+emissions')), gin)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        gen = run_cases(dict(nodes=nodes, VB=VB, vb_kwargs=dict(engine='generic')), gin)
    for k, v in res.items():
        if k.endswith('_plan'):
            continue
        tol = dict(rtol=L_RTOL, atol=1e-9) if k.endswith('_L') else MOM_TOL
        np.testing.assert_allclose(v, g[k], err_msg=k, **tol)
        np.testing.assert_allclose(v, gen[k], err_msg=k + ' (generic)', **tol)
    for tag, _ in FORMS:
        Q = res[tag + '_plan']
        assert type(Q.plans[0]).__name__ == 'WideHMMPlan'
        fn = str(tmp_path / (tag + '.ckpt'))
        Q.save(filename=fn)
        Q.update(repeat=2, verbose=False)
        L6 = Q.L[:6].copy()
        Q.load(filename=fn)
        Q.update(repeat=2, verbose=False)
        np.testing.assert_array_equal(Q.L[:6], L6)
