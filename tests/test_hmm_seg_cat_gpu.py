"""GPU: the segmented (time-parallel) chain pass of the fused discrete hidden-Markov-model block --
``vmp_hmm_seg_pass_categorical`` alone against the long-double restatement of the reference
arithmetic (inputs, restatement and ``compare`` of tests/hmm_cat_host.py: the allowance rule of
DESIGN.md sections 4.14 / 4.15 unchanged) at the segment shapes where it can go wrong, its masked
twin, tables with -1000 and -inf under a <log P> whose columns lie hundreds of nats apart, the
prior pass and fixed labels, the plan entry, and the fixture models through engine='fused+chains'.
Measured figures: DESIGN.md section 4.15d."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu

from hmm_cat_host import ALL, SUMS, compare, pass_inputs  # noqa: E402
from hmm_fused_host import mixed_mask  # noqa: E402


def seg_pass(L, y, Pt, la0, lA, labels=None, want=False, mask=None):
    """tests/test_hmm_cat_gpu.py ``gpu_pass`` on the kernels of the long-chain form."""
    import test_hmm_cat_gpu as seq_gpu
    from bayespy_amd.inference.plans import hmm_cat, hmm_seg_cat
    keep = hmm_cat.CatHMMKernels
    hmm_cat.CatHMMKernels = type('K', (hmm_seg_cat.SegmentedCatHMMKernels,), dict(seg_len=L))
    try:
        return seq_gpu.gpu_pass(y, Pt, la0, lA, labels, want, mask)
    finally:
        hmm_cat.CatHMMKernels = keep


# (B, T, M, K, L): T = 2; T = L + 1; T = L + 2; T = 2 L + 1; many chains; L = 1; L >= T - 1; the
# LDS maximum with a ragged last segment; K = 1; a long single chain; KP = 8, 2, 16
SHAPES = [(1, 2, 1, 1, 3), (5, 5, 3, 3, 4), (5, 6, 3, 3, 4), (1, 9, 128, 17, 4), (65, 12, 3, 3, 4),
          (5, 7, 128, 33, 1), (1, 6, 3, 64, 8), (5, 11, 128, 64, 3), (65, 4, 128, 1, 2),
          (1, 70, 3, 17, 16), (3, 8, 128, 5, 3), (5, 10, 128, 2, 3), (65, 9, 3, 9, 2)]


@pytest.mark.parametrize('B,T,M,K,L', SHAPES)
def test_pass_against_long_double(B, T, M, K, L):
    y, Pt, la0, lA = pass_inputs(B, T, M, K)
    got = seg_pass(L, y, Pt, la0, lA, want=True)
    assert compare(got, y, Pt, la0, lA, ALL, label=str((B, T, M, K, L))) == []
    # the optional outputs off, a second call, a mask of ones: the same bits
    off, again = seg_pass(L, y, Pt, la0, lA), seg_pass(L, y, Pt, la0, lA)
    ones = seg_pass(L, y, Pt, la0, lA, mask=np.ones((B, T)))
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(off[k], got[k], err_msg=k)
        np.testing.assert_array_equal(again[k], off[k], err_msg=k)
        np.testing.assert_array_equal(ones[k], off[k], err_msg=k)


@pytest.mark.parametrize('M,K', [(3, 5), (128, 64)])
def test_masked_pass_against_long_double(M, K):
    B, T, L = 6, 13, 3
    y, Pt, la0, lA = pass_inputs(B, T, M, K)
    mask = np.ones((B, T), bool)
    mask[0, 4:7] = False                    # the whole second segment (steps 4 ... 6)
    mask[1, 0] = mask[1, -1] = False        # the first and the last step
    mask[2] = False                         # nothing observed
    mask[3, 5:] = False                     # ragged tails, one inside a segment ...
    mask[4, 1:] = False                     # ... and one that leaves step 0 alone
    got = seg_pass(L, np.where(mask, y, -1), Pt, la0, lA, want=True, mask=mask)
    assert compare(got, y, Pt, la0, lA, ALL, label='masked ' + str((M, K)), mask=mask) == []


@pytest.mark.parametrize('L', [2, 4])
def test_extreme_tables(L):
    """A left-to-right chain: -inf below the diagonal, -1000 above the first off-diagonal, and a
    <log P> table whose columns lie hundreds of nats apart -- what a linear-domain product scaled
    per row flushes."""
    rs = np.random.RandomState(L)
    B, T, K = 3, 11, 4
    y = np.sort(rs.randint(K, size=(B, T)), axis=1)
    d = np.abs(np.arange(K)[:, None] - np.arange(K)[None, :])
    Pt = np.where(d == 0, np.log(0.9), np.where(d == 3, -1000.0, -300.0 * d))
    lA = np.full((K, K), -1000.0)
    lA[np.tril_indices(K, -1)] = -np.inf
    lA[np.arange(K), np.arange(K)] = np.log(0.7)
    lA[np.arange(K - 1), np.arange(1, K)] = np.log(0.3)
    la0 = np.array([0.0, -1000.0, -np.inf, -np.inf])
    got = seg_pass(L, y, Pt, la0, lA, want=True)
    lower = np.tril_indices(K, -1)
    assert np.all(np.isfinite(got['zz'])) and np.all(got['zz'][:, :, lower[0], lower[1]] == 0)
    assert compare(got, y, Pt, la0, lA, ALL, label='left-to-right L=%d' % L) == []


@pytest.mark.parametrize('B,T,M,K,L', [(5, 7, 4, 3, 2), (3, 4, 128, 33, 1)])
def test_prior_pass_and_labels(B, T, M, K, L):
    from test_hmm_cat_gpu import gpu_pass
    y, Pt, la0, lA = pass_inputs(B, T, M, K)
    assert compare(seg_pass(L, y, M, la0, lA), y, M, la0, lA, label='prior') == []
    lab = np.random.RandomState(1).randint(K, size=(B, T))
    for mask in (None, mixed_mask(B, T, np.random.RandomState(2))):
        r = seg_pass(L, y, Pt, la0, lA, labels=lab, want=True, mask=mask)
        ref = gpu_pass(y, Pt, la0, lA, labels=lab, want=True, mask=mask)
        for k in ALL + ('dots',):
            np.testing.assert_array_equal(r[k], ref[k], err_msg=k)


def _long_chains(Q):
    assert type(Q.plans[0]).__name__ == 'SegmentedCategoricalHMMPlan' and len(Q.plans) == 1
    Q.plans[0].seg_len = 3


def test_fixture_models_through_the_long_chain_engine(tmp_path):
    """Fails without the feature: engine='fused+chains' builds ``CategoricalHMMPlan``."""
    from bayespy_amd.inference.plans import compile_model
    from hmm_cat_models import run_cases
    from test_hmm_cat_host import _mods, _golden, _model, _nodes, check_fixtures
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_cases(_mods(_long_chains, engine='fused+chains'), gin, fill=-1)
    check_fixtures(res, g)
    Q = res['ii_plan']
    assert Q.plans[0].chains_per_wg == min(3, Q.plans[0].T - 1)     # the segment length in use
    fn = str(tmp_path / 'seg_cat.ckpt')
    Q.save(filename=fn)
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)
    plans = compile_model(_nodes(_model('ii')), engine='fused')
    assert [type(p).__name__ for p in plans] == ['CategoricalHMMPlan']


def test_plan_entry():
    from bayespy_amd import _lib
    lib = _lib.load()

    def plan(fn, *a):
        used, w = (ctypes.c_int32 if 'seg' in fn else ctypes.c_int64)(), ctypes.c_int64()
        return getattr(lib, fn)(*a, ctypes.byref(used), ctypes.byref(w)), used.value, w.value
    for B, T, M, K, L in SHAPES + [(1, 200000, 64, 16, 0), (4096, 1000, 128, 64, 0)]:
        rc, used, w = plan('vmp_hmm_seg_cat_plan', B, T, M, K, L)
        assert (rc, used) == plan('vmp_hmm_seg_plan', B, T, 1, K, L)[:2] and rc == _lib.VMP_OK
        assert w >= plan('vmp_hmm_fused_cat_plan', B, T, M, K)[2] > 0
    assert plan('vmp_hmm_seg_cat_plan', 1, 9, 3, 65, 0)[0] == _lib.VMP_ERR_UNSUPPORTED
    assert plan('vmp_hmm_seg_cat_plan', 1, 9, 129, 3, 0)[0] == _lib.VMP_ERR_UNSUPPORTED
