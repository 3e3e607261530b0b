"""GPU: the segmented (time-parallel) chain stage of the fused hidden-Markov-model block --
``vmp_hmm_seg_pass`` alone against the long-double restatement of the reference arithmetic (inputs,
restatement and ``check`` of tests/test_hmm_wide_gpu.py: the allowance rule of DESIGN.md sections
4.15 / 4.15b unchanged) at the segment shapes where it can go wrong, its masked twin, tables with
-1000 and -inf under emissions hundreds of nats apart, fixed labels and the prior pass, and the
fixture models through engine='fused+chains'.  Measured figures: DESIGN.md section 4.15c."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

pytestmark = pytest.mark.gpu

from test_hmm_wide_gpu import ALL, SUMS, _inputs, check, wide_pass  # noqa: E402


def seg_pass(L, Y, C, la0, lA, labels=None, want=False, mask=None):
    """tests/test_hmm_fused_gpu.py ``gpu_pass`` on the kernels of the long-chain form."""
    import test_hmm_fused_gpu as narrow_gpu
    from bayespy_amd.inference.plans import hmm, hmm_seg
    keep = hmm.HMMKernels
    hmm.HMMKernels = type('K', (hmm_seg.SegmentedHMMKernels,), dict(seg_len=L))
    try:
        return narrow_gpu.gpu_pass(Y, C, la0, lA, labels, want, mask)
    finally:
        hmm.HMMKernels = keep


# (B, T, D, K, L): T = 2; T = L + 1; T = L + 2; T = 2 L + 1; a ragged last segment with a ragged
# last workgroup; L = 1; L >= T - 1; every KP; B = 1, 5, 65; D = 1, 9, 32
SHAPES = [(1, 2, 1, 1, 3), (5, 5, 9, 3, 4), (5, 6, 9, 3, 4), (1, 9, 1, 17, 4), (65, 12, 1, 3, 4),
          (5, 7, 32, 33, 1), (1, 6, 9, 64, 8), (5, 11, 32, 64, 3), (65, 4, 9, 1, 2),
          (1, 70, 9, 17, 16), (5, 10, 1, 33, 3), (65, 9, 32, 3, 2)]


@pytest.mark.parametrize('B,T,D,K,L', SHAPES)
def test_pass_against_long_double(B, T, D, K, L):
    Y, C, la0, lA = _inputs(B, T, D, K)
    got = seg_pass(L, Y, C, la0, lA, want=True)
    assert check(got, Y, C, la0, lA, ALL, label=str((B, T, D, K, L))) == []
    # the optional outputs off: the same bits; a second call: the same bits
    off, again = seg_pass(L, Y, C, la0, lA), seg_pass(L, Y, C, la0, lA)
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(off[k], got[k], err_msg=k)
        np.testing.assert_array_equal(again[k], off[k], err_msg=k)


@pytest.mark.parametrize('D,K', [(9, 5), (32, 64)])
def test_masked_pass_against_long_double(D, K):
    from hmm_fused_host import nan_fill
    B, T, L = 6, 13, 3
    Y, C, la0, lA = _inputs(B, T, D, K)
    mask = np.ones((B, T), bool)
    mask[0, 4:7] = False                    # the whole second segment (steps 4 ... 6)
    mask[1, 0] = mask[1, -1] = False        # the first and the last step
    mask[2] = False                         # nothing observed
    mask[3, 5:] = False                     # ragged tails, one inside a segment ...
    mask[4, 1:] = False                     # ... and one that leaves step 0 alone
    got = seg_pass(L, nan_fill(Y, mask), C, la0, lA, want=True, mask=mask)
    assert check(got, Y, C, la0, lA, ALL, label='masked ' + str((D, K)), mask=mask) == []
    ones, none = seg_pass(L, Y, C, la0, lA, mask=np.ones((B, T))), seg_pass(L, Y, C, la0, lA)
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(ones[k], none[k], err_msg=k)


@pytest.mark.parametrize('L', [2, 4])
def test_extreme_tables(L):
    """A left-to-right chain: -inf below the diagonal, -1000 above the first off-diagonal, and
    emissions hundreds of nats apart -- what a linear-domain product scaled per row flushes."""
    from bayespy_amd.inference.plans.hmm import emission_tables
    rs = np.random.RandomState(L)
    B, T, D, K = 3, 11, 2, 4
    mu = 30.0 * np.arange(K)[:, None] * np.ones(D)
    C, _ = emission_tables(mu, np.identity(D))
    z = np.sort(rs.randint(K, size=(B, T)), axis=1)
    Y = mu[z] + rs.normal(size=(B, T, D))
    lA = np.full((K, K), -1000.0)
    lA[np.tril_indices(K, -1)] = -np.inf
    lA[np.arange(K), np.arange(K)] = np.log(0.7)
    lA[np.arange(K - 1), np.arange(1, K)] = np.log(0.3)
    la0 = np.array([0.0, -1000.0, -np.inf, -np.inf])
    got = seg_pass(L, Y, C, la0, lA, want=True)
    lower = np.tril_indices(K, -1)
    assert np.all(np.isfinite(got['zz'])) and np.all(got['zz'][:, :, lower[0], lower[1]] == 0)
    assert check(got, Y, C, la0, lA, ALL, label='left-to-right L=%d' % L) == []


@pytest.mark.parametrize('B,T,D,K,L', [(5, 7, 12, 3, 2), (3, 4, 32, 33, 1)])
def test_prior_pass_and_labels(B, T, D, K, L):
    from hmm_fused_host import compare
    Y, C, la0, lA = _inputs(B, T, D, K)
    assert compare(seg_pass(L, Y, None, la0, lA), Y, None, la0, lA, label='prior') == []
    lab = np.random.RandomState(1).randint(K, size=(B, T))
    r, ref = seg_pass(L, Y, C, la0, lA, labels=lab, want=True), wide_pass(Y, C, la0, lA, labels=lab, want=True)
    for k in ALL + ('dots',):
        np.testing.assert_array_equal(r[k], ref[k], err_msg=k)


def _long_chains(Q):
    assert type(Q.plans[0]).__name__ == 'SegmentedHMMPlan'
    Q.plans[0].seg_len = 3


def test_fixture_models_through_the_long_chain_engine(tmp_path):
    from bayespy_amd.inference.plans import compile_model
    from hmm_models import run_hmm_cases
    import test_hmm_fused_host as plain
    import test_hmm_masked_host as masked
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        g, gin = plain._golden()
        res = run_hmm_cases(plain._mods(_long_chains, engine='fused+chains'), gin)
        plain.check_fixtures(res, g)
        g, gin = masked._golden()
        masked.check_masked_fixtures(
            run_hmm_cases(masked._mods(_long_chains, engine='fused+chains'), gin), g)
    Q = res['e_plan']
    assert Q.plans[0].chains_per_wg == min(3, Q.plans[0].T - 1)     # the segment length in use
    fn = str(tmp_path / 'seg.ckpt')
    Q.save(filename=fn)
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)
    m = plain._model('a')
    assert [type(p).__name__ for p in compile_model(plain._nodes(m), engine='fused')] == ['HMMPlan']
