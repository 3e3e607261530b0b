"""GPU: the large-vocabulary pass of the fused discrete hidden-Markov-model block --
``vmp_hmm_vocab_pass`` alone against the long-double restatement of the reference arithmetic
(inputs, restatement and ``compare`` of tests/hmm_cat_host.py: the allowance rule of DESIGN.md
sections 4.14 / 4.15 unchanged) at the chunk and word shapes where the segmented count can go wrong,
a word border on a chunk border, masks, the prior pass and fixed labels, the plan entry, and the
fixture models of tests/golden/hmm_vocab.npz through engine='fused+words'.
Measured figures: DESIGN.md section 4.15e."""
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


def vocab_pass(*args, **kw):
    """tests/test_hmm_cat_gpu.py ``gpu_pass`` on the kernels of the large-vocabulary form."""
    import test_hmm_cat_gpu as seq_gpu
    from bayespy_amd.inference.plans import hmm_cat, hmm_vocab
    keep = hmm_cat.CatHMMKernels
    hmm_cat.CatHMMKernels = hmm_vocab.VocabCatHMMKernels
    try:
        return seq_gpu.gpu_pass(*args, **kw)
    finally:
        hmm_cat.CatHMMKernels = keep


# (B, T, M, K): the smallest; four chunks, the last ragged, every word across a border; one word
# over five chunks (head-only chunks, KP = 32); more words than entries (KP = 64, the LDS half of
# sum xi); three workgroups of chains (KP = 2); KP = 4, 8, 16; six full chunks at the old limit
SHAPES = [(1, 2, 1, 1), (1, 53, 3, 3), (1, 70, 1, 17), (5, 7, 129, 33), (65, 4, 4099, 2),
          (3, 11, 1000, 4), (17, 5, 131, 5), (9, 9, 300, 9), (3, 32, 128, 64)]


@pytest.mark.parametrize('B,T,M,K', SHAPES)
def test_pass_against_long_double(B, T, M, K):
    y, Pt, la0, lA = pass_inputs(B, T, M, K)
    got = vocab_pass(y, Pt, la0, lA, want=True)
    assert compare(got, y, Pt, la0, lA, ALL, label=str((B, T, M, K))) == []
    # the optional outputs off, a second call, a mask of ones: the same bits
    off, again = vocab_pass(y, Pt, la0, lA), vocab_pass(y, Pt, la0, lA)
    ones = vocab_pass(y, Pt, la0, lA, mask=np.ones((B, T)))
    for k in SUMS + ('dots',):
        np.testing.assert_array_equal(off[k], got[k], err_msg=k)
        np.testing.assert_array_equal(again[k], off[k], err_msg=k)
        np.testing.assert_array_equal(ones[k], off[k], err_msg=k)


def test_word_border_on_a_chunk_border():
    _, Pt, la0, lA = pass_inputs(1, 37, 3, 5)
    y = np.random.RandomState(7).permutation(np.repeat([0, 1, 2], [16, 16, 5]))[None, :]
    got = vocab_pass(y, Pt, la0, lA, want=True)
    assert compare(got, y, Pt, la0, lA, ALL, label='border') == []


@pytest.mark.parametrize('M', [3, 300])
def test_masked_pass_against_long_double(M):
    B, T, K = 6, 13, 5
    y, Pt, la0, lA = pass_inputs(B, T, M, K)
    mask = np.ones((B, T), bool)
    mask[0, 4:7] = False                    # a hole
    mask[1, 0] = mask[1, -1] = False        # the first and the last step
    mask[2] = False                         # nothing observed
    mask[3, 5:] = False                     # ragged tails ...
    mask[4, 1:] = False                     # ... and one that leaves step 0 alone
    got = vocab_pass(np.where(mask, y, -1), Pt, la0, lA, want=True, mask=mask)
    assert compare(got, y, Pt, la0, lA, ALL, label='masked %d' % M, mask=mask) == []


def test_prior_pass_and_labels():
    from test_hmm_cat_gpu import gpu_pass
    B, T, M, K = 5, 7, 128, 3
    y, Pt, la0, lA = pass_inputs(B, T, M, K)
    assert compare(vocab_pass(y, M, la0, lA), y, M, la0, lA, label='prior') == []
    lab = np.random.RandomState(1).randint(K, size=(B, T))
    for mask in (None, mixed_mask(B, T, np.random.RandomState(2))):
        r = vocab_pass(y, Pt, la0, lA, labels=lab, want=True, mask=mask)
        ref = gpu_pass(y, Pt, la0, lA, labels=lab, want=True, mask=mask)
        for k in ALL + ('dots',):
            np.testing.assert_array_equal(r[k], ref[k], err_msg=k)


def _on_words(Q):
    assert type(Q.plans[0]).__name__ == 'VocabCategoricalHMMPlan' and len(Q.plans) == 1


def test_fixture_models_through_the_vocabulary_engine(tmp_path):
    """Fails without the feature: engine='fused+words' matches nothing."""
    from bayespy_amd.inference.plans import compile_model
    from hmm_vocab_models import CASES, build, run_cases
    from test_hmm_cat_host import _mods, _nodes, L_RTOL, MOM_TOL
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'hmm_vocab.npz'))
    gin = {k[3:]: g[k] for k in g.files if k.startswith('in_')}
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_cases(_mods(_on_words, engine='fused+words'), gin, fill=-1)
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan') or k.endswith('_model'):
            continue
        if k.endswith('_mask'):
            np.testing.assert_array_equal(v, g[k], err_msg=k)
        elif '_u' in k:
            np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL)
        checked += 1
    assert checked == len([k for k in g.files if not k.startswith('in_')]) == 2 * 11 + 2
    assert g['x_Z_mask'].all() and not g['x_Y_mask'].all() and sorted(CASES) == ['w', 'x']
    Q = res['w_plan']
    fn = str(tmp_path / 'vocab.ckpt')
    Q.save(filename=fn)
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)
    with pytest.raises(NotImplementedError, match='M = 131, K = 3 exceed the limits of the block'):
        compile_model(_nodes(build(_mods(), gin, 'w')), engine='fused')


def test_plan_entry():
    from bayespy_amd import _lib
    lib = _lib.load()
    mk, mm = ctypes.c_int32(), ctypes.c_int32()
    assert lib.vmp_hmm_vocab_limits(ctypes.byref(mk), ctypes.byref(mm)) == _lib.VMP_OK
    assert (mk.value, mm.value) == (64, 65536)

    def plan(B, T, M, K):
        c, ch, w = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
        rc = lib.vmp_hmm_vocab_plan(B, T, M, K, B * T, ctypes.byref(c), ctypes.byref(ch),
                                    ctypes.byref(w))
        return rc, ch.value, w.value
    for B, T, M, K in SHAPES + [(1, 37, 3, 5), (6, 13, 300, 5), (5, 7, 128, 3)]:
        rc, ch, w = plan(B, T, M, K)
        assert (rc, ch) == (_lib.VMP_OK, 16) and w >= B * T * K > 0
    rc, ch, w = plan(4096, 1000, 65536, 64)
    assert rc == _lib.VMP_OK and w >= 4096 * 1000 * 64 > 0
    assert plan(1, 9, 3, 65)[0] == plan(1, 9, 65537, 3)[0] == _lib.VMP_ERR_UNSUPPORTED
    assert plan(1, 1, 3, 3)[0] == _lib.VMP_ERR_INVALID
