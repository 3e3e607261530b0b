"""CPU: the wide-emission form of the fused hidden-Markov-model block without a device -- the
matcher, the engine values, the checkpoint-form message and the host-only entry points of the
C ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _model(D, K=3, B=2, T=5):
    import bayespy_amd.nodes as nodes
    from hmm_models import build_hmm
    m = build_hmm(dict(nodes=nodes), np.zeros((B, T, D)), np.zeros((K, D)), np.identity(D))
    return m, [m['Y'], m['Z'], m['A'], m['a0']]


def test_engine_values():
    """Fails without the feature: 'fused+emissions' is no engine and D = 12 has no block."""
    from bayespy_amd.inference.plans import OPT_IN_WIDE_EMISSIONS, compile_model
    from bayespy_amd.inference.plans.hmm import HMMPlan
    from bayespy_amd.inference.plans.hmm_wide import WideHMMPlan
    assert OPT_IN_WIDE_EMISSIONS == {HMMPlan: [WideHMMPlan]}
    m, nodes = _model(12)
    with pytest.raises(NotImplementedError, match=r'fused hidden-Markov-model block, observed node '
                                                  r'Y: D = 12, K = 3 exceed the limits'):
        compile_model(nodes, engine='fused')
    plans = compile_model(nodes, engine='fused+emissions')
    assert [type(p) for p in plans] == [WideHMMPlan]
    assert compile_model(nodes, engine='fused+emissions')[0] is plans[0]       # kept where asked for
    with pytest.raises(NotImplementedError, match='exceed the limits'):
        compile_model(nodes, engine='fused')
    m, nodes = _model(8)
    assert [type(p) for p in compile_model(nodes, engine='fused+emissions')] == [HMMPlan]


def test_matcher_declines_with_the_label_of_the_form():
    from bayespy_amd.inference.plans.hmm_wide import LABEL, WideHMMPlan
    assert LABEL == 'fused hidden-Markov-model block (wide emissions)'
    for D, text in ((8, 'D = 8: use the HMM block'), (33, 'D = 33, K = 3 exceed the limits')):
        why = []
        assert WideHMMPlan.match(_model(D)[1], why) is None
        assert len(why) == 1 and why[0].startswith(LABEL) and text in why[0], why
    m, nodes = _model(12)
    m['Y'].observe(np.zeros((2, 5, 12)), mask=False)                # what HMMPlan declines
    why = []
    assert WideHMMPlan.match(nodes, why) is None and why[0].startswith(LABEL) and 'mask' in why[0]


class _Reader:
    def __init__(self, kind):
        self.kind = np.array([ord(c) for c in kind], dtype=np.uint8)

    def has(self, key):
        return key.endswith('kind')

    def get(self, key):
        return self.kind


@pytest.mark.parametrize('D,kind,text', [
    (12, 'hmm', 'Gaussian (the wide form, 9 <= D <= 32) emissions: it holds that of the block with '
                'Gaussian emissions'),
    (8, 'hmm_wide', 'Gaussian emissions: it holds that of the block with Gaussian (the wide form')])
def test_checkpoint_names_the_form(D, kind, text):
    from bayespy_amd.inference.plans import compile_model
    plan = compile_model(_model(D)[1], engine='fused+emissions')[0]
    plan._ready = True                                  # nothing to set up before the kind is read
    with pytest.raises(Exception, match=text.replace('(', r'\(').replace(')', r'\)')):
        plan.load_state(_Reader(kind), None, 0)


def test_cabi_limits_and_plan():
    from bayespy_amd import _lib
    lib = _lib.load()
    for name in ('vmp_hmm_wide_limits', 'vmp_hmm_wide_plan', 'vmp_hmm_wide_pass'):
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    mk, md = ctypes.c_int32(), ctypes.c_int32()
    assert lib.vmp_hmm_wide_limits(ctypes.byref(mk), ctypes.byref(md)) == _lib.VMP_OK
    assert (mk.value, md.value) == (64, 32)
    assert lib.vmp_hmm_wide_limits(None, None) == _lib.VMP_ERR_INVALID
    c, w = ctypes.c_int64(), ctypes.c_int64()
    plan = lambda *a: lib.vmp_hmm_wide_plan(*a, ctypes.byref(c), ctypes.byref(w))  # noqa: E731
    for B, T, D, K, KP in ((0, 2, 1, 1, 2), (1000, 70, 16, 5, 8), (4096, 1000, 32, 16, 16),
                           (10 ** 5, 10, 32, 64, 64)):
        assert plan(B, T, D, K) == _lib.VMP_OK
        assert c.value % (64 // KP) == 0 and -(-B // c.value) <= 4096
        NF = D * (D + 1) // 2 + D + 1
        least = B * T * (KP + K) + -(-B // c.value) * (K + K * K + 2) + 1024
        assert least <= w.value <= least + 2 ** 24 + K * NF
    U, I = _lib.VMP_ERR_UNSUPPORTED, _lib.VMP_ERR_INVALID
    assert plan(10, 4, 2, 65) == U and plan(10, 4, 33, 4) == U
    assert plan(-1, 4, 2, 4) == I and plan(10, 1, 2, 4) == I and plan(10, 4, 0, 4) == I
    assert lib.vmp_hmm_wide_plan(10, 4, 2, 4, None, None) == I
    # the pass judges the shape before the pointers, without a context
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda D=2, K=3, T=3, ldc=6: lib.vmp_hmm_wide_pass(  # noqa: E731
        None, 4, T, D, K, p, p, ldc, p, p, None, None, p, p, p, p, p, None, None, None)
    assert call() == I and call(T=1) == I and call(ldc=5) == I
    assert call(K=65) == U and call(D=33) == U
