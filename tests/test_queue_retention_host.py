"""
Host logic of the queue of small operations: a queued record runs LATER, so the runtime must keep
the arrays of every call the library can have queued alive until the flush
(Runtime.keep_until_flush).  The library's rules (csrc/vmp_generic.hip): inverses when
8 < n <= 32 and batch <= 4 (vmp_spd_batched), sums of <= 2048 outputs and <= 32768 products
(vmp_sum_multiply), formulas of <= small_queue_ew_max elements (vmp_ewise).  Run on a CPU runtime
with the NumPy double of the generic entry points (tests/host_generic.py), the queue opened by hand.
"""
import numpy as np
import pytest

from bayespy_amd import device
from bayespy_amd.darray import DArray, fuse
from bayespy_amd.utils import linalg, misc
from host_generic import HostGenericLib


@pytest.fixture
def rt():
    r = device.Runtime(device='cpu')
    r.lib = HostGenericLib()
    device.set_runtime(r)
    # what queue_begin does on a device: an open operation, the queue on, sums and inverses in it
    r._op_depth = 1
    r._queue_env = True
    r._tune_sm = True
    yield r
    device.set_runtime(None)


def _alive(rt):
    ids = set()
    for arrays, out in rt._queue_alive:
        for a in list(arrays) + list(out if isinstance(out, (tuple, list)) else (out,)):
            ids.add(id(getattr(a, 't', a)))
    return ids


def _spd(n, batch, rng):
    B = rng.standard_normal((batch, n, n))
    return np.einsum('bij,bkj->bik', B, B) + n * np.eye(n)


@pytest.mark.parametrize('n', [8, 9, 16, 22, 23, 24, 31, 32, 33])
@pytest.mark.parametrize('batch', [1, 2, 3, 4, 5])
def test_inverse_operand_kept_exactly_when_queued(rt, n, batch):
    C = DArray.from_host(_spd(n, batch, np.random.default_rng(n)))
    rt._queue_alive = []
    U = linalg.chol(C)
    queued = 8 < n <= 32 and batch <= 4
    assert (id(C.t) in _alive(rt)) == queued
    assert (id(U._inv.t) in _alive(rt)) == queued
    np.testing.assert_allclose(linalg.chol_inv(U).numpy(), np.linalg.inv(C.numpy()), rtol=1e-9,
                               atol=1e-12)


@pytest.mark.parametrize('nkeep,nred', [(1, 32768), (2047, 16), (2048, 16), (2048, 1), (2049, 1),
                                        (2049, 8), (16, 2048), (1024, 32)])
def test_sum_operands_kept_when_queued(rt, nkeep, nred):
    rng = np.random.default_rng(nkeep + nred)
    A = DArray.from_host(rng.standard_normal((nkeep, nred)))
    x = DArray.from_host(rng.standard_normal(nred))
    rt._queue_alive = []
    r = misc.sum_multiply(A, x, axis=-1)
    queued = nkeep <= 2048 and nkeep * nred <= 32768
    kept = id(A.t) in _alive(rt) and id(x.t) in _alive(rt)
    assert kept == queued
    np.testing.assert_allclose(r.numpy(), A.numpy() @ x.numpy(), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('ew_max', [2048, 8192])
@pytest.mark.parametrize('size', [1, 2048, 2049, 8192, 8193])
def test_formula_operands_kept_exactly_when_queued(rt, size, ew_max):
    rt.set_tune('small_queue_ew_max', ew_max)
    a = DArray.from_host(np.arange(size, dtype=np.float64))
    rt._queue_alive = []
    r = fuse(lambda v: v * v + 1.0, a)
    assert (id(a.t) in _alive(rt)) == (size <= ew_max)
    np.testing.assert_array_equal(r.numpy(), np.arange(size) ** 2 + 1.0)


def test_nothing_kept_outside_an_operation_or_with_the_tune_off(rt):
    C = DArray.from_host(_spd(24, 4, np.random.default_rng(0)))
    rt._op_depth = 0
    rt._queue_alive = []
    linalg.chol(C)
    assert rt._queue_alive == []
    rt._op_depth = 1
    rt._tune_sm = False
    linalg.chol(C)
    assert rt._queue_alive == []
