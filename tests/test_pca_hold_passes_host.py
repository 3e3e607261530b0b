"""CPU: the hint ``VB.update`` gives a plan before every sweep (``hold_passes``), with the kernel
test double.  The double has no ``hold_passes`` entry point: the loop must run exactly as it did
(tests/test_pca_plan_host.py fixes its call list).  A double WITH the entry point shows when the
plan forwards the hint."""
import os

import numpy as np

import bayespy_amd.nodes as nodes
from bayespy_amd.device import Runtime
from bayespy_amd.inference import VB

from fake_kernels import CPURuntimeKernels
from models import build_pca


class HoldingKernels(CPURuntimeKernels):
    """Records the hint beside the kernel calls (it computes every pass: holding is the
    library's business)."""

    def hold_passes(self, on):
        self.calls.append('hold' if on else 'release')


def _model(golden_dir, kernels_cls):
    g = np.load(os.path.join(golden_dir, 'pca_n500_d6_k3.npz'))
    Q = build_pca(nodes, VB, g['y'], g['x0'], 3)
    rt = Runtime(device='cpu')
    for p in Q.plans:
        p._rt = rt
        p._kernels = kernels_cls(rt)
    return Q, Q.plans[0]


def test_double_without_the_entry_point_runs_unchanged(golden_dir):
    Q, plan = _model(golden_dir, CPURuntimeKernels)
    assert plan.defer_passes and not hasattr(plan.kernels, 'hold_passes')
    Q.update(repeat=3, verbose=False)
    assert not plan._hold and not plan._lib_hold
    assert plan.kernels.calls.count('xpass_tiled') == 3 and plan.kernels.calls[-1] == 'xjoin'
    Q2, _ = _model(golden_dir, HoldingKernels)
    Q2.update(repeat=3, verbose=False)
    np.testing.assert_array_equal(Q.L[:3], Q2.L[:3])


def test_hint_is_forwarded_around_the_sweeps(golden_dir):
    Q, plan = _model(golden_dir, HoldingKernels)
    Q.update(repeat=3, verbose=False)
    calls = [c for c in plan.kernels.calls if c in ('hold', 'release', 'xpass_tiled', 'xjoin')]
    # holding starts before the first sweep and ends right AFTER the last sweep's pass was issued
    # (that pass takes the place of the held one and is launched beside tau / alpha / bound)
    assert calls == ['hold', 'xpass_tiled', 'xpass_tiled', 'xpass_tiled', 'release', 'xjoin']
    # one sweep per call: nothing to hold
    del plan.kernels.calls[:]
    Q.update(repeat=1, verbose=False)
    assert 'hold' not in plan.kernels.calls and 'release' not in plan.kernels.calls
    # a sweep that does not update X: the hold ends with the update call
    del plan.kernels.calls[:]
    Q.update(Q['W'], Q['tau'], repeat=2, verbose=False)
    calls = [c for c in plan.kernels.calls if c in ('hold', 'release', 'xpass_tiled', 'xjoin')]
    assert calls == ['hold', 'release', 'xjoin']


def test_defer_passes_false_never_holds(golden_dir):
    Q, plan = _model(golden_dir, HoldingKernels)
    plan.defer_passes = False
    Q.update(repeat=3, verbose=False)
    assert 'hold' not in plan.kernels.calls and 'release' not in plan.kernels.calls
