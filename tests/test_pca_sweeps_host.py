"""CPU: batches of PCA sweeps without the host (``vmp_pca_sweeps``).

* the stop rule of csrc/vmp_stop_rule.h, compiled with g++, against the Python expression of
  ``VB._end_iteration_step`` on edge values;
* the replay of the loop's bookkeeping from the ring, with a NumPy double of the entry added to
  the kernel test double: chunk cuts, a stop inside a chunk, the decrease warning, a status raised
  at its iteration, log lines, a ``-inf`` previous bound -- always against the per-iteration loop
  of the unchanged double, which lacks the entry and must run as it did.
"""
import ctypes
import hashlib
import math
import os
import subprocess
import tempfile
import warnings

import numpy as np
import pytest

import bayespy_amd.nodes as nodes
from bayespy_amd import _lib
from bayespy_amd.device import Runtime
from bayespy_amd.inference import VB

from fake_kernels import CPURuntimeKernels
from models import build_pca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bayespy_amd', 'csrc')


# ---- the stop rule ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def rule():
    src = os.path.join(ROOT, 'tests', 'host', 'stop_rule_host.cpp')
    hdr = os.path.join(CSRC, 'vmp_stop_rule.h')
    h = hashlib.sha256(open(src, 'rb').read() + open(hdr, 'rb').read()).hexdigest()[:16]
    d = os.path.join(tempfile.gettempdir(), 'bayespy_amd_host_%s' % h)
    so = os.path.join(d, 'libstop_rule_host.so')
    if not os.path.exists(so):
        os.makedirs(d, exist_ok=True)
        tmp = so + '.%d.tmp' % os.getpid()
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-I', CSRC, src,
                               '-o', tmp])
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    lib.stop_rule.restype = ctypes.c_int
    lib.stop_rule.argtypes = [ctypes.c_double] * 3
    lib.bound_sum.restype = ctypes.c_double
    lib.bound_sum.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                              ctypes.c_int]
    return lib


def python_rule(L, L0, tol):
    """vb.py, _record_iteration: L0 comes out of the float64 trace, L is a Python float."""
    L0 = np.float64(L0)
    with np.errstate(all='ignore'):
        div = 0.5 * (abs(L0) + abs(L))
        return bool((L - L0) / div < tol)


def _ulp_cases():
    """Bounds whose relative change lies exactly on, one ulp below and one ulp above tol."""
    out = []
    for L0, L in ((-1000.0, -999.0), (-3.5e6, -3.4999e6), (12.0, 12.5)):
        rel = (L - L0) / (0.5 * (abs(L0) + abs(L)))
        for tol in (rel, np.nextafter(rel, -np.inf), np.nextafter(rel, np.inf)):
            out.append((L, L0, float(tol)))
    return out


EDGE = [
    (float('nan'), -10.0, 1e-5), (-10.0, float('nan'), 1e-5), (-10.0, -11.0, float('nan')),
    (float('inf'), -10.0, 1e-5), (-10.0, float('inf'), 1e-5), (float('-inf'), -10.0, 1e-5),
    (-10.0, float('-inf'), 1e-5), (float('-inf'), float('-inf'), 1e-5),
    (float('inf'), float('inf'), 1e-5),
    (0.0, 0.0, 1e-5), (0.0, 0.0, 0.0), (-0.0, 0.0, -1.0),
    (-12.0, -11.0, 1e-5), (-12.0, -11.0, -1.0),              # a decrease
    (-11.0, -12.0, 1e-5), (-11.0, -12.0, 1.0), (-11.0, -11.0, 0.0), (-11.0, -11.0, 1e-300),
    (1e308, -1e308, 1e-5), (5e-324, 0.0, 1.0),
] + _ulp_cases()


@pytest.mark.parametrize('L,L0,tol', EDGE)
def test_stop_rule_header_is_the_python_expression(rule, L, L0, tol):
    assert bool(rule.stop_rule(L, L0, tol)) == python_rule(L, L0, tol)


def test_ulp_cases_fall_on_both_sides(rule):
    got = [bool(rule.stop_rule(*c)) for c in _ulp_cases()]
    assert got == [False, False, True] * 3


@pytest.mark.parametrize('order', [(0, -1, 2, 1, 3, 4), (4, 3, 2, 1, 0), (2, 0, -1, -1, 4, 3, 1),
                                   (0,), (-1, 3)])
def test_bound_sum_follows_the_order(rule, order):
    # terms whose sum depends on the order of the additions
    terms = [1e16, -1e16, 1.0, 3.0e-1, -7.77e15]
    want = 0.0
    for i in order:
        want += terms[i] if i >= 0 else 0.0
    t = (ctypes.c_double * 5)(*terms)
    o = (ctypes.c_int * len(order))(*order)
    got = rule.bound_sum(t, o, len(order))
    assert got == want
    assert rule.bound_sum((ctypes.c_double * 5)(*([float('nan')] + terms[1:])),
                          (ctypes.c_int * 1)(1), 1) == terms[1]
    assert math.isnan(rule.bound_sum((ctypes.c_double * 5)(*([float('nan')] + terms[1:])), o,
                                     len(order))) == (0 in order)


# ---- the replay ---------------------------------------------------------------------------------
class SweepKernels(CPURuntimeKernels):
    """The double plus a NumPy model of vmp_pca_sweeps: the same operations in the same order as
    the per-node calls of the double, the ring, the stop word."""

    fail_at = None          # (sweep index over all batches, status) to report once
    drop_at = None          # (sweep index over all batches, amount): lowers that sweep's Y term

    def __init__(self, rt):
        super().__init__(rt)
        self.batches = []
        self.executed = self.skipped = self.enqueued = 0

    def sweeps(self, D, K, n_total, x_prec, a0t, b0t, a0a, b0a, Y, ldy, N, X, ldx, lay, state,
               ws, n, ring, tol, compare, l0, order):
        assert lay == 1
        self.batches.append(n)
        r = ring.numpy().reshape(-1, 8)
        stop, L0 = False, l0
        for i in range(n):
            idx = self.enqueued
            self.enqueued += 1
            if stop:
                r[i, 7] = 0.0
                self.skipped += 1
                continue
            self.small_ops(D, K, n_total, x_prec, a0t, b0t, a0a, b0a, [1, 2], state)
            self.xpass_tiled(Y, N, D, K, X, ldx, state, ws)
            self.small_ops(D, K, n_total, x_prec, a0t, b0t, a0a, b0a, [3, 4, 5], state)
            t = self._v(state, D, K)['Lt']
            if self.drop_at is not None and self.drop_at[0] == idx:
                t[0] -= self.drop_at[1]
            status = 0.0
            if self.fail_at is not None and self.fail_at[0] == idx:
                status = float(self.fail_at[1])
            r[i, :6] = t[:6]
            r[i, 6] = status
            r[i, 7] = 1.0
            self.executed += 1
            L = 0.0
            for o in order:
                L += float(t[o]) if o >= 0 else 0.0
            stop = status != 0.0 or bool(compare and python_rule(L, L0, tol))
            L0 = L
        return True


def _model(golden_dir, kernels_cls, chunk=32, **kw):
    g = np.load(os.path.join(golden_dir, 'pca_n500_d6_k3.npz'))
    Q = build_pca(nodes, VB, g['y'], g['x0'], 3, **kw)
    rt = Runtime(device='cpu')
    for p in Q.plans:
        p._rt = rt
        p._kernels = kernels_cls(rt)
        p.sweep_chunk = chunk
    return Q, Q.plans[0]


def _same_trace(Q, R, n):
    assert Q.iter == R.iter == n
    np.testing.assert_array_equal(Q.L[:n], R.L[:n])
    assert len(Q.L) == len(R.L) and len(Q.cputime) == len(R.cputime)
    assert not np.any(np.isnan(Q.cputime[:n]))
    for a, b in zip(Q.model, R.model):
        np.testing.assert_array_equal(Q.l[a][:n], R.l[b][:n])
    assert Q.converged == R.converged
    for name in ('W', 'tau', 'alpha', 'X'):
        for u, v in zip(Q[name].u, R[name].u):
            np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize('chunk', [1, 3, 32])
def test_chunks_replay_the_per_iteration_loop(golden_dir, chunk):
    R, rplan = _model(golden_dir, CPURuntimeKernels)
    R.update(repeat=7, verbose=False)
    Q, plan = _model(golden_dir, SweepKernels, chunk)
    Q.update(repeat=7, verbose=False)
    # the first sweep of a fresh plan runs node by node, the other six in chunks cut at `repeat`
    assert plan.kernels.batches == {1: [1] * 6, 3: [3, 3], 32: [6]}[chunk]
    _same_trace(Q, R, 7)
    # a second call is batches from its first sweep on
    del plan.kernels.batches[:]
    R.update(repeat=4, verbose=False)
    Q.update(repeat=4, verbose=False)
    assert plan.kernels.batches == {1: [1] * 4, 3: [3, 1], 32: [4]}[chunk]
    _same_trace(Q, R, 11)
    assert plan.kernels.calls[-1] == 'xjoin'


def test_unchanged_double_lacks_the_entry_and_runs_as_it_did(golden_dir):
    Q, plan = _model(golden_dir, CPURuntimeKernels)
    assert not hasattr(plan.kernels, 'sweeps')
    Q.update(repeat=3, verbose=False)
    assert plan.kernels.calls.count('xpass_tiled') == 3 and plan.kernels.calls[-1] == 'xjoin'
    assert plan.kernels.calls.count('update_w') == 3


def find_stop(L, n):
    """From the bounds L[:n] of a per-iteration run: (s, tol, j) such that a loop which runs s
    iterations unchecked and then checks with ``tol`` -- halfway between the relative changes of
    two consecutive iterations -- stops at iteration j (1-based), 2 < j < 10, j > s + 1."""
    rel = {i + 1: (L[i] - L[i - 1]) / (0.5 * (abs(L[i - 1]) + abs(L[i]))) for i in range(1, n)}
    for j in range(9, 2, -1):                   # the latest such iteration, the shortest lead-in
        for s in range(1, j - 1):
            tol = 0.5 * (rel[j - 1] + rel[j])
            if rel[j] < tol and all(rel[i] >= tol for i in range(s + 1, j)):
                return s, tol, j
    raise AssertionError('no stopping point in %s' % rel)


def _stopping_run(golden_dir, cls, s, tol, repeat, chunk=32, verbose=False):
    Q, plan = _model(golden_dir, cls, chunk)
    Q.update(repeat=s, verbose=False)
    if hasattr(plan.kernels, 'batches'):
        del plan.kernels.batches[:]
        plan.kernels.executed = plan.kernels.skipped = 0
    Q.ignore_bound_checks = False
    Q.update(repeat=repeat, tol=tol, verbose=verbose)
    return Q, plan


def test_stop_inside_a_chunk(golden_dir, capsys):
    P, _ = _model(golden_dir, CPURuntimeKernels)
    P.update(repeat=12, verbose=False)
    s, tol, j = find_stop(P.L, 12)
    R, _ = _stopping_run(golden_dir, CPURuntimeKernels, s, tol, 12, verbose=True)
    ref_out = capsys.readouterr().out
    assert R.iter == j and R.converged
    Q, plan = _stopping_run(golden_dir, SweepKernels, s, tol, 12, verbose=True)
    out = capsys.readouterr().out
    _same_trace(Q, R, j)
    k = plan.kernels
    assert k.batches == [12] and (k.executed, k.skipped) == (j - s, 12 - (j - s))
    # the log: one line per iteration that ran, then the convergence line (times differ)
    strip = lambda t: [ln.split(' (')[0] for ln in t.splitlines()]       # noqa: E731
    assert strip(out) == strip(ref_out)
    assert len(out.splitlines()) == j - s + 1
    assert out.splitlines()[-1] == 'Converged at iteration %d.' % j


def test_repeat_none_runs_until_the_rule_stops(golden_dir):
    P, _ = _model(golden_dir, CPURuntimeKernels)
    P.update(repeat=12, verbose=False)
    s, tol, j = find_stop(P.L, 12)
    R, _ = _stopping_run(golden_dir, CPURuntimeKernels, s, tol, None)
    Q, plan = _stopping_run(golden_dir, SweepKernels, s, tol, None, chunk=2)
    _same_trace(Q, R, j)
    nb = (j - s + 1) // 2
    assert plan.kernels.batches == [2] * nb and plan.kernels.skipped == 2 * nb - (j - s)


def test_decrease_warns_and_stops_at_its_iteration(golden_dir):
    Q, plan = _model(golden_dir, SweepKernels)
    Q.ignore_bound_checks = False
    plan.kernels.drop_at = (2, 1e7)            # third batched sweep = iteration 4
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        Q.update(repeat=8, tol=1e-12, verbose=False)
    msgs = [str(x.message) for x in w if 'Lower bound decreased' in str(x.message)]
    assert len(msgs) == 1
    assert Q.iter == 4 and Q.converged
    assert (plan.kernels.executed, plan.kernels.skipped) == (3, 4)
    # with the checks off the same drop neither warns nor stops
    Q, plan = _model(golden_dir, SweepKernels)
    plan.kernels.drop_at = (2, 1e7)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        Q.update(repeat=8, tol=1e-12, verbose=False)
    assert not [x for x in w if 'Lower bound decreased' in str(x.message)]
    assert Q.iter == 8 and plan.kernels.skipped == 0


def test_status_is_raised_at_its_iteration(golden_dir):
    Q, plan = _model(golden_dir, SweepKernels)
    plan.kernels.fail_at = (3, _lib.VMP_ERR_NOT_POSDEF)         # iteration 5
    with pytest.raises(_lib.NotPositiveDefiniteError):
        Q.update(repeat=9, verbose=False)
    # iterations 1-4 are recorded, the failing one is not: where the per-iteration loop leaves it
    assert Q.iter == 4 and not np.isnan(Q.L[3]) and np.isnan(Q.L[4])
    assert (plan.kernels.executed, plan.kernels.skipped) == (4, 4)
    assert plan.kernels.calls[-1] == 'xjoin'


def test_minus_infinity_as_the_previous_bound(golden_dir):
    def run(cls):
        Q, plan = _model(golden_dir, cls)
        Q.ignore_bound_checks = False
        # X is still the point mass of its initial value: the bound of this iteration is -inf
        Q.update(Q['W'], Q['tau'], Q['alpha'], repeat=1, verbose=False)
        assert Q.L[0] == -np.inf and plan._delta == {'X'}
        plan.place_plate_arrays()
        with warnings.catch_warnings():
            # (numpy reports inf / inf; the decrease warning must stay silent: -inf - L < 0)
            warnings.simplefilter('ignore', RuntimeWarning)
            warnings.filterwarnings('error', message='Lower bound decreased')
            Q.update(repeat=4, tol=1e-3, verbose=False)
        return Q, plan
    R, _ = run(CPURuntimeKernels)
    Q, plan = run(SweepKernels)
    assert plan.kernels.batches and plan.kernels.batches[0] > 1
    _same_trace(Q, R, R.iter)
    assert R.iter > 2


def test_autosave_cuts_the_chunks(golden_dir, tmp_path):
    saved = {}

    def run(cls, name):
        Q, plan = _model(golden_dir, cls, autosave_filename=str(tmp_path / name),
                         autosave_iterations=3)
        iters = []
        save = Q.save

        def spy(*a, **kw):
            iters.append(Q.iter)
            save(*a, **kw)
            from bayespy_amd.inference.checkpoint import Reader
            r = Reader(str(tmp_path / name))
            saved[name, Q.iter] = {k: np.array(r.get(k)) for k in r.keys()}
            r.close()
        Q.save = spy
        Q.update(repeat=7, verbose=False)
        return Q, plan, iters
    R, _, it_r = run(CPURuntimeKernels, 'ref.ckpt')
    Q, plan, it_q = run(SweepKernels, 'new.ckpt')
    assert it_r == it_q == [3, 6]
    assert plan.kernels.batches == [2, 3, 1]
    for it in (3, 6):
        a, b = saved['ref.ckpt', it], saved['new.ckpt', it]
        assert sorted(a) == sorted(b)
        for key in a:
            if key != 'cputime':
                np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    _same_trace(Q, R, 7)


def test_fallbacks_use_no_batch(golden_dir):
    # a callback needs the host after every sweep
    Q, plan = _model(golden_dir, SweepKernels, callback=lambda: None)
    Q.update(repeat=3, verbose=False)
    assert plan.kernels.batches == []
    # another node order
    Q, plan = _model(golden_dir, SweepKernels)
    Q.update(Q['X'], Q['W'], Q['tau'], Q['alpha'], repeat=3, verbose=False)
    assert plan.kernels.batches == []
    # the streaming-statistics form
    Q, plan = _model(golden_dir, SweepKernels)
    plan.stats = 'stream'
    Q.update(repeat=3, verbose=False)
    assert plan.kernels.batches == []
    # passes that are not deferred
    Q, plan = _model(golden_dir, SweepKernels)
    plan.defer_passes = False
    Q.update(repeat=3, verbose=False)
    assert plan.kernels.batches == []
