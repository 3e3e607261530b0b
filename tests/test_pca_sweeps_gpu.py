"""
Batches of PCA sweeps that run without the host (vmp_pca_sweeps) against the per-iteration loop,
which the tune key "pca_sweeps" = 0 selects: the same kernels' arithmetic in the same order, so
EVERYTHING is compared bitwise (np.array_equal), never with a tolerance.

The counters (vmp_pca_sweep_counts, vmp_pca_pass_counts) belong to the process-wide context:
every check is on deltas.
"""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [96, 101]                                   # whole tiles | a ragged last tile
DKS = [(5, 3), (32, 16), (128, 32)]              # padded | exact | the headline's kernel instances
OUTSIDE = (130, 8)                               # D > 128: not one of the LDS-resident forms


def _data(N, D, K):
    rng = np.random.default_rng(1000 * D + 10 * K + N)
    w = rng.standard_normal((D, K))
    x = rng.standard_normal((K, N))
    y = w @ x + 0.1 * rng.standard_normal((D, N))
    return y, rng.standard_normal((N, K))


def _switch(on):
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    rt.check(rt.lib.vmp_tune_set(b'pca_sweeps', 1 if on else 0))


@pytest.fixture(autouse=True)
def _restore_switch():
    yield
    _switch(True)


def _build(N, D, K, chunk=32, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from models import build_pca
    y, x0 = _data(N, D, K)
    Q = build_pca(nodes, VB, y, x0, K, **kw)
    plan = Q.plans[0]
    plan.sweep_chunk = chunk
    return Q, plan


def _snapshot(Q):
    n = Q.iter
    out = {'iter': n, 'converged': Q.converged, 'L': np.array(Q.L[:n])}
    for node in Q.model:
        out['l/' + node.name] = np.array(Q.l[node][:n])
    for name in ('W', 'tau', 'alpha'):
        for i, u in enumerate(Q[name].u):
            out['%s/u%d' % (name, i)] = np.array(u)
    out['X/u0'] = np.array(Q['X'].u[0])
    return out


def _assert_same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key


class sweep_counts:
    def __init__(self, plan):
        # plans of earlier tests are finalised now, not inside the counted window: PCAPlan.__del__
        # joins the plate stream of the shared context, which launches a pass that is held
        gc.collect()
        self.k = plan.kernels
        self.start = self.k.sweep_counts()
        self.pstart = self.k.pass_counts()

    def delta(self):
        return tuple(a - b for a, b in zip(self.k.sweep_counts(), self.start))

    def passes(self):
        return tuple(a - b for a, b in zip(self.k.pass_counts(), self.pstart))


_REF = {}


def _reference(N, D, K):
    """The per-iteration loop: update(repeat=7) on a fresh plan, then update(repeat=5)."""
    if (N, D, K) not in _REF:
        _switch(False)
        Q, plan = _build(N, D, K)
        c = sweep_counts(plan)
        Q.update(repeat=7, verbose=False)
        first = _snapshot(Q)
        Q.update(repeat=5, verbose=False)
        assert c.delta() == (0, 0, 0)
        _REF[N, D, K] = (first, _snapshot(Q))
        _switch(True)
    return _REF[N, D, K]


@pytest.mark.parametrize('chunk', [1, 3, 32])
@pytest.mark.parametrize('D,K', DKS)
@pytest.mark.parametrize('N', NS)
def test_batches_equal_the_per_iteration_loop(N, D, K, chunk):
    ref1, ref2 = _reference(N, D, K)
    Q, plan = _build(N, D, K, chunk)
    c = sweep_counts(plan)
    Q.update(repeat=7, verbose=False)
    # the first sweep of a fresh plan runs node by node, the other six as batches
    assert c.delta() == (6, 6, 0)
    assert c.passes() == (1, 6)
    _assert_same(_snapshot(Q), ref1)
    c = sweep_counts(plan)
    Q.update(repeat=5, verbose=False)
    assert c.delta() == (5, 5, 0)
    assert c.passes() == (1, 4)
    _assert_same(_snapshot(Q), ref2)


@pytest.mark.parametrize('N', NS)
def test_shape_outside_the_fast_forms_falls_back(N):
    D, K = OUTSIDE
    ref1, ref2 = _reference(N, D, K)
    Q, plan = _build(N, D, K)
    c = sweep_counts(plan)
    Q.update(repeat=7, verbose=False)
    _assert_same(_snapshot(Q), ref1)
    Q.update(repeat=5, verbose=False)
    _assert_same(_snapshot(Q), ref2)
    assert c.delta() == (0, 0, 0)
    assert c.passes() == (2, 10)


def find_stop(L, n):
    """From the bounds L[:n] of a per-iteration run: (s, tol, j) such that a loop which runs s
    iterations unchecked and then checks with ``tol`` -- halfway between the relative changes of
    two consecutive iterations of that run -- stops at iteration j (1-based), 2 < j < 10."""
    rel = {i + 1: (L[i] - L[i - 1]) / (0.5 * (abs(L[i - 1]) + abs(L[i]))) for i in range(1, n)}
    for j in range(9, 2, -1):                   # the latest such iteration, the shortest lead-in
        for s in range(1, j - 1):
            tol = 0.5 * (rel[j - 1] + rel[j])
            if rel[j] < tol and all(rel[i] >= tol for i in range(s + 1, j)):
                return s, tol, j
    raise AssertionError('no stopping point in %s' % rel)


@pytest.mark.parametrize('N,D,K', [(101, 32, 16), (96, 128, 32), (101, 5, 3)])
def test_early_stop_inside_a_chunk(N, D, K):
    _switch(False)
    P, _ = _build(N, D, K)
    P.update(repeat=12, verbose=False)
    s, tol, j = find_stop(P.L, 12)
    assert 2 < j < 10

    def run():
        Q, plan = _build(N, D, K)
        Q.update(repeat=s, verbose=False)
        Q.ignore_bound_checks = False
        c = sweep_counts(plan)
        Q.update(repeat=12, tol=tol, verbose=False)
        return Q, c
    R, c = run()
    assert R.iter == j and R.converged and c.delta() == (0, 0, 0)
    _switch(True)
    Q, c = run()
    assert Q.iter == j and Q.converged
    _assert_same(_snapshot(Q), _snapshot(R))
    # one chunk of 12: j - s sweeps ran, the rest of the chunk was skipped on the device
    assert c.delta() == (12, j - s, 12 - (j - s))
    assert c.passes()[0] == 1


def test_fallbacks_do_not_use_the_entry():
    N, D, K = 101, 32, 16

    def runs(on):
        _switch(on)
        out = []
        # a callback
        Q, plan = _build(N, D, K, callback=lambda: None)
        c = sweep_counts(plan)
        Q.update(repeat=4, verbose=False)
        out.append(_snapshot(Q))
        # another order of the nodes
        Q, plan = _build(N, D, K)
        Q.update(Q['X'], Q['W'], Q['tau'], Q['alpha'], repeat=4, verbose=False)
        out.append(_snapshot(Q))
        # streaming statistics
        Q, plan = _build(N, D, K)
        plan.stats = 'stream'
        Q.update(repeat=4, verbose=False)
        out.append(_snapshot(Q))
        assert c.delta() == (0, 0, 0)
        return out
    for a, b in zip(runs(True), runs(False)):
        _assert_same(a, b)


def test_autosave_inside_an_update_call(tmp_path):
    from bayespy_amd.inference.checkpoint import Reader
    N, D, K = 101, 32, 16

    def run(on, name):
        _switch(on)
        Q, plan = _build(N, D, K, autosave_filename=str(tmp_path / name), autosave_iterations=3)
        saved, save = {}, Q.save

        def spy(*a, **kw):
            save(*a, **kw)
            r = Reader(str(tmp_path / name))
            saved[Q.iter] = {k: np.array(r.get(k)) for k in r.keys()}
            r.close()
        Q.save = spy
        c = sweep_counts(plan)
        Q.update(repeat=7, verbose=False)
        return saved, _snapshot(Q), c.delta()
    ref, ref_end, d0 = run(False, 'ref.ckpt')
    new, new_end, d1 = run(True, 'new.ckpt')
    assert sorted(ref) == sorted(new) == [3, 6]
    assert d0 == (0, 0, 0) and d1 == (6, 6, 0)
    for it in (3, 6):
        assert sorted(ref[it]) == sorted(new[it])
        for key in ref[it]:
            if key != 'cputime':
                assert np.array_equal(ref[it][key], new[it][key], equal_nan=True), (it, key)
    _assert_same(ref_end, new_end)
