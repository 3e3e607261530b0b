"""
The one-launch sweep with the bound off the critical path, tune key "pca_sweep_defer" = 1 (default):
the tail hands over to the next head as soon as <tau>, <alpha>, Cov_X and sum <x><x>^T are ready;
<log tau>, <log alpha>, the bound, the ring slot and the stop rule are formed by one wavefront
beside the head's first inverse, from special-function values that are computed once per (priors,
D, plates, x_prec) and kept in the context.  A stop is read behind that inverse, before the head's
first store to the state.

None of this changes an expression or an order of accumulation, so EVERYTHING is compared bitwise
(np.array_equal / bytes), never with a tolerance, against each of
    "pca_sweep_defer" = 0       the tail computes the bound before the head starts,
    "pca_sweep_ticket" = 0      three launches per sweep:
the state block, every ring slot, the control words (through the counters), Q.L, the moments and
the <x> of the final pass.

N = 4096 and the shapes of test_pca_sweep_local_pxx_gpu.py (which explains their padding and ragged
groups).  A reference run is made once per (shape, form, scenario) and shared.
"""
import functools

import numpy as np
import pytest

from test_pca_sweep_ticket_gpu import _assert_same, _batches, _build, _snapshot, _tune, counts, find_stop

pytestmark = pytest.mark.gpu

N = 4096
DKS = [(128, 32), (96, 20), (40, 9), (32, 16), (20, 5)]
DEFER1, DEFER0, TICKET0 = 'deferred bound', 'bound in the tail', 'three launches'
REFS = (DEFER0, TICKET0)
SP_COUNT, SP_S_STATE, SP_S_RING = 19, 19, 20        # enum SP_* of csrc/vmp_pca_small.hip


def _select(form):
    _tune(b'pca_sweep_ticket', 0 if form == TICKET0 else 1)
    _tune(b'pca_sweep_wide', 1)
    _tune(b'pca_sweep_local_pxx', 1)
    _tune(b'pca_sweep_defer', 1 if form == DEFER1 else 0)


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    _tune(b'pca_sweep_ticket', 1)
    _tune(b'pca_sweep_wide', 1)
    _tune(b'pca_sweep_local_pxx', 1)
    _tune(b'pca_sweep_defer', 1)
    _tune(b'pca_sweep_stamps', 0)
    _tune(b'pca_sweeps', 1)


@functools.lru_cache(maxsize=None)
def _calls(form, D, K, repeats, chunk=32):
    """update calls on one fresh plan, a snapshot after each (the first sweep of a fresh plan runs
    node by node, the rest as chunks): the counters and the mid launches are checked on the way."""
    _select(form)
    Q, plan = _build(N, D, K, chunk)
    out = []
    for call, repeat in enumerate(repeats):
        swept = repeat - 1 if call == 0 else repeat
        c = counts(plan)
        Q.update(repeat=repeat, verbose=False)
        b = _batches(swept, chunk)
        out.append(_snapshot(Q, plan, ring=max(b)))
        assert c.delta() == (swept, swept, 0)
        assert c.passes()[0] == 1
        assert c.mid() == (0 if form == TICKET0 else sum(n - 1 for n in b))
    return tuple(out)


@pytest.mark.parametrize('ref', REFS)
@pytest.mark.parametrize('D,K', DKS)
def test_update_of_12_equals(D, K, ref):
    new, = _calls(DEFER1, D, K, (12,))
    old, = _calls(ref, D, K, (12,))
    assert new['iter'] == 12 and new['ring'].size == 8 * 11
    assert np.all(new['ring'].reshape(11, 8)[:, 7] == 1.0)          # every slot executed
    _assert_same(new, old)


@pytest.mark.parametrize('D,K', [(128, 32), (40, 9)])
def test_two_calls_on_one_plan_in_chunks_of_5(D, K):
    repeats = (12, 12)
    new = _calls(DEFER1, D, K, repeats, 5)                      # chunks 5 5 1 | 5 5 2
    for ref in REFS:
        for a, b in zip(new, _calls(ref, D, K, repeats, 5)):
            _assert_same(a, b)
    assert new[1]['iter'] == 24


@pytest.mark.parametrize('D,K', [(128, 32), (20, 5)])
def test_early_stop_inside_a_chunk(D, K):
    """The side work of sweep j of a chunk of 12 stops the loop while the head of sweep j + 1 is in
    its first inverse: that head must leave no trace.  The same executed and skipped counts, the
    later slots "not executed", the same state (every word of it, so also what the head would have
    stored) -- and the chunk of 4 after it is the reference's too."""
    _tune(b'pca_sweeps', 0)
    P, _ = _build(N, D, K)
    P.update(repeat=12, verbose=False)
    s, tol, j = find_stop(P.L, 12)
    assert 2 < j < 10                                   # strictly inside the chunk
    _tune(b'pca_sweeps', 1)

    def run(form):
        _select(form)
        Q, plan = _build(N, D, K)
        Q.update(repeat=s, verbose=False)
        Q.ignore_bound_checks = False
        c = counts(plan)
        Q.update(repeat=12, tol=tol, verbose=False)
        assert Q.iter == j and Q.converged
        assert c.delta() == (12, j - s, 12 - (j - s))
        assert c.mid() == (0 if form == TICKET0 else 11)
        first = _snapshot(Q, plan, ring=12)
        Q.ignore_bound_checks = True
        c = counts(plan)
        Q.update(repeat=4, verbose=False)
        assert c.delta() == (4, 4, 0) and c.mid() == (0 if form == TICKET0 else 3)
        return first, _snapshot(Q, plan, ring=4)
    new = run(DEFER1)
    ring = new[0]['ring'].reshape(12, 8)
    assert np.all(ring[:j - s, 7] == 1.0) and np.all(ring[j - s:, 7] == 0.0)
    for form in REFS:
        for a, b in zip(new, run(form)):
            _assert_same(a, b)


def test_checkpoint_saved_and_loaded_is_identical(tmp_path):
    """Q.save after 9, every entry of the file byte for byte ('cputime' is the host's clock), then
    Q.load into a fresh model and one more chunk: the bits of the tail that computes the bound."""
    from bayespy_amd.inference.checkpoint import Reader
    D, K = 96, 20

    def run(form, name):
        _select(form)
        Q, plan = _build(N, D, K, 5)
        Q.update(repeat=9, verbose=False)
        Q.save(filename=str(tmp_path / name))
        r = Reader(str(tmp_path / name))
        saved = {k: np.array(r.get(k)) for k in r.keys()}
        r.close()
        R, rplan = _build(N, D, K, 5)
        R.load(filename=str(tmp_path / name))
        R.update(repeat=5, verbose=False)
        return saved, _snapshot(R, rplan, ring=5)
    (new, cont), (ref, rcont) = run(DEFER1, 'defer.ckpt'), run(DEFER0, 'tail.ckpt')
    assert sorted(new) == sorted(ref)
    for key in new:
        if key != 'cputime':
            assert new[key].dtype == ref[key].dtype and new[key].shape == ref[key].shape, key
            assert new[key].tobytes() == ref[key].tobytes(), key
    _assert_same(cont, rcont)


def test_two_plans_with_different_priors_updated_alternately():
    """The cached special functions belong to (priors, D, plates, x_prec): two plans of one process
    that differ in all of a0, b0, D and K, updated in turn, each find the other's values in the
    context and must replace them.  Each is the same plan run alone with "pca_sweep_defer" = 0."""
    specs = [((128, 32), dict(a0=1e-2, b0=1e-2)), ((40, 9), dict(a0=3e-1, b0=7e-3))]

    def alone(spec):
        (D, K), kw = spec
        _select(DEFER0)
        Q, plan = _build(N, D, K, 5, **kw)
        out = []
        for repeat in (7, 6, 5):
            Q.update(repeat=repeat, verbose=False)
            out.append(_snapshot(Q, plan, ring=5))
        return out
    want = [alone(spec) for spec in specs]
    _select(DEFER1)
    built = [_build(N, D, K, 5, **kw) for (D, K), kw in specs]
    got = [[], []]
    for repeat in (7, 6, 5):
        for i, (Q, plan) in enumerate(built):
            Q.update(repeat=repeat, verbose=False)
            got[i].append(_snapshot(Q, plan, ring=5))
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            _assert_same(a, b)


def test_stamps_of_the_side_wavefront():
    """"pca_sweep_stamps" = 2: the rows also hold where the side wavefront stored the tau / alpha
    state and where it wrote the ring and the stop word; the results are the unstamped bits."""
    D, K = 128, 32
    off, = _calls(DEFER1, D, K, (12,))
    _tune(b'pca_sweep_stamps', 2)
    try:
        _select(DEFER1)
        Q, plan = _build(N, D, K)
        Q.update(repeat=12, verbose=False)
        on = _snapshot(Q, plan, ring=11)
        rows, allocated = plan.kernels.sweep_stamps()
    finally:
        _tune(b'pca_sweep_stamps', 0)
    _assert_same(on, off)
    assert allocated and rows.shape == (10, 24)
    for row in rows:
        t = row[:SP_COUNT]
        t = t[t != 0].astype(np.int64)
        assert t.size == 18 and np.all(np.diff(t) >= 0)
        assert row[SP_S_STATE] != 0 and row[SP_S_RING] >= row[SP_S_STATE]
        assert row[SP_S_STATE] >= t[0]
        assert np.all(row[SP_S_RING + 1:] == 0)
