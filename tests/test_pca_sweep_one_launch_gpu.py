"""
The one-launch held sweep (pca_sweep_mid_kernel) against three launches per sweep, which the tune key
"pca_sweep_ticket" = 0 selects and which is scalar code of its own.

In the one launch the chains of sum y<x>^T (phase A) run on v_mfma_f64_4x4x4_4b_f64 and the 8-row
partials of sum <x><x>^T (the tail) on v_mfma_f64_16x16x4_f64, both of which add their four products
to C in ascending order of the k-slots, every step fused (test_mfma_order_gpu.py); the workgroup that
runs phase B forms sum <x><x>^T from what it holds in LDS instead of adding stored partial blocks; and
<log tau>, <log alpha>, the bound, the ring slot and the stop rule are formed by one wavefront beside
the next head's first inverse, from special-function values that are computed once per (priors, D,
plates, x_prec) and kept in the context.  None of this changes an expression or an order of
accumulation, so EVERYTHING is compared bitwise (np.array_equal / bytes), never with a tolerance:
the state block, every ring slot, the control words (through the counters), Q.L, the moments and
the <x> of the final pass.

N = 4096.  Shapes: (128, 32) the headline's instance, 16 workgroups and four 16 x 16 tiles of
sum <x><x>^T; (96, 20) K < KP = 32 with K no multiple of 4 and DP = 128 > D, so padded columns, padded
rows and whole groups of rows beyond D; (40, 9) KP = 16, DP = 64, D no multiple of 32; (32, 16)
K = KP = 16, one tile, nothing padded; (20, 5) KP = 16 and a group that ends inside its 8 rows.
Phase A alone also runs at (33, 17) -- D is no multiple of 4, so the last matrix instruction of every
chain has k-slots beyond D, which must contribute exact zeros whatever the padding holds -- and at
(8, 3).  The chunk sweep runs at the N = 257 and the shapes of test_pca_sweep_ticket_gpu.py.
A reference run is made once per (shape, form, scenario) and shared.

The scenarios that test_pca_sweep_{defer,mfma,local_pxx}_gpu.py still run under their earlier names
are plain functions here (update_of_12, two_calls_in_chunks_of_5, ...), called by the tests of both.
"""
import functools

import numpy as np
import pytest

import test_pca_sweep_ticket_gpu as ticket_file
from test_pca_sweep_ticket_gpu import (_assert_same, _batches, _build, _snapshot, _tune, counts,
                                       find_stop, phase_a_alone)

pytestmark = pytest.mark.gpu

N = 4096
DKS = [(128, 32), (96, 20), (40, 9), (32, 16), (20, 5)]
ONE, THREE = 'one launch', 'three launches'
# enum SP_* of csrc/vmp_pca_small.hip
SP_T_PARTIALS, SP_T_LOADS, SP_T_PXX, SP_COUNT, SP_S_STATE, SP_S_RING = 6, 7, 8, 19, 19, 20


def _select(form, stamps=0):
    _tune(b'pca_sweep_ticket', 1 if form == ONE else 0)
    _tune(b'pca_sweep_stamps', stamps)


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    _tune(b'pca_sweep_ticket', 1)
    _tune(b'pca_sweep_stamps', 0)
    _tune(b'pca_sweeps', 1)


def _run_calls(form, n, D, K, repeats, chunk, stamps=0):
    """update calls on one fresh plan, a snapshot after each (the first sweep of a fresh plan runs
    node by node, the rest as chunks): the counters and the mid launches are checked on the way."""
    _select(form, stamps)
    Q, plan = _build(n, D, K, chunk)
    out = []
    for call, repeat in enumerate(repeats):
        swept = repeat - 1 if call == 0 else repeat
        c = counts(plan)
        Q.update(repeat=repeat, verbose=False)
        b = _batches(swept, chunk)
        out.append(_snapshot(Q, plan, ring=max(b)))
        assert c.delta() == (swept, swept, 0)
        assert c.passes()[0] == 1
        assert c.mid() == (sum(m - 1 for m in b) if form == ONE else 0)
    return tuple(out), plan


@functools.lru_cache(maxsize=None)
def _calls(form, D, K, repeats, chunk=32, n=N):
    return _run_calls(form, n, D, K, repeats, chunk)[0]


def update_of_12(D, K):
    new, = _calls(ONE, D, K, (12,))
    old, = _calls(THREE, D, K, (12,))
    assert new['iter'] == 12 and new['ring'].size == 8 * 11
    assert np.all(new['ring'].reshape(11, 8)[:, 7] == 1.0)          # every slot executed
    _assert_same(new, old)


@pytest.mark.parametrize('D,K', DKS)
def test_update_of_12_equals(D, K):
    update_of_12(D, K)


def two_calls_in_chunks_of_5(D, K):
    """Two update calls on one plan, the second of several chunks: every chunk after the first of
    the process draws from ticket words that only the kernels have put back to zero.  A word left
    non-zero would send no workgroup, or the wrong one, into phase B: the ring slots and the state
    would not be the reference's.  The mid launches are counted as before (in _run_calls)."""
    repeats = (12, 12)
    new = _calls(ONE, D, K, repeats, 5)                         # chunks 5 5 1 | 5 5 2
    for a, b in zip(new, _calls(THREE, D, K, repeats, 5)):
        _assert_same(a, b)
    assert new[1]['iter'] == 24


@pytest.mark.parametrize('D,K', [(128, 32), (40, 9)])
def test_two_calls_reuse_ticket_words_cleared_by_the_kernels(D, K):
    two_calls_in_chunks_of_5(D, K)


@pytest.mark.parametrize('chunk', [2, 5, 32])
@pytest.mark.parametrize('D,K', ticket_file.DKS)
def test_chunks_of_2_5_and_32_in_two_calls(D, K, chunk):
    # chunk 32: the first call is one full chunk of 32 sweeps (31 mid launches), the second one of 5
    repeats = (33, 5) if chunk == 32 else (7, 5)
    new = _calls(ONE, D, K, repeats, chunk, ticket_file.N)
    for a, b in zip(new, _calls(THREE, D, K, repeats, chunk, ticket_file.N)):
        _assert_same(a, b)


def early_stop_inside_a_chunk(D, K):
    """The side wavefront of sweep j of a chunk of 12 stops the loop while the head of sweep j + 1 is
    in its first inverse: that head must leave no trace.  The same executed and skipped counts, the
    later slots "not executed", the same state (every word of it, so also what the head would have
    stored) -- and the chunk of 4 after it, on the ticket words that chunk left (its stopped
    launches drew nothing), is the reference's too."""
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
        assert c.mid() == (11 if form == ONE else 0)
        first = _snapshot(Q, plan, ring=12)
        Q.ignore_bound_checks = True
        c = counts(plan)
        Q.update(repeat=4, verbose=False)
        assert c.delta() == (4, 4, 0) and c.mid() == (3 if form == ONE else 0)
        return first, _snapshot(Q, plan, ring=4)
    new = run(ONE)
    ring = new[0]['ring'].reshape(12, 8)
    assert np.all(ring[:j - s, 7] == 1.0) and np.all(ring[j - s:, 7] == 0.0)
    for a, b in zip(new, run(THREE)):
        _assert_same(a, b)


@pytest.mark.parametrize('D,K', [(128, 32), (20, 5)])
def test_early_stop_inside_a_chunk(D, K):
    early_stop_inside_a_chunk(D, K)


def checkpoint_saved_and_loaded(tmp_path, D, K):
    """Q.save after 9 (two chunks of 5), every entry of the file byte for byte ('cputime' is the
    host's clock and differs between any two runs, of one form too), then Q.load into a fresh model
    and one more chunk."""
    from bayespy_amd.inference.checkpoint import Reader

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
    (new, cont), (ref, rcont) = run(ONE, 'one.ckpt'), run(THREE, 'three.ckpt')
    assert sorted(new) == sorted(ref)
    for key in new:
        if key != 'cputime':
            assert new[key].dtype == ref[key].dtype and new[key].shape == ref[key].shape, key
            assert new[key].tobytes() == ref[key].tobytes(), key
    _assert_same(cont, rcont)


@pytest.mark.parametrize('D,K', [(96, 20), (128, 32)])
def test_checkpoint_saved_and_loaded_is_identical(tmp_path, D, K):
    checkpoint_saved_and_loaded(tmp_path, D, K)


def test_two_plans_with_different_priors_updated_alternately():
    """The cached special functions belong to (priors, D, plates, x_prec): two plans of one process
    that differ in all of a0, b0, D and K, updated in turn, each find the other's values in the
    context and must replace them.  Each is the same plan run alone with three launches per sweep,
    which reads no cached value."""
    specs = [((128, 32), dict(a0=1e-2, b0=1e-2)), ((40, 9), dict(a0=3e-1, b0=7e-3))]

    def alone(spec):
        (D, K), kw = spec
        _select(THREE)
        Q, plan = _build(N, D, K, 5, **kw)
        out = []
        for repeat in (7, 6, 5):
            Q.update(repeat=repeat, verbose=False)
            out.append(_snapshot(Q, plan, ring=5))
        return out
    want = [alone(spec) for spec in specs]
    _select(ONE)
    built = [_build(N, D, K, 5, **kw) for (D, K), kw in specs]
    got = [[], []]
    for repeat in (7, 6, 5):
        for i, (Q, plan) in enumerate(built):
            Q.update(repeat=repeat, verbose=False)
            got[i].append(_snapshot(Q, plan, ring=5))
    for g, w in zip(got, want):
        for a, b in zip(g, w):
            _assert_same(a, b)


def test_stamp_buffer_only_with_the_key_on():
    """The context is the process's, so whether it owns a stamp buffer depends on what ran before:
    the first check is therefore relative to the state found.  With the key off a run neither
    allocates the buffer (in a process that never had the key on: there is none before and none
    after) nor writes it; with it on every mid launch of the batch leaves a row of non-decreasing
    stamps and the results stay the same bits; off again, the rows are not written any more."""
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.pca import HIPKernels
    D, K, n = 128, 32, ticket_file.N
    rows0, allocated0 = HIPKernels(get_runtime()).sweep_stamps()
    off, plan = _run_calls(ONE, n, D, K, (7, 5), 5)
    rows, allocated = plan.kernels.sweep_stamps()
    assert allocated == allocated0 and np.array_equal(rows, rows0)
    if not allocated:
        assert rows.shape[0] == 0
    on, plan = _run_calls(ONE, n, D, K, (7, 5), 5, stamps=1)
    for a, b in zip(on, off):
        _assert_same(a, b)
    rows, allocated = plan.kernels.sweep_stamps()
    assert allocated and rows.shape == (4, 24)                  # the latest batch: 5 sweeps, 4 mid
    for row in rows:
        t = row[row != 0].astype(np.int64)
        assert t.size >= 17 and np.all(np.diff(t) >= 0)
    again, plan = _run_calls(ONE, n, D, K, (7, 5), 5)
    rows2, allocated = plan.kernels.sweep_stamps()
    assert allocated and np.array_equal(rows2, rows)
    for a, b in zip(again, off):
        _assert_same(a, b)


@functools.lru_cache(maxsize=None)
def _stamped(level):
    """update of 12 at the headline's instance with the stamped build: the snapshot and the rows"""
    (on,), plan = _run_calls(ONE, N, 128, 32, (12,), 32, stamps=level)
    rows, allocated = plan.kernels.sweep_stamps()
    assert allocated and rows.shape == (10, 24)
    return on, rows


@pytest.mark.parametrize('level', [1, 2])
def test_stamped_build_leaves_the_unstamped_bits(level):
    off, = _calls(ONE, 128, 32, (12,))
    _assert_same(_stamped(level)[0], off)


def rows_hold_18_stamps_ascending(level):
    for row in _stamped(level)[1]:
        t = row[:SP_COUNT]
        t = t[t != 0].astype(np.int64)
        assert t.size == 18 and np.all(np.diff(t) >= 0)


@pytest.mark.parametrize('level', [1, 2])
def test_every_row_holds_its_18_stamps_in_ascending_order(level):
    rows_hold_18_stamps_ascending(level)


def test_stamps_of_the_side_wavefront():
    """"pca_sweep_stamps" = 2: the rows also hold where the side wavefront stored the tau / alpha
    state and where it wrote the ring and the stop word; at 1 those words stay zero."""
    for row in _stamped(2)[1]:
        t = row[:SP_COUNT]
        t = t[t != 0].astype(np.int64)
        assert row[SP_S_STATE] != 0 and row[SP_S_RING] >= row[SP_S_STATE]
        assert row[SP_S_STATE] >= t[0]
        assert np.all(row[SP_S_RING + 1:] == 0)
    for row in _stamped(1)[1]:
        assert np.all(row[SP_COUNT:] == 0)


def test_stamp_at_pxx_formed_and_none_at_partials_summed():
    """The tail forms sum <x><x>^T after its loads have landed and adds no stored partial blocks: the
    "Pxx formed" boundary is in every row, "partial blocks summed" in none."""
    for row in _stamped(1)[1]:
        assert row[SP_T_PARTIALS] == 0 and row[SP_T_LOADS] != 0 and row[SP_T_PXX] >= row[SP_T_LOADS]
        t = row[row != 0].astype(np.int64)
        assert t.size == 18 and np.all(np.diff(t) >= 0)


@pytest.mark.parametrize('D,K', DKS + [(33, 17), (8, 3)])
def test_phase_a_alone_equals_the_three_launch_kernel(D, K):
    """Phase A through vmp_pca_gram_stats_form, form 1 against form 0, on random A and G: the whole
    state block bit for bit, Syx non-zero, and a workspace of NaN that form 1 leaves all NaN
    (phase_a_alone in test_pca_sweep_ticket_gpu.py)."""
    phase_a_alone(D, K, 11 * D + K)
