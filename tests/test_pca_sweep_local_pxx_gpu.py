"""
The one-launch sweep with sum <x><x>^T formed by the workgroup that runs phase B, tune key
"pca_sweep_local_pxx" = 1 (default): phase A stores no partial blocks, the tail forms every group's
partial from the A and the rows of sum y<x>^T it holds in LDS and adds the partials in the order of
reduce_partials_kernel.  The ticket words are put back to zero by the kernels (no memset per chunk),
and the first head of a chunk runs the wide head body in a launch of its own.

None of this changes an expression or an order of accumulation, so EVERYTHING is compared bitwise
(np.array_equal / bytes), never with a tolerance, against each of
    "pca_sweep_local_pxx" = 0   the partial blocks travel through memory,
    "pca_sweep_wide" = 0        the bodies of the three-launch sweep inside the launch,
    "pca_sweep_ticket" = 0      three launches per sweep:
the state block, every ring slot, Q.L, the moments and the <x> of the final pass.

N = 4096.  Shapes: (128, 32) the headline's; (96, 20) DP = 128, KP = 32 with K no multiple of 4 and
a 32-row block of padding; (40, 9) DP = 64, KP = 16 with three 8-row groups of padding; (32, 16) no
padding at all; and (20, 5), a ragged 8-row group.  A reference run is made once per (shape, form,
scenario) and shared.
"""
import functools

import numpy as np
import pytest

from test_pca_sweep_ticket_gpu import _assert_same, _batches, _build, _snapshot, _tune, counts, find_stop

pytestmark = pytest.mark.gpu

N = 4096
DKS = [(128, 32), (96, 20), (40, 9), (32, 16), (20, 5)]
LOCAL1, LOCAL0, WIDE0, TICKET0 = 'local Pxx', 'partial blocks', 'old bodies', 'three launches'
REFS = (LOCAL0, WIDE0, TICKET0)


def _select(form):
    _tune(b'pca_sweep_ticket', 0 if form == TICKET0 else 1)
    _tune(b'pca_sweep_wide', 0 if form == WIDE0 else 1)
    _tune(b'pca_sweep_local_pxx', 1 if form == LOCAL1 else 0)


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    _tune(b'pca_sweep_ticket', 1)
    _tune(b'pca_sweep_wide', 1)
    _tune(b'pca_sweep_local_pxx', 1)
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
    new, = _calls(LOCAL1, D, K, (12,))
    old, = _calls(ref, D, K, (12,))
    assert new['iter'] == 12 and new['ring'].size == 8 * 11
    assert np.all(new['ring'].reshape(11, 8)[:, 7] == 1.0)          # every slot executed
    _assert_same(new, old)


@pytest.mark.parametrize('D,K', [(128, 32), (40, 9)])
def test_two_calls_reuse_ticket_words_cleared_by_the_kernels(D, K):
    """Two update calls on one plan, the second of several chunks: every chunk after the first of
    the process draws from ticket words that only the kernels have put back to zero.  A word left
    non-zero would send no workgroup, or the wrong one, into phase B: the ring slots and the state
    would not be the reference's.  The mid launches are counted as before (in _calls)."""
    repeats = (12, 12)
    new = _calls(LOCAL1, D, K, repeats, 5)                      # chunks 5 5 1 | 5 5 2
    for ref in REFS:
        for a, b in zip(new, _calls(ref, D, K, repeats, 5)):
            _assert_same(a, b)
    assert new[1]['iter'] == 24


@pytest.mark.parametrize('D,K', [(128, 32), (20, 5)])
def test_early_stop_inside_a_chunk(D, K):
    """The tail of sweep j of a chunk of 12 stops the loop: the same executed and skipped counts,
    the later slots "not executed", the same state -- and the chunk after it, on the ticket words
    that chunk left (its stopped launches drew nothing), is the reference's too."""
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
    new = run(LOCAL1)
    ring = new[0]['ring'].reshape(12, 8)
    assert np.all(ring[:j - s, 7] == 1.0) and np.all(ring[j - s:, 7] == 0.0)
    for form in REFS:
        for a, b in zip(new, run(form)):
            _assert_same(a, b)


def test_checkpoint_saved_and_loaded_is_identical(tmp_path):
    """Q.save after two chunks, every entry of the file byte for byte ('cputime' is the host's clock),
    then Q.load into a fresh model and one more chunk: the parent path's bits."""
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
    (new, cont), (ref, rcont) = run(LOCAL1, 'local.ckpt'), run(LOCAL0, 'blocks.ckpt')
    assert sorted(new) == sorted(ref)
    for key in new:
        if key != 'cputime':
            assert new[key].dtype == ref[key].dtype and new[key].shape == ref[key].shape, key
            assert new[key].tobytes() == ref[key].tobytes(), key
    _assert_same(cont, rcont)


def test_stamped_build_is_the_same_code_with_a_stamp_at_pxx_formed():
    """The stamped build of the local form leaves one row per mid launch, non-decreasing, with the
    "Pxx formed" boundary in it and no "partial blocks summed"; the results are the unstamped bits."""
    D, K = 128, 32
    off, = _calls(LOCAL1, D, K, (12,))
    _tune(b'pca_sweep_stamps', 1)
    try:
        _select(LOCAL1)
        Q, plan = _build(N, D, K)
        Q.update(repeat=12, verbose=False)
        on = _snapshot(Q, plan, ring=11)
        rows, allocated = plan.kernels.sweep_stamps()
    finally:
        _tune(b'pca_sweep_stamps', 0)
    _assert_same(on, off)
    assert allocated and rows.shape == (10, 24)
    SP_T_PARTIALS, SP_T_LOADS, SP_T_PXX = 6, 7, 8              # enum SP_* of csrc/vmp_pca_small.hip
    for row in rows:
        assert row[SP_T_PARTIALS] == 0 and row[SP_T_LOADS] != 0 and row[SP_T_PXX] >= row[SP_T_LOADS]
        t = row[row != 0].astype(np.int64)
        assert t.size == 18 and np.all(np.diff(t) >= 0)
