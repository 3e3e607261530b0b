"""
Phase B of the one-launch sweep (pca_sweep_mid_kernel) with the wide tail and head bodies, tune key
"pca_sweep_wide" = 1 (default), against the bodies of the three-launch sweep inside the same launch
("pca_sweep_wide" = 0) and against three launches per sweep ("pca_sweep_ticket" = 0).  Only data
movement and scheduling differ, so EVERYTHING is compared bitwise (np.array_equal), never with a
tolerance: the state block, the ring, Q.L, the moments, ``converged`` and ``iter``.

Phase A of the wide launch is a body of its own as well: form 2 of vmp_pca_gram_stats_form, against
form 0.  The helpers, N = 257 and the four shapes are those of test_pca_sweep_ticket_gpu.py.
"""
import numpy as np
import pytest

from test_pca_sweep_ticket_gpu import (DKS, N, _assert_same, _batches, _build, _snapshot, _tune,
                                       counts, find_stop)

pytestmark = pytest.mark.gpu

TICKET0, WIDE0, WIDE1 = 'three launches', 'one launch, old bodies', 'one launch, wide bodies'


def _select(form, stamps=0):
    _tune(b'pca_sweep_ticket', 0 if form == TICKET0 else 1)
    _tune(b'pca_sweep_wide', 1 if form == WIDE1 else 0)
    _tune(b'pca_sweep_stamps', stamps)


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    _tune(b'pca_sweep_ticket', 1)
    _tune(b'pca_sweep_wide', 1)
    _tune(b'pca_sweep_stamps', 0)
    _tune(b'pca_sweeps', 1)


def _two_calls(form, D, K, chunk, repeats, stamps=0):
    """Two update calls on a fresh plan, a snapshot after each (the first sweep of a fresh plan runs
    node by node, the rest as batches cut at `chunk`)."""
    _select(form, stamps)
    Q, plan = _build(N, D, K, chunk)
    out = []
    for call, repeat in enumerate(repeats):
        swept = repeat - 1 if call == 0 else repeat
        c = counts(plan)
        Q.update(repeat=repeat, verbose=False)
        b = _batches(swept, chunk)
        out.append(_snapshot(Q, plan, ring=max(b)))
        assert c.delta() == (swept, swept, 0)
        assert c.mid() == (0 if form == TICKET0 else sum(n - 1 for n in b))
    return out, plan


@pytest.mark.parametrize('chunk', [2, 5, 32])
@pytest.mark.parametrize('D,K', DKS)
def test_wide_bodies_equal_old_bodies_and_three_launches(D, K, chunk):
    # chunk 32: the first call is one full chunk of 32 sweeps (31 mid launches), the second one of 5
    repeats = (33, 5) if chunk == 32 else (7, 5)
    new, _ = _two_calls(WIDE1, D, K, chunk, repeats)
    for form in (WIDE0, TICKET0):
        ref, _ = _two_calls(form, D, K, chunk, repeats)
        for a, b in zip(new, ref):
            _assert_same(a, b)


@pytest.mark.parametrize('D,K', [(20, 5), (128, 32)])
def test_early_stop_inside_a_chunk(D, K):
    """The tail of sweep j of a chunk of 12 stops the loop: the wide head of sweep j + 1 must not have
    stored anything (state, control block and counters are the reference's) and the later sweeps of
    the chunk are marked "not executed"."""
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
        return _snapshot(Q, plan, ring=12)
    new = run(WIDE1)
    ring = new['ring'].reshape(12, 8)
    assert np.all(ring[:j - s, 7] == 1.0) and np.all(ring[j - s:, 7] == 0.0)
    for form in (WIDE0, TICKET0):
        _assert_same(new, run(form))


def test_saved_checkpoint_is_identical(tmp_path):
    """Q.save after two chunks: every entry of the file byte for byte ('cputime' is the host's clock
    and differs between any two runs, of one form too)."""
    from bayespy_amd.inference.checkpoint import Reader
    D, K = 128, 32

    def run(form, name):
        _select(form)
        Q, plan = _build(N, D, K, 5)
        Q.update(repeat=9, verbose=False)
        Q.save(filename=str(tmp_path / name))
        r = Reader(str(tmp_path / name))
        out = {k: np.array(r.get(k)) for k in r.keys()}
        r.close()
        return out
    new, ref = run(WIDE1, 'wide.ckpt'), run(WIDE0, 'old.ckpt')
    assert sorted(new) == sorted(ref)
    for key in new:
        if key != 'cputime':
            assert new[key].dtype == ref[key].dtype and new[key].shape == ref[key].shape, key
            assert new[key].tobytes() == ref[key].tobytes(), key


def test_stamp_buffer_only_with_the_key_on():
    """The context is the process's, so whether it owns a stamp buffer depends on what ran before:
    the first check is therefore relative to the state found.  With the key off a run neither
    allocates the buffer (in a process that never had the key on: there is none before and none
    after) nor writes it; with it on every mid launch of the batch leaves a row of non-decreasing
    stamps and the results stay the same bits; off again, the rows are not written any more."""
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.pca import HIPKernels
    D, K = 128, 32
    rows0, allocated0 = HIPKernels(get_runtime()).sweep_stamps()
    off, plan = _two_calls(WIDE1, D, K, 5, (7, 5))
    rows, allocated = plan.kernels.sweep_stamps()
    assert allocated == allocated0 and np.array_equal(rows, rows0)
    if not allocated:
        assert rows.shape[0] == 0
    on, plan = _two_calls(WIDE1, D, K, 5, (7, 5), stamps=1)
    for a, b in zip(on, off):
        _assert_same(a, b)
    rows, allocated = plan.kernels.sweep_stamps()
    assert allocated and rows.shape == (4, 24)                  # the latest batch: 5 sweeps, 4 mid
    for row in rows:
        t = row[row != 0].astype(np.int64)
        assert t.size >= 17 and np.all(np.diff(t) >= 0)
    again, plan = _two_calls(WIDE1, D, K, 5, (7, 5))
    rows2, allocated = plan.kernels.sweep_stamps()
    assert allocated and np.array_equal(rows2, rows)
    for a, b in zip(again, off):
        _assert_same(a, b)


@pytest.mark.parametrize('D,K', DKS)
def test_wide_phase_a_alone_equals_the_old_kernel(D, K):
    """Phase A of the wide launch through its stand-alone entry (form 2) against pca_gram_stats_kernel
    (form 0) and against the body of "pca_sweep_wide" = 0 (form 1) on random A and G, padding
    included: the state block with the Syx rows and the partial blocks, bit for bit, and nothing
    written behind the last block."""
    from bayespy_amd.device import get_runtime, ptr
    from bayespy_amd.inference.plans.pca import HIPKernels
    rt = get_runtime()
    k = HIPKernels(rt)
    L = k.layout(D, K)
    DP, KP = int(L.DP), int(L.KP)
    nb = DP // 8
    rng = np.random.default_rng(11 * D + K)
    host = np.zeros(int(L.total))
    host[L.off_A:L.off_A + KP * DP] = rng.standard_normal(KP * DP)
    host[L.off_G:L.off_G + DP * DP] = rng.standard_normal(DP * DP)
    got = []
    for form in (0, 1, 2):
        st = rt.torch.from_numpy(host.copy()).to(rt.device)
        ws = rt.zeros(int(k.workspace_doubles(D, K)))
        ws.fill_(float('nan'))
        rt.sync_stream()
        rt.check(rt.lib.vmp_pca_gram_stats_form(k.ctx, D, K, ptr(st), ptr(ws), form))
        rt.sync_stream()
        got.append((st.cpu().numpy().copy(), ws[:nb * KP * KP + 64].cpu().numpy().copy()))
    s0, p0 = got[0]
    assert not np.array_equal(s0, host)                 # (the statistics were written at all)
    for s, p in got[1:]:
        assert np.array_equal(s, s0)
        assert np.array_equal(p, p0, equal_nan=True)
        assert not np.isnan(p[:nb * KP * KP]).any() and np.isnan(p[nb * KP * KP:]).all()
