"""
The one-launch sweep with its Gram products on the matrix cores, tune key "pca_sweep_mfma" = 1
(default): the chains of sum y<x>^T in phase A run on v_mfma_f64_4x4x4_4b_f64 and the 8-row partials
of sum <x><x>^T in the tail on v_mfma_f64_16x16x4_f64, instead of scalar fused multiply-adds fed from
LDS.  Both instructions add their four products to C in ascending order of the k-slots, every step
fused (test_mfma_order_gpu.py), so no chain changes and EVERYTHING is compared bitwise
(np.array_equal / bytes), never with a tolerance, against each of
    "pca_sweep_mfma" = 0        the scalar chains in the same launch,
    "pca_sweep_ticket" = 0      three launches per sweep:
the state block, every ring slot, the control words (through the counters), Q.L, the moments and
the <x> of the final pass.

N = 4096 and the shapes of test_pca_sweep_defer_gpu.py: (128, 32) the headline's instance, 16
workgroups and four 16 x 16 tiles of sum <x><x>^T; (96, 20) K < KP = 32 and DP = 128 > D, so padded
columns, padded rows and whole groups of rows beyond D; (40, 9) KP = 16, D no multiple of 32;
(32, 16) K = KP = 16, one tile, nothing padded; (20, 5) KP = 16 and a group that ends inside its 8
rows.  Phase A alone also runs at (33, 17): D is no multiple of 4, so the last matrix instruction
of every chain has k-slots beyond D, which must contribute exact zeros whatever the padding holds.
A reference run is made once per (shape, form, scenario) and shared.
"""
import functools

import numpy as np
import pytest

from test_pca_sweep_ticket_gpu import _assert_same, _batches, _build, _snapshot, _tune, counts, find_stop

pytestmark = pytest.mark.gpu

N = 4096
DKS = [(128, 32), (96, 20), (40, 9), (32, 16), (20, 5)]
MFMA1, MFMA0, TICKET0 = 'matrix cores', 'scalar chains', 'three launches'
REFS = (MFMA0, TICKET0)
SP_COUNT = 19                                       # enum SP_* of csrc/vmp_pca_small.hip


def _select(form):
    _tune(b'pca_sweep_ticket', 0 if form == TICKET0 else 1)
    _tune(b'pca_sweep_wide', 1)
    _tune(b'pca_sweep_local_pxx', 1)
    _tune(b'pca_sweep_defer', 1)
    _tune(b'pca_sweep_mfma', 1 if form == MFMA1 else 0)


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    _tune(b'pca_sweep_ticket', 1)
    _tune(b'pca_sweep_wide', 1)
    _tune(b'pca_sweep_local_pxx', 1)
    _tune(b'pca_sweep_defer', 1)
    _tune(b'pca_sweep_mfma', 1)
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
    new, = _calls(MFMA1, D, K, (12,))
    old, = _calls(ref, D, K, (12,))
    assert new['iter'] == 12 and new['ring'].size == 8 * 11
    assert np.all(new['ring'].reshape(11, 8)[:, 7] == 1.0)          # every slot executed
    _assert_same(new, old)


@pytest.mark.parametrize('D,K', [(128, 32), (40, 9)])
def test_two_calls_on_one_plan_in_chunks_of_5(D, K):
    repeats = (12, 12)
    new = _calls(MFMA1, D, K, repeats, 5)                       # chunks 5 5 1 | 5 5 2
    for ref in REFS:
        for a, b in zip(new, _calls(ref, D, K, repeats, 5)):
            _assert_same(a, b)
    assert new[1]['iter'] == 24


@pytest.mark.parametrize('D,K', [(128, 32), (20, 5)])
def test_early_stop_inside_a_chunk(D, K):
    """A stop at sweep j of a chunk of 12, strictly inside it: the same executed and skipped counts,
    the later slots "not executed", the same state -- and the chunk of 4 after it is the
    reference's too."""
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
    new = run(MFMA1)
    ring = new[0]['ring'].reshape(12, 8)
    assert np.all(ring[:j - s, 7] == 1.0) and np.all(ring[j - s:, 7] == 0.0)
    for form in REFS:
        for a, b in zip(new, run(form)):
            _assert_same(a, b)


def test_checkpoint_saved_and_loaded_is_identical(tmp_path):
    """Q.save after 9, every entry of the file byte for byte ('cputime' is the host's clock), then
    Q.load into a fresh model and one more chunk."""
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
    (new, cont), (ref, rcont) = run(MFMA1, 'mfma.ckpt'), run(MFMA0, 'scalar.ckpt')
    assert sorted(new) == sorted(ref)
    for key in new:
        if key != 'cputime':
            assert new[key].dtype == ref[key].dtype and new[key].shape == ref[key].shape, key
            assert new[key].tobytes() == ref[key].tobytes(), key
    _assert_same(cont, rcont)


def test_stamped_build():
    """"pca_sweep_stamps" = 2 with the matrix-core products: the unstamped bits, and every row holds
    the 18 stamps of the workgroup that ran phase B in ascending order."""
    D, K = 128, 32
    off, = _calls(MFMA1, D, K, (12,))
    _tune(b'pca_sweep_stamps', 2)
    try:
        _select(MFMA1)
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


@pytest.mark.parametrize('D,K', DKS + [(33, 17)])
def test_phase_a_alone_equals_the_scalar_bodies(D, K):
    """Phase A through vmp_pca_gram_stats_form on random A and G, padding included (so a chain that
    read a padded column or kept a padded row would show): form 3, Syx on the matrix cores, against
    form 2, the scalar wide body, and form 0, the kernel every other path uses -- the Syx rows in
    the state and the partial blocks of sum <x><x>^T, bit for bit."""
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
    torch = rt.torch
    got = []
    for form in (3, 2, 0):
        st = torch.from_numpy(host.copy()).to(rt.device)
        ws = rt.zeros(int(k.workspace_doubles(D, K)))
        ws.fill_(float('nan'))
        rt.sync_stream()
        rt.check(rt.lib.vmp_pca_gram_stats_form(k.ctx, D, K, ptr(st), ptr(ws), form))
        rt.sync_stream()
        got.append((st.cpu().numpy().copy(), ws[:nb * KP * KP + 64].cpu().numpy().copy()))
    (s3, p3), (s2, p2), (s0, p0) = got
    assert np.array_equal(s3, s2) and np.array_equal(s3, s0)
    assert np.array_equal(p3, p2, equal_nan=True) and np.array_equal(p3, p0, equal_nan=True)
    assert not np.isnan(p3[:nb * KP * KP]).any() and np.isnan(p3[nb * KP * KP:]).all()
    syx = s3[L.off_S:L.off_S + DP * KP].reshape(DP, KP)[:D, :K]
    assert np.any(syx != 0.0)
