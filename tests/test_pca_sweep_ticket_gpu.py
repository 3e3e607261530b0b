"""
One launch per held sweep (pca_sweep_mid_kernel: Gram statistics on DP / 8 workgroups, tail and the
next sweep's head in the workgroup that draws the last ticket) against three launches per sweep,
which the tune key "pca_sweep_ticket" = 0 selects.  Every sum keeps its order, so EVERYTHING is
compared bitwise (np.array_equal), never with a tolerance: the state block, the ring, Q.L, the
moments, ``converged`` and ``iter``.

The counters belong to the process-wide context: every check is on deltas.
"""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 257
# the forms vmp_pca_sweep_covered accepts, the smallest that reach each, and ragged ones:
# KP = 16, DP = 32 (4 workgroups) | KP = 16 with a ragged 8-row group | KP = 32, DP = 64 with a
# ragged 32-row block | the headline's instance (16 workgroups)
DKS = [(8, 3), (20, 5), (33, 17), (128, 32)]
OUTSIDE = (130, 8)                               # D > 128: not one of the LDS-resident forms


def _data(N, D, K):
    rng = np.random.default_rng(1000 * D + 10 * K + N)
    w = rng.standard_normal((D, K))
    x = rng.standard_normal((K, N))
    y = w @ x + 0.1 * rng.standard_normal((D, N))
    return y, rng.standard_normal((N, K))


def _tune(key, value):
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    rt.check(rt.lib.vmp_tune_set(key, int(value)))


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    _tune(b'pca_sweep_ticket', 1)
    _tune(b'pca_sweeps', 1)


def _build(N, D, K, chunk=32, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from models import build_pca
    y, x0 = _data(N, D, K)
    Q = build_pca(nodes, VB, y, x0, K, **kw)
    plan = Q.plans[0]
    plan.sweep_chunk = chunk
    return Q, plan


def _snapshot(Q, plan=None, ring=0):
    n = Q.iter
    out = {'iter': n, 'converged': Q.converged, 'L': np.array(Q.L[:n])}
    for node in Q.model:
        out['l/' + node.name] = np.array(Q.l[node][:n])
    for name in ('W', 'tau', 'alpha'):
        for i, u in enumerate(Q[name].u):
            out['%s/u%d' % (name, i)] = np.array(u)
    out['X/u0'] = np.array(Q['X'].u[0])
    if plan is not None:
        plan.kernels.xjoin()
        plan.rt.sync_stream()
        out['state'] = plan.state.cpu().numpy().copy()
        if ring:
            out['ring'] = plan._sweep_ring[:8 * ring].cpu().numpy().copy()
    return out


def _assert_same(a, b):
    assert sorted(a) == sorted(b)
    for key in a:
        assert np.array_equal(np.asarray(a[key]), np.asarray(b[key]), equal_nan=True), key


class counts:
    def __init__(self, plan):
        # plans of earlier tests are finalised now, not inside the counted window (their __del__
        # joins the plate stream of the shared context, which launches a pass that is held)
        gc.collect()
        self.k = plan.kernels
        self.start = self.k.sweep_counts()
        self.pstart = self.k.pass_counts()
        self.mstart = self.k.sweep_mid_count()

    def delta(self):
        return tuple(a - b for a, b in zip(self.k.sweep_counts(), self.start))

    def passes(self):
        return tuple(a - b for a, b in zip(self.k.pass_counts(), self.pstart))

    def mid(self):
        return self.k.sweep_mid_count() - self.mstart


def _batches(n, chunk):
    return [min(chunk, n - i) for i in range(0, n, chunk)]


def _two_calls(ticket, N, D, K, chunk, repeats=(7, 5)):
    """update(repeat=7) on a fresh plan (the first sweep runs node by node, six as batches cut at
    `chunk`), then update(repeat=5): snapshots and the mid launches / passes of each call.  The
    ring is snapshot over the longest batch of the call: its first slots hold the last batch, the
    rest what the longest one left."""
    _tune(b'pca_sweep_ticket', ticket)
    Q, plan = _build(N, D, K, chunk)
    out = []
    for call, repeat in enumerate(repeats):
        swept = repeat - 1 if call == 0 else repeat
        c = counts(plan)
        Q.update(repeat=repeat, verbose=False)
        b = _batches(swept, chunk)
        snap = _snapshot(Q, plan, ring=max(b))
        assert c.delta() == (swept, swept, 0)
        assert c.passes()[0] == 1                               # one pass per call
        assert c.mid() == (sum(n - 1 for n in b) if ticket else 0)
        out.append(snap)
    return out


@pytest.mark.parametrize('chunk', [1, 2, 5, 32])
@pytest.mark.parametrize('D,K', DKS)
def test_one_launch_sweeps_equal_three_launch_sweeps(D, K, chunk):
    # chunks of 2 and 5 run several chunks back to back within a call (the ticket words are cleared
    # per chunk) and are cut by `repeat` (6 = 5 + 1, 5 = 2 + 2 + 1)
    ref = _two_calls(0, N, D, K, chunk)
    new = _two_calls(1, N, D, K, chunk)
    for a, b in zip(new, ref):
        _assert_same(a, b)


@pytest.mark.parametrize('D,K', [(20, 5), (128, 32)])            # KP = 16 | KP = 32
def test_full_chunks_of_32_sweeps(D, K):
    """Chunks of the full default length: update(repeat=33) on a fresh plan is one chunk of 32
    sweeps -- 31 mid launches on ticket words 0 .. 30, the ring at its full length -- and
    update(repeat=40) a full chunk and a remainder of 8, 31 + 7 mid launches (asserted in
    _two_calls); state, ring and bounds bitwise against three launches per sweep."""
    assert _batches(32, 32) == [32] and _batches(40, 32) == [32, 8]
    ref = _two_calls(0, N, D, K, 32, repeats=(33, 40))
    new = _two_calls(1, N, D, K, 32, repeats=(33, 40))
    assert new[0]['ring'].size == 8 * 32 and new[0]['iter'] == 33 and new[1]['iter'] == 73
    assert np.all(new[1]['ring'].reshape(32, 8)[:, 7] == 1.0)            # every slot executed
    for a, b in zip(new, ref):
        _assert_same(a, b)


def test_shape_outside_the_fast_forms_has_no_mid_launch():
    D, K = OUTSIDE
    Q, plan = _build(N, D, K)
    c = counts(plan)
    Q.update(repeat=4, verbose=False)
    assert c.delta() == (0, 0, 0) and c.mid() == 0


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


@pytest.mark.parametrize('D,K', [(20, 5), (128, 32)])
def test_early_stop_inside_a_chunk(D, K):
    """The stop is at sweep j of a chunk of 12: the head of sweep j + 1 must not have run (the state
    is what the per-iteration loop leaves) and the later launches of the chunk draw no ticket."""
    _tune(b'pca_sweeps', 0)
    P, _ = _build(N, D, K)
    P.update(repeat=12, verbose=False)
    s, tol, j = find_stop(P.L, 12)
    assert 2 < j < 10

    def run():
        Q, plan = _build(N, D, K)
        Q.update(repeat=s, verbose=False)
        Q.ignore_bound_checks = False
        c = counts(plan)
        Q.update(repeat=12, tol=tol, verbose=False)
        return Q, plan, c
    R, rplan, c = run()                                          # the per-iteration loop
    assert R.iter == j and R.converged and c.delta() == (0, 0, 0) and c.mid() == 0
    loop = _snapshot(R, rplan)
    _tune(b'pca_sweeps', 1)
    _tune(b'pca_sweep_ticket', 0)
    T, tplan, c = run()
    assert c.delta() == (12, j - s, 12 - (j - s)) and c.mid() == 0
    three = _snapshot(T, tplan, ring=12)
    _tune(b'pca_sweep_ticket', 1)
    Q, plan, c = run()
    assert Q.iter == j and Q.converged
    assert c.delta() == (12, j - s, 12 - (j - s)) and c.mid() == 11
    assert c.passes()[0] == 1
    one = _snapshot(Q, plan, ring=12)
    _assert_same(one, three)
    for key in loop:
        if key != 'state':          # (the loop's state block is compared through the moments)
            assert np.array_equal(np.asarray(one[key]), np.asarray(loop[key]), equal_nan=True), key
    # what the head of sweep j + 1 would have overwritten is what the loop left
    L = plan.layout
    for off, n in ((L.off_W, D * L.KP), (L.off_CW, L.KP * L.KP), (L.off_Sww, L.KP * L.KP),
                   (L.off_CX, L.KP * L.KP), (L.off_A, L.KP * L.DP)):
        assert np.array_equal(one['state'][off:off + n], loop['state'][off:off + n]), off


def phase_a_alone(D, K, seed):
    """Phase A of the one-launch sweep through its stand-alone entry (form 1 of
    vmp_pca_gram_stats_form) against pca_gram_stats_kernel (form 0) on random A and G, padding
    included (so a chain that read a padded column or kept a padded row would show): the whole
    state block, with the Syx rows in it, bit for bit.  Form 0 also leaves the DP / 8 partial blocks
    of sum <x><x>^T in the workspace and nothing behind them; form 1 forms no partial blocks and must
    leave the workspace, filled with NaN here, untouched.  Returns the layout, the host block the
    two started from and the state form 1 left."""
    from bayespy_amd.device import get_runtime, ptr
    from bayespy_amd.inference.plans.pca import HIPKernels
    rt = get_runtime()
    k = HIPKernels(rt)
    L = k.layout(D, K)
    DP, KP = int(L.DP), int(L.KP)
    nb = DP // 8
    rng = np.random.default_rng(seed)
    host = np.zeros(int(L.total))
    host[L.off_A:L.off_A + KP * DP] = rng.standard_normal(KP * DP)
    host[L.off_G:L.off_G + DP * DP] = rng.standard_normal(DP * DP)
    torch = rt.torch
    got = []
    for form in (0, 1):
        st = torch.from_numpy(host.copy()).to(rt.device)
        ws = rt.zeros(int(k.workspace_doubles(D, K)))
        ws.fill_(float('nan'))
        rt.sync_stream()
        rt.check(rt.lib.vmp_pca_gram_stats_form(k.ctx, D, K, ptr(st), ptr(ws), form))
        rt.sync_stream()
        got.append((st.cpu().numpy().copy(), ws.cpu().numpy().copy()))
    (s0, p0), (s1, p1) = got
    assert np.array_equal(s0, s1)
    assert not np.isnan(p0[:nb * KP * KP]).any() and np.isnan(p0[nb * KP * KP:]).all()
    assert np.isnan(p1).all()
    syx = s1[L.off_S:L.off_S + DP * KP].reshape(DP, KP)[:D, :K]
    assert np.any(syx != 0.0)
    return L, host, s1


@pytest.mark.parametrize('D,K', DKS)
def test_gram_statistics_body_alone_equals_the_old_kernel(D, K):
    """Forms 1 and 0 of vmp_pca_gram_stats_form bit for bit (phase_a_alone), and the statistics are
    what they say: Syx = G A^T on the unpadded block."""
    L, host, s1 = phase_a_alone(D, K, 7 * D + K)
    DP, KP = int(L.DP), int(L.KP)
    A = host[L.off_A:L.off_A + KP * DP].reshape(KP, DP)
    G = host[L.off_G:L.off_G + DP * DP].reshape(DP, DP)
    want = G[:D, :D] @ A[:K, :D].T
    np.testing.assert_allclose(s1[L.off_S:L.off_S + DP * KP].reshape(DP, KP)[:D, :K], want,
                               rtol=0, atol=1e-12 * D * np.abs(want).max())


def test_gram_statistics_form_out_of_range_is_an_error():
    from bayespy_amd._lib import VMP_ERR_INVALID
    from bayespy_amd.device import get_runtime, ptr
    from bayespy_amd.inference.plans.pca import HIPKernels
    rt = get_runtime()
    k = HIPKernels(rt)
    st = rt.zeros(int(k.layout(8, 3).total))
    ws = rt.zeros(int(k.workspace_doubles(8, 3)))
    for form in (-1, 2, 3):
        assert rt.lib.vmp_pca_gram_stats_form(k.ctx, 8, 3, ptr(st), ptr(ws), form) == VMP_ERR_INVALID
