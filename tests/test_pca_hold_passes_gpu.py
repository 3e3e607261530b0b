"""
Held latent passes of the Gram-form PCA block (vmp_pca_hold_passes): a pass whose <x> the next
pass overwrites before anything can read it is never launched; every pass whose <x> can be read
is, bit for bit as without holding.

Everything is compared BITWISE (torch.equal / np.array_equal) against the same call sequence
with holding off: holding changes which launches happen, never what a launch computes.  The
counters (vmp_pca_pass_counts) belong to the process-wide context, so every check is on deltas.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (N, D, K, layout): exact instance, tile-major | guarded, row-major | fewer tiles than the four
# wavefronts of one workgroup | ragged last tile (row-major, unpadded: fast + guarded launch)
SHAPES = [(3000, 128, 32, 'tiled'), (1500, 50, 9, 'rows'), (100, 64, 16, 'tiled'),
          (2049, 128, 32, 'rows')]
SENTINEL = -7.25


class Block:
    """Device arrays of one PCA block, set up through the C ABI alone."""

    def __init__(self, N, D, K, layout, seed=0):
        import torch
        from bayespy_amd.device import get_runtime
        from bayespy_amd.inference.plans.pca import HIPKernels
        self.rt = rt = get_runtime()
        self.k = k = HIPKernels(rt)
        self.N, self.D, self.K, self.tiled = N, D, K, layout == 'tiled'
        self.L = L = k.layout(D, K)
        self.KP, self.DP = int(L.KP), int(L.DP)
        # tile-major Y: X has whole tiles; row-major: no padding, so that N = 2049 has a ragged tile
        self.ld = (N + 31) // 32 * 32 if self.tiled else N + (N & 1)
        g = torch.Generator(device=rt.device)
        g.manual_seed(1000 + seed + N)
        self.g = g
        self.Y = rt.zeros(D, self.ld)
        self.Y[:, :N] = torch.randn(D, N, generator=g, device=rt.device, dtype=torch.float64)
        self.state = rt.zeros(int(L.total))
        self.ws = rt.empty(int(k.workspace_doubles(D, K)))
        rt.sync_stream()
        k.init_state(D, K, 1e-2, 1e-2, 1e-2, 1e-2, self.state)
        k.gram(self.Y, self.ld, N, D, K, self.state, self.ws)
        self.Yt = k.tile_y(self.Y, self.ld, N, D, K) if self.tiled else None
        self.As = [self.random_A() for _ in range(3)]

    def random_A(self):
        import torch
        A = self.rt.zeros(self.KP, self.DP)
        A[:self.K, :self.D] = torch.randn(self.K, self.D, generator=self.g, device=self.rt.device,
                                          dtype=torch.float64)
        return A.reshape(-1)

    def new_x(self):
        X = self.rt.empty(self.KP, self.ld)
        X.fill_(SENTINEL)
        return X

    def xpass(self, A, X):
        """One latent pass with A in the state; returns a copy of S."""
        L = self.L
        self.state[L.off_A:L.off_A + self.KP * self.DP].copy_(A)
        if self.tiled:
            self.k.xpass_tiled(self.Yt, self.N, self.D, self.K, X, self.ld, self.state, self.ws)
        else:
            self.k.xpass(self.Y, self.ld, self.N, self.D, self.K, X, self.ld, self.state, self.ws)
        self.k.ensure_gram()
        return self.state[L.off_S:L.off_S + L.len_S].clone()

    def eager(self, A):
        """(X, S) of a launched pass with A, holding off."""
        import torch
        X = self.new_x()
        S = self.xpass(A, X)
        self.k.xjoin()
        torch.cuda.synchronize()
        return X, S


class counts:
    """Delta of (launched, superseded) over a block of code."""

    def __init__(self, k):
        self.k = k

    def __enter__(self):
        self.start = self.k.pass_counts()
        return self

    def delta(self):
        a, b = self.k.pass_counts()
        return a - self.start[0], b - self.start[1]

    def __exit__(self, *exc):
        self.k.hold_passes(False)          # never leave the shared context holding
        return False


@pytest.mark.parametrize('N,D,K,layout', SHAPES)
def test_three_calls_into_one_x_launch_one_pass(N, D, K, layout):
    import torch
    b = Block(N, D, K, layout)
    ref = [b.eager(A) for A in b.As]
    # the eager passes are what the matrix product says (results with holding off: as ever)
    want = b.As[2].reshape(b.KP, b.DP)[:K, :D] @ b.Y[:, :N]
    assert torch.allclose(ref[2][0][:K, :N], want, rtol=1e-11, atol=1e-11)
    X = b.new_x()
    with counts(b.k) as c:
        b.k.hold_passes(True)
        for A, (_, S_ref) in zip(b.As, ref):
            assert torch.equal(b.xpass(A, X), S_ref)
        torch.cuda.synchronize()
        assert bool((X == SENTINEL).all())
        assert c.delta() == (0, 2)
        b.k.xjoin()
        torch.cuda.synchronize()
        assert torch.equal(X, ref[2][0])
        assert c.delta() == (1, 2)


def test_two_targets_launch_both():
    import torch
    b = Block(2049, 128, 32, 'rows')
    ref = [b.eager(A) for A in b.As[:2]]
    X1, X2 = b.new_x(), b.new_x()
    with counts(b.k) as c:
        b.k.hold_passes(True)
        b.xpass(b.As[0], X1)
        b.xpass(b.As[1], X2)
        b.k.xjoin()
        torch.cuda.synchronize()
        assert torch.equal(X1, ref[0][0]) and torch.equal(X2, ref[1][0])
        assert c.delta() == (2, 0)


@pytest.mark.parametrize('reader', ['stats_from_x', 'pass', 'tile_x', 'ctx_sync', 'hold_off'])
def test_reader_launches_the_held_pass(reader):
    """Each call is followed by the same reads with holding on and off: X, S and the reader's own
    output are bitwise equal, and the held pass was launched (not superseded)."""
    import torch
    b = Block(3000, 128, 32, 'tiled')
    k, L = b.k, b.L

    def read(X):
        out = None
        if reader == 'stats_from_x':
            k.stats_from_x(b.Y, b.ld, b.N, b.D, b.K, X, b.ld, b.state, b.ws)
        elif reader == 'pass':
            k.pass_(b.Y, b.ld, b.N, b.D, b.K, X, b.ld, b.state, b.ws)
        elif reader == 'tile_x':
            out = b.rt.zeros(k.tiled_x_doubles(b.D, b.K, b.N))
            k.tile_x(True, X, b.ld, b.N, b.D, b.K, out)
        elif reader == 'ctx_sync':
            b.rt.check(b.rt.lib.vmp_ctx_sync(b.rt.ctx))
        else:
            k.hold_passes(False)            # launches without joining: the device sync below waits
        torch.cuda.synchronize()
        return X.clone(), b.state[L.off_S:L.off_S + L.len_S].clone(), out

    X0 = b.new_x()
    b.xpass(b.As[0], X0)
    want = read(X0)
    X = b.new_x()
    with counts(k) as c:
        k.hold_passes(True)
        b.xpass(b.As[0], X)
        assert c.delta() == (0, 0)
        got = read(X)
        assert c.delta() == (1, 0)
    assert not bool((got[0][:b.K, :b.N] == SENTINEL).any())
    for g, w in zip(got, want):
        assert (g is None and w is None) or torch.equal(g, w)


def test_hold_off_and_the_switch():
    """Default (off) and "pca_hold_passes" = 0: one launch per call, nothing superseded."""
    import torch
    b = Block(1500, 50, 9, 'rows')
    ref = [b.eager(A) for A in b.As]
    for switch_off in (False, True):
        X = b.new_x()
        with counts(b.k) as c:
            if switch_off:
                b.rt.check(b.rt.lib.vmp_tune_set(b'pca_hold_passes', 0))
                b.k.hold_passes(True)                  # a no-op now
            try:
                for A in b.As:
                    b.xpass(A, X)
                assert c.delta() == (3, 0)
            finally:
                b.rt.check(b.rt.lib.vmp_tune_set(b'pca_hold_passes', 1))
            b.k.xjoin()
            torch.cuda.synchronize()
            assert torch.equal(X, ref[2][0])


# ---- plan level: two identical models, one launching every pass, one deferring -------------------

def _model(N, D, K, layout, defer, seed=5, **vb_kwargs):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    from models import build_pca
    from oracle.pca import make_pca_data
    y, x0 = make_pca_data(N, D, K, seed=seed)
    Q = build_pca(nodes, VB, y, x0, K, **vb_kwargs)
    plan = Q.plans[0]
    plan.plate_layout = layout
    plan.defer_passes = defer
    return Q, plan


def _moments(Q):
    return [u for name in ('W', 'tau', 'alpha', 'X') for u in Q[name].get_moments()]


def _launched(plan, fn):
    a = plan.kernels.pass_counts()[0]
    fn()
    return plan.kernels.pass_counts()[0] - a


@pytest.mark.parametrize('N,D,K,layout', SHAPES)
def test_update_repeat_launches_one_pass(N, D, K, layout):
    res = []
    for defer in (False, True):
        Q, plan = _model(N, D, K, layout, defer)
        n = _launched(plan, lambda: Q.update(repeat=5, verbose=False))
        res.append((n, Q.L[:5].copy(), _moments(Q)))
    assert (res[0][0], res[1][0]) == (5, 1)
    assert np.array_equal(res[0][1], res[1][1])
    for a, b in zip(res[0][2], res[1][2]):
        assert np.array_equal(a, b)


def test_single_sweep_updates_launch_every_pass():
    res = []
    for defer in (False, True):
        Q, plan = _model(3000, 128, 32, 'tiled', defer)
        n = _launched(plan, lambda: [Q.update(repeat=1, verbose=False) for _ in range(5)])
        res.append((n, Q.L[:5].copy(), Q['X'].get_moments()[0]))
    assert (res[0][0], res[1][0]) == (5, 5)
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


def test_early_stop_by_tol_leaves_the_right_x():
    res = []
    for defer in (False, True):
        Q, plan = _model(1500, 50, 9, 'rows', defer)
        Q.ignore_bound_checks = False
        Q.update(repeat=40, tol=0.05, verbose=False)
        res.append((Q.iter, Q['X'].get_moments()[0], Q.L[:Q.iter].copy()))
    assert res[0][0] == res[1][0] and 1 < res[0][0] < 40        # stopped early, not on its first sweep
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


def test_callback_that_reads_x_sees_every_iteration():
    res = []
    for defer in (False, True):
        Q, plan = _model(2049, 128, 32, 'tiled', defer)
        seen = []
        Q.set_callback(lambda: seen.append(Q['X'].get_moments()[0].copy()))
        n = _launched(plan, lambda: Q.update(repeat=4, verbose=False))
        res.append((n, seen))
    assert (res[0][0], res[1][0]) == (4, 4) and len(res[0][1]) == len(res[1][1]) == 4
    for a, b in zip(res[0][1], res[1][1]):
        assert np.array_equal(a, b)
    assert not np.array_equal(res[1][1][0], res[1][1][3])       # (the iterations do differ)


def test_timing_records_the_launched_pass_only():
    Q, plan = _model(3000, 128, 32, 'tiled', True)
    Q.update(repeat=1, verbose=False)
    plan.enable_timing(True)
    try:
        Q.update(repeat=4, verbose=False)
        times = plan.pass_times_ms(64)
    finally:
        plan.enable_timing(False)
    assert len(times) == 1 and times[0][0] > 0
