"""GPU: GaussianMarkovChain with time-varying dynamics / innovation precision.

``vmp_chain_pair_stats`` through raw ctypes against a long-double NumPy sum, per element within
(ny + 2) u sum_b |x_i x_j| (recursive summation; covers any fixed order), bit-identical between
calls and equal to the g++ build of the same header; the models of tests/chain_tv_models.py against
the live-reference fixtures (tests/golden/chain_tv.npz) with the tolerances of test_chain_gpu.py
(bound rtol 1e-9, per-node terms rtol 1e-8 / atol 1e-7, moments rtol 1e-7 / atol 1e-9), with the
tune key chain_pair_stats on and off; eager against recorded sweeps; save / load; which path
answered, read from the family's launch count."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import chain_tv_host
from chain_tv_models import TAGS, build_chain_tv, run_chain_tv_case, SWEEPS

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FAST = ('b2', 'b4', 'b12', 'cA', 'cnu')        # shared dynamics, several sequences, D <= limit


def _rt():
    from bayespy_amd.device import get_runtime
    return get_runtime()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _limits(ny=0, N=1, D=1):
    from bayespy_amd.utils import linalg
    return linalg.chain_pair_stats_limits(ny, N, D)


def _pair_stats(x):
    """(Sxx, Sxp) of one raw call; x: host (ny, N, D)."""
    rt = _rt()
    torch = rt.torch
    ny, N, D = x.shape
    _, _, nw = _limits(ny, N, D)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(rt.device) if ny else \
        torch.zeros(8, dtype=torch.float64, device=rt.device)
    Sxx = torch.full((N, D, D), np.nan, dtype=torch.float64, device=rt.device)
    Sxp = torch.full((max(N - 1, 1), D, D), np.nan, dtype=torch.float64, device=rt.device)
    work = torch.empty(max(nw, 1), dtype=torch.float64, device=rt.device)
    rt.sync_stream()
    rt.check(rt.lib.vmp_chain_pair_stats(rt.ctx, ny, N, D, _vp(xd), _vp(Sxx), _vp(Sxp), _vp(work),
                                         nw))
    return Sxx.cpu().numpy(), Sxp.cpu().numpy()[:N - 1]


def _shapes():
    """ny in {0, 1, 5, 1000, 65537}, N in {2, 3, 64, 1001}, D = 1 .. 16: the full cross up to
    ny = 1000 except that the largest pair (1000, 1001) and ny = 65537 take a few D each (the
    long-double reference of the rest would take minutes on the host)."""
    out = []
    for ny in (0, 1, 5, 1000):
        for N in (2, 3, 64, 1001):
            for D in range(1, 17):
                if ny == 1000 and N == 1001 and D not in (1, 4, 7, 16):
                    continue
                out.append((ny, N, D))
    out += [(65537, 2, D) for D in range(1, 17)]
    out += [(65537, 3, 5), (65537, 3, 9), (65537, 3, 16), (65537, 64, 1), (65537, 64, 4),
            (65537, 64, 7), (65537, 64, 16), (65537, 1001, 1)]
    return out


def _check(x):
    ny, N, D = x.shape
    Sxx, Sxp = _pair_stats(x)
    rxx, rxp, axx, axp = chain_tv_host.reference_pair_stats(x)
    exx = np.abs(Sxx - rxx) - (ny + 2) * U * axx
    exp_ = np.abs(Sxp - rxp) - (ny + 2) * U * axp
    assert np.all(np.isfinite(Sxx)) and np.all(np.isfinite(Sxp))
    assert np.all(exx <= 0), (x.shape, float(exx.max()))
    assert np.all(exp_ <= 0), (x.shape, float(exp_.max()))
    return Sxx, Sxp


def test_limits_query():
    max_d, on, nw = _limits(1000, 64, 4)
    assert max_d >= 16 and on and nw > 0
    lib = chain_tv_host.chain_tv_host()
    assert max_d == lib.chain_tv_max_d() and nw == lib.chain_tv_work_doubles(1000, 64, 4)


def test_pair_stats_against_long_double_sums():
    max_d = _limits()[0]
    assert max_d == 16          # _shapes() runs D = 1 .. the limit
    for ny, N, D in _shapes():
        rs = np.random.RandomState(ny % 1000 + 7 * N + D)
        x = rs.normal(size=(ny, N, D)) * np.exp(rs.normal(size=(ny, 1, 1)))
        Sxx, Sxp = _check(x)
        if ny == 0:
            assert not Sxx.any() and not Sxp.any()


@pytest.mark.parametrize('scale', [1e150, 1e-150])
def test_pair_stats_of_scaled_inputs(scale):
    for ny, N, D in ((5, 3, 2), (1000, 64, 4), (1000, 3, 16), (65537, 2, 3)):
        rs = np.random.RandomState(ny % 1000 + N + D)
        _check(scale * rs.normal(size=(ny, N, D)))


def test_two_calls_give_identical_bits_and_the_host_build_agrees():
    for ny, N, D in ((1000, 64, 4), (65537, 3, 16), (5, 1001, 7), (1000, 2, 1)):
        x = np.random.RandomState(N).normal(size=(ny, N, D))
        a = _pair_stats(x)
        b = _pair_stats(x)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        h = chain_tv_host.host_pair_stats(x)
        assert np.array_equal(a[0], h[0]) and np.array_equal(a[1], h[1])


def test_arguments_are_checked():
    from bayespy_amd import _lib
    rt = _rt()
    t = rt.torch.zeros(4096, dtype=rt.torch.float64, device=rt.device)
    p, null = _vp(t), ctypes.c_void_p(None)
    f = rt.lib.vmp_chain_pair_stats
    rt.sync_stream()
    assert f(None, 1, 2, 2, p, p, p, p, 4096) == _lib.VMP_ERR_INVALID
    assert f(rt.ctx, -1, 2, 2, p, p, p, p, 4096) == _lib.VMP_ERR_INVALID
    assert f(rt.ctx, 1, 0, 2, p, p, p, p, 4096) == _lib.VMP_ERR_INVALID
    assert f(rt.ctx, 1, 2, 0, p, p, p, p, 4096) == _lib.VMP_ERR_INVALID
    assert f(rt.ctx, 1, 2, 2, null, p, p, p, 4096) == _lib.VMP_ERR_INVALID
    assert f(rt.ctx, 1, 2, 2, p, null, p, p, 4096) == _lib.VMP_ERR_INVALID
    assert f(rt.ctx, 1, 2, 2, p, p, null, p, 4096) == _lib.VMP_ERR_INVALID
    assert f(rt.ctx, 1, 2, 2, p, p, p, null, 4096) == _lib.VMP_ERR_INVALID
    assert f(rt.ctx, 1, 2, 2, p, p, p, p, 1) == _lib.VMP_ERR_INVALID          # workspace too small
    assert f(rt.ctx, 1, 2, 17, p, p, p, p, 4096) == _lib.VMP_ERR_UNSUPPORTED
    assert f(rt.ctx, 0, 2, 2, null, p, p, p, 4096) == _lib.VMP_OK            # ny = 0 reads no x
    rt.synchronize()


# -- models ------------------------------------------------------------------------------------------
def _golden(golden_dir):
    f = np.load(os.path.join(golden_dir, 'chain_tv.npz'))
    return f, {k[3:]: f[k] for k in f.files if k.startswith('in_')}


@pytest.fixture
def tune():
    rt = _rt()
    yield lambda v: rt.set_tune('chain_pair_stats', int(v))
    rt.set_tune('chain_pair_stats', 1)


def _calls(Q):
    X = Q['X']
    return X._plan.family[id(X)].pair_stats_calls


def _launches():
    """Calls of the library entry point vmp_chain_pair_stats made so far (utils/linalg.py)."""
    from bayespy_amd.utils import linalg
    return linalg.PAIR_STATS_LAUNCHES[0]


@pytest.mark.parametrize('on', [True, False])
@pytest.mark.parametrize('tag', TAGS)
def test_models_match_reference(golden_dir, tune, monkeypatch, tag, on):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    f, g = _golden(golden_dir)
    tune(on)
    monkeypatch.setenv('BAYESPY_AMD_GRAPH', '0')      # every sweep eager: the family counts each
    before = _launches()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        Q, track = build_chain_tv(N_, VB, g, tag)
        assert type(Q.plans[0]).__name__ == 'GenericPlan'
        Q.update(repeat=SWEEPS, verbose=False)
    # the library entry point ran once per sweep (both messages share its sums), or never
    assert _launches() - before == (SWEEPS if (on and tag in FAST) else 0)
    # A and nu (where they are nodes) were each answered from the kernel's sums in every sweep, or
    # never: case d (A carries the sequence plate), a (one chain) and e (no time plate) never are
    assert _calls(Q) == (2 * SWEEPS if (on and tag in FAST) else 0)
    np.testing.assert_allclose(Q.L[:SWEEPS], f[tag + '_L'], rtol=1e-9)
    for nm, nd in track.items():
        np.testing.assert_allclose(Q.l[nd][:SWEEPS], f['%s_%s_L' % (tag, nm)], rtol=1e-8,
                                   atol=1e-7, err_msg=nm)
        for i, ui in enumerate(nd.u):
            key = '%s_%s_u%d' % (tag, nm, i)
            if key in f.files:
                np.testing.assert_allclose(np.broadcast_to(ui, f[key].shape), f[key], rtol=1e-7,
                                           atol=1e-9, err_msg=key)


def _wide(D, B=5, N=6, M=20, seed=3):
    rs = np.random.RandomState(seed)
    g = {'w_y': rs.normal(size=(M, B, N)), 'w_x0': rs.normal(size=(B, N, D)),
         'w_c0': rs.normal(size=(M, 1, 1, D))}
    return g, (('w', B, D, N, M),)


def test_a_state_above_the_kernel_limit_never_reaches_the_kernel(monkeypatch, tune):
    """D = limit + 1 = 17.  On the device the chain's own smoother (vmp_block_banded_solve, D <= 16)
    refuses such a model before any message is formed, so the family's fallback above the limit
    cannot run here: it is exercised through the host double (test_chain_tv_host.py), and the
    entry point itself answers VMP_ERR_UNSUPPORTED (test_arguments_are_checked).  Here: the error
    is the smoother's, and the kernel was not launched."""
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    import chain_tv_models as m
    D = _limits()[0] + 1
    g, cases = _wide(D)
    monkeypatch.setattr(m, 'CASES', cases)
    monkeypatch.setenv('BAYESPY_AMD_GRAPH', '0')
    tune(True)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        Q, track = build_chain_tv(N_, VB, g, 'w')
        with pytest.raises(NotImplementedError, match='block_banded_solve'):
            Q.update(repeat=1, verbose=False)
    assert _calls(Q) == 0


def test_eager_and_recorded_sweeps_are_bit_identical(golden_dir, monkeypatch):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    _, g = _golden(golden_dir)

    def run():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            Q, track = build_chain_tv(N_, VB, g, 'b4')
            Q.update(repeat=8, verbose=False)
        info = Q['X']._plan.graph_info()
        return [Q.L[:8].copy()] + [np.array(u) for nd in track.values() for u in nd.u], info, \
            _calls(Q)
    monkeypatch.setenv('BAYESPY_AMD_GRAPH', '0')
    eager, _, n_eager = run()
    assert n_eager == 16
    monkeypatch.setenv('BAYESPY_AMD_GRAPH', '1')
    graph, info, n_graph = run()
    assert info['recorded'] and info['disabled'] is None, info
    assert info['replays'] >= 3, info
    assert 0 < n_graph < 16          # the replays launch the recorded kernel without the family
    for a, b in zip(eager, graph):
        assert np.array_equal(a, b)


def test_save_load_round_trip(golden_dir, tmp_path):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    _, g = _golden(golden_dir)

    def build():
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            return build_chain_tv(N_, VB, g, 'b4')
    Q, track = build()
    Q.update(repeat=2, verbose=False)
    fn = str(tmp_path / 'chain_tv.bin')
    Q.save(filename=fn)
    Q.update(repeat=3, verbose=False)
    Q2, track2 = build()
    Q2.load(filename=fn)
    Q2.update(repeat=3, verbose=False)
    assert np.array_equal(Q2.L[:5], Q.L[:5])
    for nm in track:
        for x, y in zip(track2[nm].u, track[nm].u):
            np.testing.assert_array_equal(x, y)
