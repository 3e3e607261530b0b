"""GPU: GaussianMarkovChain with input signals.

``vmp_chain_input_stats`` through raw ctypes against long-double NumPy sums, per element within
(ny + 2) u sum_b |terms| (recursive summation; covers any fixed order), bit-identical between calls
and equal to the g++ build of the same header; the models of tests/chain_in_models.py against the
live-reference fixtures (tests/golden/chain_in.npz) with the tolerances of test_chain_tv_gpu.py
(bound rtol 1e-9, per-node terms rtol 1e-8 / atol 1e-7, moments rtol 1e-7 / atol 1e-9), with the
tune key chain_input_stats on and off; eager against recorded sweeps; save / load; which path
answered, read from the launch counter."""
import ctypes
import os
import warnings

import numpy as np
import pytest

import chain_in_host
from chain_in_models import FULL_MOMENTS, TAGS, build_chain_in, SWEEPS

pytestmark = pytest.mark.gpu

FAST = ('b', 'c', 'd', 'e', 'g')      # shared [A | B] and nu, several sequences, D, K <= limits
DK = ((1, 1), (1, 16), (16, 1), (7, 5), (16, 16))


def _rt():
    from bayespy_amd.device import get_runtime
    return get_runtime()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(None)


def _limits(ny=0, zrows=1, N=2, D=1, K=1):
    from bayespy_amd.utils import linalg
    return linalg.chain_input_stats_limits(ny, zrows, N, D, K)


def _input_stats(x, z, with_zz=True):
    """(Snz, Spz, Szz or None) of one raw call; x: host (ny, N, D), z: host (zrows, N-1, K).  The
    outputs are pre-filled with NaN."""
    rt = _rt()
    torch = rt.torch
    ny, N, D = x.shape
    zrows, _, K = z.shape
    _, _, _, nw = _limits(ny, zrows, N, D, K)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(rt.device) if a.size else \
            torch.zeros(8, dtype=torch.float64, device=rt.device)

    def nan(shape):
        return torch.full(shape, np.nan, dtype=torch.float64, device=rt.device)
    xd, zd = dev(x), dev(z)
    Snz, Spz = nan((N - 1, D, K)), nan((N - 1, D, K))
    Szz = nan((N - 1, K, K)) if with_zz else None
    work = torch.empty(max(nw, 1), dtype=torch.float64, device=rt.device)
    rt.sync_stream()
    rt.check(rt.lib.vmp_chain_input_stats(rt.ctx, ny, zrows, N, D, K, _vp(xd), _vp(zd), _vp(Snz),
                                          _vp(Spz), _vp(Szz), _vp(work), nw))
    return Snz.cpu().numpy(), Spz.cpu().numpy(), (Szz.cpu().numpy() if with_zz else None)


def _shapes(D, K):
    """The full cross of ny in {0, 1, 5, 9, 1000} (9 crosses the stage of 8 rows), N in
    {2, 3, TT + 1, 2 TT + 1} for the time tile TT of (D, K), both zrows, Szz asked for and NULL."""
    TT = chain_in_host.chain_in_host().chain_in_tile(D, K)
    return [(ny, N, D, K, shared, with_zz)
            for ny in (0, 1, 5, 9, 1000) for N in (2, 3, TT + 1, 2 * TT + 1)
            for shared in (False, True) for with_zz in (False, True)]


def test_limits_query_agrees_with_the_host_build():
    lib = chain_in_host.chain_in_host()
    max_d, max_k, on, nw = _limits(1000, 1000, 64, 4, 3)
    assert (max_d, max_k) == (16, 16) == (lib.chain_in_max_d(), lib.chain_in_max_k())
    assert on and nw == lib.chain_in_work_doubles(1000, 64, 4, 3) > 0
    for ny, N, D, K in ((0, 2, 1, 1), (9, 33, 16, 16), (100000, 1001, 7, 5)):
        assert _limits(ny, 1, N, D, K)[3] == lib.chain_in_work_doubles(ny, N, D, K)
    assert _limits(5, 5, 3, 17, 1)[3] == 0 and _limits(5, 5, 3, 1, 17)[3] == 0


@pytest.mark.parametrize('D,K', DK)
def test_input_stats_against_long_double_sums(D, K):
    for ny, N, D, K, shared, with_zz in _shapes(D, K):
        x, z = chain_in_host.make_xz(ny, 1 if shared else ny, N, D, K)
        S = _input_stats(x, z, with_zz)
        assert (S[2] is None) == (not with_zz)
        chain_in_host.check_against_long_double(S, x, z)       # finite, and exact zeros at ny = 0


@pytest.mark.parametrize('scale', [1e150, 1e-150])
def test_input_stats_of_scaled_inputs(scale):
    for ny, N, D, K, shared in ((5, 3, 2, 3, False), (1000, 18, 7, 5, False), (1000, 3, 16, 16, True),
                                (9, 33, 1, 16, True)):
        x, z = chain_in_host.make_xz(ny, 1 if shared else ny, N, D, K, scale)
        chain_in_host.check_against_long_double(_input_stats(x, z), x, z)


def test_two_calls_give_identical_bits_and_the_host_build_agrees():
    for ny, N, D, K, shared in ((1000, 18, 4, 3, False), (1000, 3, 16, 16, False),
                                (9, 103, 7, 5, True), (1000, 2, 1, 1, True), (5, 33, 16, 1, False)):
        x, z = chain_in_host.make_xz(ny, 1 if shared else ny, N, D, K)
        a = _input_stats(x, z)
        b = _input_stats(x, z)
        h = chain_in_host.host_input_stats(x, z)
        for u, v, w in zip(a, b, h):
            assert np.array_equal(u, v) and np.array_equal(u, w)
        c = _input_stats(x, z, with_zz=False)
        assert np.array_equal(c[0], a[0]) and np.array_equal(c[1], a[1])


def test_arguments_are_checked():
    from bayespy_amd import _lib
    rt = _rt()
    t = rt.torch.zeros(4096, dtype=rt.torch.float64, device=rt.device)
    p, null = _vp(t), ctypes.c_void_p(None)
    f = rt.lib.vmp_chain_input_stats
    INV, UNS = _lib.VMP_ERR_INVALID, _lib.VMP_ERR_UNSUPPORTED
    rt.sync_stream()
    #         ctx     ny zrows N  D  K  x  z  Snz Spz Szz work nwork
    assert f(None, 2, 2, 3, 2, 2, p, p, p, p, p, p, 4096) == INV
    assert f(rt.ctx, -1, 1, 3, 2, 2, p, p, p, p, p, p, 4096) == INV
    assert f(rt.ctx, 2, 2, 1, 2, 2, p, p, p, p, p, p, 4096) == INV           # N < 2
    assert f(rt.ctx, 2, 2, 3, 0, 2, p, p, p, p, p, p, 4096) == INV
    assert f(rt.ctx, 2, 2, 3, 2, 0, p, p, p, p, p, p, 4096) == INV
    assert f(rt.ctx, 4, 2, 3, 2, 2, p, p, p, p, p, p, 4096) == INV           # zrows not in {1, ny}
    assert f(rt.ctx, 4, 0, 3, 2, 2, p, p, p, p, p, p, 4096) == INV
    assert f(rt.ctx, 2, 2, 3, 2, 2, null, p, p, p, p, p, 4096) == INV
    assert f(rt.ctx, 2, 2, 3, 2, 2, p, null, p, p, p, p, 4096) == INV
    assert f(rt.ctx, 2, 2, 3, 2, 2, p, p, null, p, p, p, 4096) == INV
    assert f(rt.ctx, 2, 2, 3, 2, 2, p, p, p, null, p, p, 4096) == INV
    assert f(rt.ctx, 2, 2, 3, 2, 2, p, p, p, p, p, null, 4096) == INV
    assert f(rt.ctx, 2, 2, 3, 2, 2, p, p, p, p, p, p, 1) == INV              # workspace too small
    assert f(rt.ctx, 2, 2, 3, 17, 2, p, p, p, p, p, p, 4096) == UNS
    assert f(rt.ctx, 2, 2, 3, 2, 17, p, p, p, p, p, p, 4096) == UNS
    assert f(rt.ctx, 2, 2, 3, 2, 2, p, p, p, p, null, p, 4096) == _lib.VMP_OK     # Szz may be NULL
    assert f(rt.ctx, 0, 0, 3, 2, 2, null, null, p, p, p, p, 4096) == _lib.VMP_OK  # ny = 0 reads nothing
    rt.synchronize()
    q = rt.lib.vmp_chain_input_stats_limits
    i32, i64 = ctypes.c_int32(0), ctypes.c_int64(0)
    r = ctypes.byref
    assert q(2, 2, 3, 2, 2, None, r(i32), r(i32), r(i64)) == INV
    assert q(4, 2, 3, 2, 2, r(i32), r(i32), r(i32), r(i64)) == INV
    assert q(2, 2, 1, 2, 2, r(i32), r(i32), r(i32), r(i64)) == INV
    assert q(2, 2, 3, 17, 2, r(i32), r(i32), r(i32), r(i64)) == UNS
    assert q(2, 2, 3, 2, 17, r(i32), r(i32), r(i32), r(i64)) == UNS
    assert q(2, 1, 3, 2, 2, r(i32), r(i32), r(i32), r(i64)) == _lib.VMP_OK and i64.value > 0


# -- models ------------------------------------------------------------------------------------------
def _golden(golden_dir):
    f = np.load(os.path.join(golden_dir, 'chain_in.npz'))
    return f, {k[3:]: f[k] for k in f.files if k.startswith('in_')}


@pytest.fixture
def tune():
    rt = _rt()
    yield lambda v: rt.set_tune('chain_input_stats', int(v))
    rt.set_tune('chain_input_stats', 1)


def _calls(Q):
    X = Q['X']
    return X._plan.family[id(X)].input_stats_calls


def _launches():
    """Calls of the library entry point vmp_chain_input_stats made so far (utils/linalg.py)."""
    from bayespy_amd.utils import linalg
    return linalg.INPUT_STATS_LAUNCHES[0]


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
        Q, track = build_chain_in(N_, VB, g, tag)
        assert type(Q.plans[0]).__name__ == 'GenericPlan'
        Q.update(repeat=SWEEPS, verbose=False)
    # the library entry point ran once per sweep (both messages share its sums), or never: case a
    # is one chain, in case f [A | B] carries the sequence plate
    assert _launches() - before == (SWEEPS if (on and tag in FAST) else 0)
    assert _calls(Q) == (2 * SWEEPS if (on and tag in FAST) else 0)
    np.testing.assert_allclose(Q.L[:SWEEPS], f[tag + '_L'], rtol=1e-9)
    for nm, nd in track.items():
        np.testing.assert_allclose(Q.l[nd][:SWEEPS], f['%s_%s_L' % (tag, nm)], rtol=1e-8,
                                   atol=1e-7, err_msg=nm)
        for i, ui in enumerate(nd.u):
            key = '%s_%s_u%d' % (tag, nm, i)
            if i > 0 and tag not in FULL_MOMENTS:
                assert key not in f.files          # the large case stores the means only
                continue
            np.testing.assert_allclose(np.broadcast_to(ui, f[key].shape), f[key], rtol=1e-7,
                                       atol=1e-9, err_msg=key)


@pytest.mark.parametrize('D,K', [(17, 2), (2, 17)])
def test_dimensions_above_the_limits_never_reach_the_kernel(monkeypatch, tune, D, K):
    """D = 17: the chain's own smoother (vmp_block_banded_solve, D <= 16) refuses the model before
    any message is formed.  K = 17 with D = 2: the model runs, on the general operations.  Either
    way the kernel is not launched."""
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    import chain_in_models as m
    B, N, M = 5, 5, 20
    rs = np.random.RandomState(3)
    g = {'b_y': rs.normal(size=(M, B, N)), 'b_x0': rs.normal(size=(B, N, D)),
         'b_c0': rs.normal(size=(M, 1, 1, D)), 'b_u': rs.normal(size=(B, N - 1, K))}
    monkeypatch.setattr(m, 'CASES', (('b', B, D, K, N, M),))
    monkeypatch.setenv('BAYESPY_AMD_GRAPH', '0')
    tune(True)
    before = _launches()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        Q, track = m.build_chain_in(N_, VB, g, 'b')
        if D > 16:
            with pytest.raises(NotImplementedError, match='block_banded_solve'):
                Q.update(repeat=1, verbose=False)
        else:
            Q.update(repeat=2, verbose=False)
            assert np.all(np.isfinite(Q.L[:2]))
    assert _calls(Q) == 0 and _launches() == before


def test_eager_and_recorded_sweeps_are_bit_identical(golden_dir, monkeypatch):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    _, g = _golden(golden_dir)

    def run(tag):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            Q, track = build_chain_in(N_, VB, g, tag)
            Q.update(repeat=8, verbose=False)
        info = Q['X']._plan.graph_info()
        return [Q.L[:8].copy()] + [np.array(u) for nd in track.values() for u in nd.u], info, \
            _calls(Q)
    for tag in ('b', 'e'):
        monkeypatch.setenv('BAYESPY_AMD_GRAPH', '0')
        eager, _, n_eager = run(tag)
        assert n_eager == 16
        monkeypatch.setenv('BAYESPY_AMD_GRAPH', '1')
        graph, info, n_graph = run(tag)
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
            return build_chain_in(N_, VB, g, 'e')
    Q, track = build()
    Q.update(repeat=2, verbose=False)
    fn = str(tmp_path / 'chain_in.bin')
    Q.save(filename=fn)
    Q.update(repeat=3, verbose=False)
    Q2, track2 = build()
    Q2.load(filename=fn)
    Q2.update(repeat=3, verbose=False)
    assert np.array_equal(Q2.L[:5], Q.L[:5])
    for nm in track:
        for x, y in zip(track2[nm].u, track[nm].u):
            np.testing.assert_array_equal(x, y)
