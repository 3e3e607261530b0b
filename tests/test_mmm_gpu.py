"""GPU: the fused multinomial-mixture block (inference/plans/mmm.py, csrc/vmp_mmm.hip) -- every
fixture of tests/golden/mmm.npz through ``VB(..., engine='fused')``, each entry point alone through
the C ABI against the long-double restatement of tests/mmm_host.py at sizes that cross tile,
lane-group, word-block and chunk boundaries, fixed labels, bit-identity, the rows of r_out, the
flags of the pack and the argument checks."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

L_RTOL = 1e-9
MID = (300, 70, 5)                          # (N, M, K)
# the word blocks are 128 wide, a chunk has 256 rows: N = 256 and 513 are the last row of a first
# chunk and the first row of a third
SHAPES = sorted(set([(MID[0], MID[1], K) for K in (1, 2, 15, 16, 17, 64)]
                    + [(MID[0], M, MID[2]) for M in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)]
                    + [(N, MID[1], MID[2]) for N in (0, 1, 63, 65, 257, 763, 256, 513)]
                    + [MID, (763, 257, 64)]))
BITS = ('S', 'Nk', 'sum_lse', 'Nk_c', 'S_L')


def _kernels():
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.mmm import MMMKernels
    rt = get_runtime()
    rt.sync_stream()
    return rt, MMMKernels(rt)


def _up(rt, a):
    return rt.torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)


def _device_pack(N, M, x, trials):
    """dict of xp (N, M) uint16, flags, lcoef and the device buffer."""
    from mmm_host import DTYPES
    rt, k = _kernels()
    torch = rt.torch
    xp = torch.zeros(max(N * M, 4), dtype=torch.int16, device=rt.device)
    flags = torch.zeros(4, dtype=torch.int32, device=rt.device)
    lcoef, ws = rt.zeros(1), rt.empty(1024)
    n = np.ascontiguousarray(np.broadcast_to(trials, (N,)), dtype=np.int64)
    k.pack(N, M, DTYPES[x.dtype.name], _up(rt, x) if N else rt.zeros(1),
           _up(rt, n) if N else rt.zeros(1), xp, flags, lcoef, ws)
    rt.synchronize()
    return dict(xp=xp.cpu().numpy()[:N * M].view(np.uint16).reshape(N, M),
                flags=flags.cpu().numpy(), lcoef=float(lcoef.cpu().numpy()[0]), dev=xp)


def _device_pass(N, M, K, xp_dev, L, c, labels=None, want_r=False):
    """dict of S (K, M), Nk, sum_lse, Nk_c, S_L and r (or None) of vmp_mmm_pass."""
    rt, k = _kernels()
    chunk, wsd = k.plan(N, M, K)
    assert chunk == 256
    S, Nk, scal = rt.empty(K, M), rt.empty(K), rt.zeros(8)
    ws = rt.empty(int(wsd))
    r = rt.empty(N, K) if want_r and N else None
    lab = None if labels is None else _up(rt, labels.astype(np.int32))
    k.pass_(N, M, K, xp_dev, lab, _up(rt, L), _up(rt, c), ws, S, Nk, scal, r)
    rt.synchronize()
    s = scal.cpu().numpy()
    return dict(S=S.cpu().numpy(), Nk=Nk.cpu().numpy(), sum_lse=s[0], Nk_c=s[1], S_L=s[2],
                r=np.zeros((0, K)) if want_r and not N else (None if r is None else r.cpu().numpy()))


def _device_tables(M, K, elog_p, elog_pi):
    rt, k = _kernels()
    L, c = rt.empty(M, K), rt.empty(K)
    k.tables(M, K, None if elog_p is None else _up(rt, elog_p), _up(rt, elog_pi), L, c)
    rt.synchronize()
    return L.cpu().numpy(), c.cpu().numpy()


@pytest.mark.parametrize('N,M,K', SHAPES)
def test_every_entry_point_against_long_double_restatement(N, M, K):
    """Per quantity 8 times the deviation of the plain float64 evaluation from long double, floor
    4 ulp of the magnitude; soft rows and fixed labels."""
    from mmm_host import (host_pack, host_pass, host_tables, restate_pack, restate_pass,
                          restate_tables, tolerances, error, pass_inputs, PASS_QUANTITIES)
    inp = pass_inputs(N, M, K)
    x, trials = inp['x'], inp['trials']
    pk = _device_pack(N, M, x, trials)
    hp = host_pack(x, trials)
    np.testing.assert_array_equal(pk['xp'], hp['xp'])
    assert not pk['flags'].any()
    ld, f64 = restate_pack(x, trials), restate_pack(x, trials, np.float64)
    tol, dev = tolerances(ld, f64, ('lcoef',))
    err = error(pk['lcoef'], ld['lcoef'])
    print('lcoef %s: float64 deviation %.3g, kernel %.3g, allowed %.3g'
          % ((N, M, K), dev['lcoef'], err, tol['lcoef']))
    assert err <= tol['lcoef']
    # the tables
    L, c = _device_tables(M, K, inp['elog_p'], inp['elog_pi'])
    ldt = restate_tables(inp['elog_p'], inp['elog_pi'], M, K)
    f64t = restate_tables(inp['elog_p'], inp['elog_pi'], M, K, np.float64)
    tol, dev = tolerances(dict(zip('Lc', ldt)), dict(zip('Lc', f64t)), 'Lc')
    for nm, g_, r_ in zip('Lc', (L, c), ldt):
        assert error(g_, r_) <= tol[nm], nm
    hl, hc = host_tables(M, K, inp['elog_p'], inp['elog_pi'])
    np.testing.assert_array_equal(L, hl)
    np.testing.assert_array_equal(c, hc)
    L0, c0 = _device_tables(M, K, None, inp['elog_pi'])
    assert not L0.any() and np.array_equal(c0, c)
    # the pass
    got = _device_pass(N, M, K, pk['dev'], L, c, want_r=True)
    ld = restate_pass(x, L, c)
    f64 = restate_pass(x, L, c, np.float64)
    tol, dev = tolerances(ld, f64, PASS_QUANTITIES)
    host = host_pass(N, M, K, hp['xp'], None, L, c, want_r=True)
    for key in PASS_QUANTITIES:
        err, herr = error(got[key], ld[key]), error(host[key], ld[key])
        print('%s %s: float64 deviation %.3g, kernel %.3g, host build %.3g, allowed %.3g'
              % (key, (N, M, K), dev[key], err, herr, tol[key]))
        assert err <= tol[key], (key, err, tol[key])
    if N and K > 1:                             # soft rows: a condition on the inputs
        assert np.mean(np.asarray(ld['r'], dtype=np.float64).max(axis=1) < 0.99) >= 0.5
    if N:
        # each r_k is one rounded quotient of the sum s (half an ulp of r_k, half an ulp of one in
        # all) and adding K of them in float64 rounds K - 1 times more
        np.testing.assert_allclose(got['r'].sum(axis=1), 1.0, rtol=0, atol=(K + 1) * 2.0 ** -53)
    # fixed labels: exact integer counts, lse = 0
    got = _device_pass(N, M, K, pk['dev'], L, c, labels=inp['labels'], want_r=True)
    one = np.eye(K)[inp['labels']]
    np.testing.assert_array_equal(got['r'], one)
    np.testing.assert_array_equal(got['Nk'], one.sum(0))
    np.testing.assert_array_equal(got['S'], one.T @ x.astype(float))
    assert got['sum_lse'] == 0


@pytest.mark.parametrize('N,M,K', [MID, (763, 257, 64), (257, 129, 16), (65, 65, 17)])
def test_bit_identity(N, M, K):
    """Two launches on the same inputs, with and without r_out, every dtype of x: the same bits."""
    from mmm_host import pass_inputs, host_tables
    inp = pass_inputs(N, M, K)
    L, c = host_tables(M, K, inp['elog_p'], inp['elog_pi'])

    def run(xx, want_r=True):
        pk = _device_pack(N, M, xx, inp['trials'])
        out = _device_pass(N, M, K, pk['dev'], L, c, want_r=want_r)
        out['xp'], out['lcoef'] = pk['xp'], pk['lcoef']
        return out
    x = inp['x']
    a, b, n = run(x), run(x), run(x, want_r=False)
    others = [b, run(x.astype(np.float64)), run(x.astype(np.int32)), run(x.astype(np.uint8))]
    for key in BITS + ('r', 'xp', 'lcoef'):
        for other in others:
            np.testing.assert_array_equal(a[key], other[key], err_msg=key)
    for key in BITS:
        np.testing.assert_array_equal(a[key], n[key], err_msg=key)


@pytest.mark.parametrize('fixed', [False, True], ids=['soft', 'labels'])
@pytest.mark.parametrize('N,M,K', [(65, 65, 17), (257, 129, 16), (763, 257, 64), (0, 70, 5)])
def test_the_pass_is_the_poisson_pass(N, M, K, fixed):
    """vmp_mmm_pass runs the Poisson block's pass kernel: on the same packed x, L and c,
    vmp_pmm_pass(hidden = 0, l = L, lb = zeros) gives the same bits of N_k, sum lse, r_out and S
    (its D x K transposed).  scal[1] and scal[2] are added in another order there and are left out.
    The shapes: a ragged second tile with K padded into a second lane group; a second chunk and a
    second word block (the carry through the partial, and fixed labels skipping the logit walk);
    KT = 4 with three blocks and three chunks; no rows (the combine alone)."""
    from bayespy_amd.inference.plans.pmm import PMMKernels
    from mmm_host import pass_inputs, host_tables
    inp = pass_inputs(N, M, K)
    L, c = host_tables(M, K, inp['elog_p'], inp['elog_pi'])
    labels = inp['labels'] if fixed else None
    pk = _device_pack(N, M, inp['x'], inp['trials'])
    got = _device_pass(N, M, K, pk['dev'], L, c, labels=labels, want_r=True)
    rt, _ = _kernels()
    k = PMMKernels(rt)
    S, Nk, scal = rt.empty(M, K), rt.empty(K), rt.zeros(8)
    ws = rt.empty(int(k.plan(N, M, K)[1]))
    r = rt.empty(N, K) if N else None
    lab = None if labels is None else _up(rt, labels.astype(np.int32))
    k.pass_(N, M, K, 0, pk['dev'], lab, _up(rt, L), rt.zeros(M, K), _up(rt, c), ws, S, None, Nk,
            scal, r)
    rt.synchronize()
    np.testing.assert_array_equal(got['Nk'], Nk.cpu().numpy())
    np.testing.assert_array_equal(got['sum_lse'], scal.cpu().numpy()[0])
    np.testing.assert_array_equal(got['S'], S.cpu().numpy().T)
    if N:
        np.testing.assert_array_equal(got['r'], r.cpu().numpy())


def test_pack_flags_and_the_cap():
    from mmm_host import pass_inputs
    N, M, K = MID
    inp = pass_inputs(N, M, K)
    x, trials = inp['x'], inp['trials']
    for v, flags in ((-1.0, (1, 0, 0, 0)), (0.5, (1, 0, 1, 0)), (np.nan, (1, 0, 1, 0)),
                     (1e300, (0, 1, 0, 0)), (65535.0, (0, 1, 0, 0))):
        bad = x.astype(np.float64)
        bad[5, 6] = v
        got = _device_pack(N, M, bad, trials)
        assert tuple(got['flags']) == flags and got['xp'][5, 6] == 0, v
    for v, flags in ((-1, (1, 0, 0, 0)), (65535, (0, 1, 0, 0)), (2 ** 40, (0, 1, 0, 0))):
        bad = x.copy()
        bad[5, 6] = v
        assert tuple(_device_pack(N, M, bad, trials)['flags']) == flags, v
    # a row that misses its number of trials, the last row included
    for row, d in ((5, 1), (5, -1), (N - 1, 1)):
        off = trials.copy()
        off[row] += d
        assert tuple(_device_pack(N, M, x, off)['flags']) == (0, 0, 0, 1)
    for a in (x.copy(), x.astype(np.float64)):
        a[5, 6] = 65534                             # exactly the cap: accepted
        got = _device_pack(N, M, a, a.sum(axis=1).astype(np.int64))
        assert not got['flags'].any() and got['xp'][5, 6] == 65534


# -- end to end ------------------------------------------------------------------------------------------
def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    return dict(nodes=nodes, VB=VB, vb_kwargs=kw)


def test_fixtures_on_the_fused_block():
    """Fails without the feature: NotImplementedError from VB(..., engine='fused').  The bound and
    its terms at rtol 1e-9, the moments at rtol 1e-7."""
    from mmm_models import run_mmm_cases, CASES
    from test_mmm_host import check_fixture, _golden, PER_CASE
    from bayespy_amd.inference.plans.mmm import MultinomialMixturePlan
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_mmm_cases(_mods(engine='fused'), gin)
    for tag in CASES:
        assert isinstance(res[tag + '_plan'].plans[0], MultinomialMixturePlan)
    assert check_fixture(res, g, CASES) == len(CASES) * PER_CASE
    np.testing.assert_allclose(res['a_Z_u0'].sum(axis=1), 1.0, rtol=0, atol=4 * 2.0 ** -53)


def test_per_row_trials_a_device_tensor_invalid_counts_and_the_example():
    import torch
    from mmm_models import build_mmm
    from mmm_host import pass_inputs, restate_pack
    from bayespy_amd.inference import VB
    inp = pass_inputs(300, 17, 3)
    x, trials = inp['x'], inp['trials']
    m = build_mmm(_mods(), x, trials[:, None], 3)
    m['X']._data = torch.from_numpy(x).to('cuda')
    np.random.seed(3)
    m['P'].initialize_from_random()
    Q = VB(m['Z'], m['R'], m['X'], m['P'], engine='fused')
    Q.update(repeat=4, verbose=False)
    plan = Q.plans[0]
    assert type(plan).__name__ == 'MultinomialMixturePlan'
    assert np.all(np.isfinite(Q.L[:4])) and np.all(np.diff(Q.L[:4]) > -1e-8)
    np.testing.assert_allclose(float(plan.lcoef.cpu().numpy()[0]),
                               float(restate_pack(x, trials)['lcoef']), rtol=1e-13)
    for v, exc, text in ((-1, ValueError, 'Counts must be non-negative'),
                         (70000, NotImplementedError, 'fused multinomial-mixture block.*65534'),
                         (int(x[5, 0]) + 1, ValueError, 'Counts must sum to the number of trials')):
        bad = torch.from_numpy(x).to('cuda')
        bad[5, 0] = v
        m['X']._data = bad
        plan.invalidate(m['X'])
        with pytest.raises(exc, match=text):
            Q.update(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import multinomial_mixture
    out = multinomial_mixture.run(N=500, M=12, K=3, sweeps=8, verbose=False)
    assert out['plan'] == 'MultinomialMixturePlan' and np.all(np.diff(out['L']) > -1e-6)
    assert out['accuracy'] > 0.6


def test_the_pass_entry_point_is_exported():
    """Fails without the feature: the library has no such symbol."""
    from bayespy_amd import _lib
    assert hasattr(_lib.load(), 'vmp_mmm_pass')


# -- argument checks: nothing is launched ------------------------------------------------------------------
def test_argument_checks():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(4096)
    z.fill_(7.0)
    p = ctypes.c_void_p(z.data_ptr())
    ok = [p] * 9                # x, labels, L, c, ws, S, Nk, scal, r_out
    for i in (0, 2, 3, 4, 5, 6, 7):
        args = list(ok)
        args[i] = None
        assert lib.vmp_mmm_pass(ctx, 4, 4, 4, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_mmm_pass(None, 4, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_mmm_pass(ctx, -1, 4, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_mmm_pass(ctx, 4, 0, 4, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_mmm_pass(ctx, 4, 4, 0, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_mmm_pass(ctx, 4, 4, 65, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_mmm_pass(ctx, 4, 1025, 4, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_mmm_pass(ctx, 4, 1025, 4, *[None] * 9) == _lib.VMP_ERR_UNSUPPORTED
    four = [p] * 4              # elog_p, elog_pi, L, c
    for i in (1, 2, 3):
        args = list(four)
        args[i] = None
        assert lib.vmp_mmm_tables(ctx, 4, 4, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_mmm_tables(ctx, 0, 4, *four) == _lib.VMP_ERR_INVALID
    assert lib.vmp_mmm_tables(ctx, 4, 65, *four) == _lib.VMP_ERR_UNSUPPORTED
    six = [p] * 6               # x, trials, x_packed, flags, lcoef, ws
    for i in range(6):
        args = list(six)
        args[i] = None
        assert lib.vmp_mmm_pack(ctx, 4, 4, 0, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_mmm_pack(ctx, 4, 4, 4, *six) == _lib.VMP_ERR_INVALID
    assert lib.vmp_mmm_pack(ctx, -1, 4, 0, *six) == _lib.VMP_ERR_INVALID
    assert lib.vmp_mmm_pack(ctx, 4, 1025, 0, *six) == _lib.VMP_ERR_UNSUPPORTED
    rt.synchronize()
    assert np.all(z.cpu().numpy() == 7.0)                   # nothing was launched
