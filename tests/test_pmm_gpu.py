"""GPU: the fused Poisson-mixture block (inference/plans/pmm.py, csrc/vmp_pmm.hip) -- every fixture
of tests/golden/pmm.npz through ``VB(..., engine='fused')``, each entry point alone through the C
ABI against the long-double restatement of tests/pmm_host.py at sizes that cross tile, lane-group,
column-block and chunk boundaries, fixed labels, masks, bit-identity, the flags of the pack and the
argument checks."""
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
MID = (300, 70, 5)                          # (N, D, K)
# the column blocks are 128 (nothing hidden) and 64 (hidden entries) wide
SHAPES = sorted(set([(MID[0], MID[1], K) for K in (1, 2, 15, 16, 17, 64)]
                    + [(MID[0], D, MID[2]) for D in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)]
                    + [(N, MID[1], MID[2]) for N in (0, 1, 63, 65, 257, 763)]
                    + [MID, (763, 257, 64)]))
BITS = ('S', 'M', 'Nk', 'sum_lse', 'Nk_c', 'S_lM')


def _kernels():
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.pmm import PMMKernels
    rt = get_runtime()
    rt.sync_stream()
    return rt, PMMKernels(rt)


def _up(rt, a):
    return rt.torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)


def _device_pack(N, D, x, mask):
    """dict of xp (N, D) uint16, flags, n_observed, n_hidden, lgam and the device buffer."""
    from pmm_host import DTYPES
    rt, k = _kernels()
    torch = rt.torch
    xp = torch.zeros(max(N * D, 4), dtype=torch.int16, device=rt.device)
    flags = torch.zeros(3, dtype=torch.int32, device=rt.device)
    counts = torch.zeros(2, dtype=torch.int64, device=rt.device)
    lgam, ws = rt.zeros(1), rt.empty(2048)
    md = None if mask is None else _up(rt, np.asarray(mask).astype(np.uint8))
    k.pack(N, D, DTYPES[x.dtype.name], _up(rt, x) if N else rt.zeros(1), md, xp, flags, counts,
           lgam, ws)
    rt.synchronize()
    n = counts.cpu().numpy()
    return dict(xp=xp.cpu().numpy()[:N * D].view(np.uint16).reshape(N, D),
                flags=flags.cpu().numpy(), n_observed=int(n[0]), n_hidden=int(n[1]),
                lgam=float(lgam.cpu().numpy()[0]), dev=xp)


def _device_pass(N, D, K, hidden, xp_dev, l, lb, c, labels=None, want_r=False):
    """dict of S, M (D, K), Nk, sum_lse, Nk_c, S_lM and r (or None) of vmp_pmm_pass."""
    rt, k = _kernels()
    chunk, wsd = k.plan(N, D, K)
    assert chunk == 256
    S, M, Nk, scal = rt.empty(D, K), rt.zeros(D, K), rt.empty(K), rt.zeros(8)
    ws = rt.empty(int(wsd))
    r = rt.empty(N, K) if want_r and N else None
    lab = None if labels is None else _up(rt, labels.astype(np.int32))
    k.pass_(N, D, K, hidden, xp_dev, lab, _up(rt, l), _up(rt, lb), _up(rt, c), ws, S, M, Nk, scal, r)
    rt.synchronize()
    s = scal.cpu().numpy()
    Nk = Nk.cpu().numpy()
    return dict(S=S.cpu().numpy(), M=M.cpu().numpy() if hidden else np.broadcast_to(Nk, (D, K)),
                Nk=Nk, sum_lse=s[0], Nk_c=s[1], S_lM=s[2],
                r=np.zeros((0, K)) if want_r and not N else (None if r is None else r.cpu().numpy()))


def _device_tables(D, K, form, lam_mom, elog_pi):
    rt, k = _kernels()
    l, lb, c, lsum = rt.empty(D, K), rt.empty(D, K), rt.empty(K), rt.empty(K)
    k.tables(D, K, form, None if lam_mom is None else _up(rt, lam_mom), _up(rt, elog_pi), l, lb, c,
             lsum)
    rt.synchronize()
    return tuple(t.cpu().numpy() for t in (l, lb, c, lsum))


def _device_update(D, K, per_element, a0, b0, S, cnt):
    rt, k = _kernels()
    par, mom, bound = rt.empty(D * K, 2), rt.empty(D * K, 2), rt.zeros(1)
    k.update(D, K, per_element, _up(rt, a0), _up(rt, b0), None if S is None else _up(rt, S),
             None if cnt is None else _up(rt, cnt), par, mom, bound)
    rt.synchronize()
    return par.cpu().numpy(), mom.cpu().numpy(), float(bound.cpu().numpy()[0])


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_every_entry_point_against_long_double_restatement(N, D, K):
    """Per quantity 8 times the deviation of the plain float64 evaluation from long double, floor
    4 ulp of the magnitude; without a mask, with the mask of fixture (f) and with
    fixed labels."""
    from pmm_host import (host_pack, host_pass, host_tables, restate_pack, restate_pass,
                          restate_tables, restate_update, tolerances, error, mixed_mask,
                          pass_inputs, PASS_QUANTITIES, UPDATE_QUANTITIES)
    inp = pass_inputs(N, D, K)
    x, rs = inp['x'], inp['rs']
    for hidden in (0, 1):
        mask = mixed_mask(N, D, rs, 64) if hidden else None
        pk = _device_pack(N, D, x, mask)
        hp = host_pack(x, mask)
        np.testing.assert_array_equal(pk['xp'], hp['xp'])
        assert not pk['flags'].any()
        assert (pk['n_observed'], pk['n_hidden']) == (hp['n_observed'], hp['n_hidden'])
        ld, f64 = restate_pack(x, mask), restate_pack(x, mask, np.float64)
        tol, dev = tolerances(ld, f64, ('lgam',))
        err = error(pk['lgam'], ld['lgam'])
        print('lgam %s hidden=%d: float64 deviation %.3g, kernel %.3g, allowed %.3g'
              % ((N, D, K), hidden, dev['lgam'], err, tol['lgam']))
        assert err <= tol['lgam']
        # the tables: as they are and centred
        for form in (hidden, hidden | 2):
            got = _device_tables(D, K, form, inp['lam_mom'], inp['elog_pi'])
            ldt = restate_tables(inp['lam_mom'], inp['elog_pi'], D, K, form)
            f64t = restate_tables(inp['lam_mom'], inp['elog_pi'], D, K, form, np.float64)
            names = ('l', 'lb', 'c', 'lsum')
            tol, dev = tolerances(dict(zip(names, ldt)), dict(zip(names, f64t)), names)
            for nm, g_, r_ in zip(names, got, ldt):
                assert error(g_, r_) <= tol[nm], (nm, form)
        l, lb, c, lsum = got
        hl, hlb, hc, _ = host_tables(D, K, hidden | 2, inp['lam_mom'], inp['elog_pi'])
        np.testing.assert_array_equal(l, hl)
        np.testing.assert_array_equal(c, hc)
        # the pass
        got = _device_pass(N, D, K, hidden, pk['dev'], l, lb, c, want_r=True)
        ld = restate_pass(x, mask, l, lb, c, hidden)
        f64 = restate_pass(x, mask, l, lb, c, hidden, np.float64)
        tol, dev = tolerances(ld, f64, PASS_QUANTITIES)
        host = host_pass(N, D, K, hidden, hp['xp'], None, l, lb, c, want_r=True)
        for key in PASS_QUANTITIES:
            err, herr = error(got[key], ld[key]), error(host[key], ld[key])
            print('%s %s hidden=%d: float64 deviation %.3g, kernel %.3g, host build %.3g, allowed '
                  '%.3g' % (key, (N, D, K), hidden, dev[key], err, herr, tol[key]))
            assert err <= tol[key], (key, hidden, err, tol[key])
        if N and K > 1:                         # soft rows: a condition on the inputs
            assert np.mean(np.asarray(ld['r'], dtype=np.float64).max(axis=1) < 0.99) >= 0.5
        if hidden and N > 2:
            # the row of nothing: r = softmax(c); a column of nothing: exact zeros
            np.testing.assert_allclose(got['r'][2], np.exp(c) / np.exp(c).sum(), rtol=1e-13)
        if hidden and D > 2 and N:
            assert np.all(got['S'][1] == 0) and np.all(got['M'][1] == 0)
        # the update from these statistics
        cnt = got['M'] if hidden else got['Nk']
        par, mom, bound = _device_update(D, K, hidden, inp['a0'], inp['b0'], got['S'],
                                         np.ascontiguousarray(cnt))
        ldu = restate_update(inp['a0'], inp['b0'], got['S'], cnt)
        f64u = restate_update(inp['a0'], inp['b0'], got['S'], cnt, np.float64)
        tol, dev = tolerances(ldu, f64u, UPDATE_QUANTITIES)
        for key, val in (('par', par), ('mom', mom), ('bound', bound)):
            err = error(val, ldu[key])
            print('%s %s hidden=%d: float64 deviation %.3g, kernel %.3g, allowed %.3g'
                  % (key, (N, D, K), hidden, dev[key], err, tol[key]))
            assert err <= tol[key], (key, hidden, err, tol[key])
        # fixed labels: exact integer counts, lse = 0
        got = _device_pass(N, D, K, hidden, pk['dev'], l, lb, c, labels=inp['labels'],
                           want_r=True)
        m = np.ones((N, D), dtype=bool) if mask is None else mask
        one = np.eye(K)[inp['labels']]
        np.testing.assert_array_equal(got['r'], one)
        one = one * m.any(axis=1)[:, None]
        np.testing.assert_array_equal(got['Nk'], one.sum(0))
        np.testing.assert_array_equal(got['S'], np.where(m, x, 0).astype(float).T @ one)
        if hidden:
            np.testing.assert_array_equal(got['M'], m.astype(float).T @ one)
        assert got['sum_lse'] == 0
    # the prior: a bound term of exactly zero
    par, mom, bound = _device_update(D, K, 1, inp['a0'], inp['b0'], None, None)
    assert bound == 0.0
    np.testing.assert_array_equal(par.reshape(D, K, 2)[..., 0], inp['a0'])


@pytest.mark.parametrize('N,D,K', [MID, (763, 257, 64), (257, 129, 16), (65, 65, 17)])
def test_bit_identity(N, D, K):
    """Two calls, with and without r_out, different junk at hidden positions, a mask of ones
    against no mask: the same bits."""
    from pmm_host import mixed_mask, pass_inputs, host_tables, junk_at_hidden
    inp = pass_inputs(N, D, K)
    x = inp['x']
    m = mixed_mask(N, D, inp['rs'], 64)
    l, lb, c, _ = host_tables(D, K, 3, inp['lam_mom'], inp['elog_pi'])

    def run(xx, mask, want_r=True):
        pk = _device_pack(N, D, xx, mask)
        hidden = 1 if pk['n_hidden'] else 0
        out = _device_pass(N, D, K, hidden, pk['dev'], l, lb, c, want_r=want_r)
        out['xp'], out['lgam'], out['hidden'] = pk['xp'], pk['lgam'], hidden
        return out
    a, b, n = run(x, m), run(x, m), run(x, m, want_r=False)
    j1 = run(junk_at_hidden(x, m, np.nan), m)
    junk = junk_at_hidden(x, m, 0.0)
    junk[~m] = np.resize([-1.0, 1e300, np.nan, 0.5, 70000.0], int((~m).sum()))
    j2 = run(junk, m)
    assert a['hidden'] == 1
    for key in BITS + ('r', 'xp', 'lgam'):
        for other in (b, j1, j2):
            np.testing.assert_array_equal(a[key], other[key], err_msg=key)
    for key in BITS:
        np.testing.assert_array_equal(a[key], n[key], err_msg=key)
    l, lb, c, _ = host_tables(D, K, 2, inp['lam_mom'], inp['elog_pi'])
    u, o = run(x, None), run(x, np.ones((N, D), dtype=bool))
    assert u['hidden'] == 0 and o['hidden'] == 0            # the same instance
    for key in BITS + ('r', 'xp', 'lgam'):
        np.testing.assert_array_equal(u[key], o[key], err_msg=key)


def test_pack_dtypes_both_flags_and_the_cap():
    from pmm_host import host_pack, pass_inputs, HIDDEN
    N, D, K = MID
    inp = pass_inputs(N, D, K)
    x, rs = inp['x'], inp['rs']
    mask = rs.rand(N, D) < 0.7
    want = host_pack(x, mask)
    for a in (x.astype(np.float64), x.astype(np.int64), x.astype(np.int32), x.astype(np.uint8)):
        got = _device_pack(N, D, a, mask)
        np.testing.assert_array_equal(got['xp'], want['xp'])
        assert got['lgam'] == want['lgam'] and got['n_hidden'] == want['n_hidden']
    mask[5, 6] = True
    for v, flags in ((-1.0, (1, 0, 0)), (0.5, (1, 0, 1)), (np.nan, (1, 0, 1)), (1e300, (0, 1, 0)),
                     (65535.0, (0, 1, 0))):
        bad = x.astype(np.float64)
        bad[5, 6] = v
        got = _device_pack(N, D, bad, mask)
        assert tuple(got['flags']) == flags and got['xp'][5, 6] == HIDDEN, v
    for v, flags in ((-1, (1, 0, 0)), (65535, (0, 1, 0)), (2 ** 40, (0, 1, 0))):
        bad = x.copy()
        bad[5, 6] = v
        got = _device_pack(N, D, bad, mask)
        assert tuple(got['flags']) == flags and got['xp'][5, 6] == HIDDEN, v
    for a in (x.copy(), x.astype(np.float64)):
        a[5, 6] = 65534                             # exactly the cap: accepted
        got = _device_pack(N, D, a, mask)
        assert not got['flags'].any() and got['xp'][5, 6] == 65534


# -- end to end ------------------------------------------------------------------------------------------
def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    return dict(nodes=nodes, VB=VB, vb_kwargs=kw)


def test_fixtures_on_the_fused_block():
    """Fails without the feature: NotImplementedError from VB(..., engine='fused')."""
    from pmm_models import run_pmm_cases, CASES
    from test_pmm_host import check_fixture, _golden, PER_CASE
    from bayespy_amd.inference.plans.pmm import PoissonMixturePlan
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_pmm_cases(_mods(engine='fused'), gin)
    for tag in CASES:
        assert isinstance(res[tag + '_plan'].plans[0], PoissonMixturePlan)
    assert check_fixture(res, g, CASES) == len(CASES) * PER_CASE
    for k in ('L', 'Z_u0', 'lam_u0', 'lam_u1', 'R_u0'):
        np.testing.assert_array_equal(res['g_' + k], res['a_' + k], err_msg=k)
    assert res['f_plan'].plans[0].hidden == 1 and res['g_plan'].plans[0].hidden == 0


def test_the_fused_block_and_the_generic_engine_agree_on_case_a():
    from pmm_models import run_pmm_cases
    from test_pmm_host import _golden
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fused = run_pmm_cases(_mods(engine='fused'), gin, only=('a',))
        generic = run_pmm_cases(_mods(engine='generic'), gin, only=('a',))
    assert type(generic['a_plan'].plans[0]).__name__ == 'GenericPlan'
    np.testing.assert_allclose(fused['a_L'], generic['a_L'], rtol=L_RTOL)


def test_the_pass_entry_point_is_exported():
    """Fails without the feature: the library has no such symbol."""
    from bayespy_amd import _lib
    assert hasattr(_lib.load(), 'vmp_pmm_pass')


def test_invalid_counts_on_a_device_tensor_device_mask_and_the_example():
    import torch
    from pmm_models import build_pmm
    from test_pmm_host import _golden
    from bayespy_amd.inference import VB
    g, gin = _golden()
    x, mask = gin['a_x'], gin['f_mask']
    m = build_pmm(_mods(), x, 3, a0=gin['a_a0'], b0=gin['a_b0'], alpha=gin['a_alpha'],
                  observe=False)
    m['X'].observe(np.where(mask, x, 0), mask=torch.from_numpy(mask).to('cuda'))
    m['lam'].initialize_from_value(gin['a_lam0'])
    Q = VB(m['Z'], m['R'], m['X'], m['lam'], engine='fused')
    Q.ignore_bound_checks = True
    Q.update(repeat=4, verbose=False)
    assert type(Q.plans[0]).__name__ == 'PoissonMixturePlan'
    np.testing.assert_allclose(Q.L[:4], g['f_L'], rtol=L_RTOL)
    np.testing.assert_array_equal(m['Z'].mask, g['f_Z_mask'])
    np.testing.assert_array_equal(m['lam'].mask, g['f_lam_mask'])
    assert mask[5, 0]
    for v, exc, text in ((-1, ValueError, 'Values must be positive'),
                         (70000, NotImplementedError, 'fused Poisson-mixture block.*65534')):
        bad = torch.from_numpy(np.where(mask, x, 0)).to('cuda')
        bad[5, 0] = v
        m['X']._data = bad
        Q.plans[0].invalidate(m['X'])
        with pytest.raises(exc, match=text):
            Q.update(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import poisson_mixture
    for missing in (False, True):
        out = poisson_mixture.run(N=500, D=12, K=3, sweeps=8, missing=missing, verbose=False)
        assert out['plan'] == 'PoissonMixturePlan' and np.all(np.diff(out['L']) > -1e-6)
        assert out['accuracy'] > 0.6


# -- argument checks: nothing is launched ------------------------------------------------------------------
def test_argument_checks():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(4096)
    z.fill_(7.0)
    p = ctypes.c_void_p(z.data_ptr())
    ok = [p] * 11               # x, labels, l, lb, c, ws, S, M, Nk, scal, r_out
    for hidden, required in ((0, (0, 2, 3, 4, 5, 6, 8, 9)), (1, (0, 2, 3, 4, 5, 6, 7, 8, 9))):
        for i in required:
            args = list(ok)
            args[i] = None
            assert lib.vmp_pmm_pass(ctx, 4, 4, 4, hidden, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_pmm_pass(None, 4, 4, 4, 0, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_pass(ctx, -1, 4, 4, 0, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_pass(ctx, 4, 0, 4, 0, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_pass(ctx, 4, 4, 4, 2, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_pass(ctx, 4, 4, 65, 0, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_pmm_pass(ctx, 4, 1025, 4, 0, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_pmm_pass(ctx, 4, 1025, 4, 0, *[None] * 11) == _lib.VMP_ERR_UNSUPPORTED
    six = [p] * 6               # lam_mom, elog_pi, l, lb, c, lsum
    for i in (1, 2, 3, 4):
        args = list(six)
        args[i] = None
        assert lib.vmp_pmm_tables(ctx, 4, 4, 0, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_pmm_tables(ctx, 4, 4, 4, *six) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_tables(ctx, 4, 65, 0, *six) == _lib.VMP_ERR_UNSUPPORTED
    seven = [p] * 7             # x, mask, x_packed, flags, counts, lgam, ws
    for i in (0, 2, 3, 4, 5, 6):
        args = list(seven)
        args[i] = None
        assert lib.vmp_pmm_pack(ctx, 4, 4, 0, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_pmm_pack(ctx, 4, 4, 4, *seven) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_pack(ctx, 4, 1025, 0, *seven) == _lib.VMP_ERR_UNSUPPORTED
    upd = [p] * 7               # prior_a, prior_b, S, cnt, par, mom, bound
    for i in (0, 1, 4, 5, 6):
        args = list(upd)
        args[i] = None
        assert lib.vmp_pmm_update(ctx, 4, 4, 0, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_pmm_update(ctx, 4, 4, 2, *upd) == _lib.VMP_ERR_INVALID
    assert lib.vmp_pmm_update(ctx, 4, 65, 0, *upd) == _lib.VMP_ERR_UNSUPPORTED
    rt.synchronize()
    assert np.all(z.cpu().numpy() == 7.0)                   # nothing was launched
