"""GPU: the fused binomial-mixture block (inference/plans/binm.py, csrc/vmp_binm.hip) -- every fixture
of tests/golden/binm.npz through ``VB(..., engine='fused')`` and, for the masks the block declines,
through the generic engine; each entry point alone through the C ABI against the long-double
restatement of tests/binm_host.py at sizes that cross tile, lane-group, column-block and chunk
boundaries, both forms of the pass, fixed labels, masks, bit-identity, the flags of the pack and the
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
# the column blocks are 64 (two planes) and 128 (one plane) wide: B - 1, B, B + 1, 2 B + 1 of both
SHAPES = sorted(set([(MID[0], MID[1], K) for K in (1, 2, 15, 16, 17, 64)]
                    + [(MID[0], D, MID[2]) for D in (1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 257)]
                    + [(N, MID[1], MID[2]) for N in (0, 1, 63, 65, 257, 763)]
                    + [MID, (763, 257, 64)]))
BITS = ('S', 'T', 'Nk', 'counts', 'sum_lse', 'Nk_c', 'dots')


def _kernels():
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.binm import BINMKernels
    rt = get_runtime()
    rt.sync_stream()
    return rt, BINMKernels(rt)


def _up(rt, a):
    return rt.torch.from_numpy(np.ascontiguousarray(a)).to(rt.device)


def _device_pack(N, D, x, n, mask, strides=None):
    """dict of xp, np (N, D) uint16, flags, n_observed, n_hidden, constant, lcoef and the device
    buffers.  ``strides``: ``n`` is an int64 buffer read with these element strides."""
    from binm_host import DTYPES, trials_strides
    rt, k = _kernels()
    torch = rt.torch
    if strides is None:
        t, ts_n, ts_d = trials_strides(n, N, D)
    else:
        t, (ts_n, ts_d) = np.ascontiguousarray(n, dtype=np.int64), strides
    assert N == 0 or (N - 1) * ts_n + (D - 1) * ts_d < t.size       # every read inside the buffer
    xp = torch.zeros(max(N * D, 4), dtype=torch.int16, device=rt.device)
    np_ = torch.zeros(max(N * D, 4), dtype=torch.int16, device=rt.device)
    flags = torch.zeros(4, dtype=torch.int32, device=rt.device)
    counts = torch.zeros(3, dtype=torch.int64, device=rt.device)
    lcoef, ws = rt.zeros(1), rt.empty(3072)
    md = None if mask is None else _up(rt, np.asarray(mask).astype(np.uint8))
    k.pack(N, D, DTYPES[x.dtype.name], _up(rt, x) if N else rt.zeros(1),
           _up(rt, t) if t.size else rt.zeros(1), ts_n, ts_d, md, xp, np_, flags, counts, lcoef, ws)
    rt.synchronize()
    c = counts.cpu().numpy()
    plane = lambda p: p.cpu().numpy()[:N * D].view(np.uint16).reshape(N, D)     # noqa: E731
    return dict(xp=plane(xp), np=plane(np_), flags=flags.cpu().numpy(), n_observed=int(c[0]),
                n_hidden=int(c[1]), constant=int(c[2]), lcoef=float(lcoef.cpu().numpy()[0]),
                dev=(xp, np_))


def _device_pass(N, D, K, one_plane, dev, ncol, l1, l0, c, labels=None, want_r=False):
    """dict of S, T (D, K), Nk, counts, sum_lse, Nk_c, dots and r (or None) of vmp_binm_pass."""
    rt, k = _kernels()
    chunk, wsd = k.plan(N, D, K)
    assert chunk == 256
    S, T, Nk, counts, scal = rt.empty(D, K), rt.empty(D, K), rt.empty(K), rt.empty(D * K, 2), \
        rt.zeros(8)
    ws = rt.empty(int(wsd))
    r = rt.empty(N, K) if want_r and N else None
    lab = None if labels is None else _up(rt, labels.astype(np.int32))
    k.pass_(N, D, K, one_plane, dev[0], dev[1], None if ncol is None else _up(rt, ncol), lab,
            _up(rt, l1), _up(rt, l0), _up(rt, c), ws, S, T, Nk, counts, scal, r)
    rt.synchronize()
    s = scal.cpu().numpy()
    return dict(S=S.cpu().numpy(), T=T.cpu().numpy(), Nk=Nk.cpu().numpy(),
                counts=counts.cpu().numpy(), sum_lse=s[0], Nk_c=s[1], dots=s[2],
                r=np.zeros((0, K)) if want_r and not N else (None if r is None else r.cpu().numpy()))


def _device_tables(D, K, form, elog_p, elog_pi, ncol=None):
    rt, k = _kernels()
    l1, l0, c, cf = rt.empty(D, K), rt.empty(D, K), rt.empty(K), rt.empty(K)
    k.tables(D, K, form, None if elog_p is None else _up(rt, elog_p), _up(rt, elog_pi),
             None if ncol is None else _up(rt, ncol), l1, l0, c, None if ncol is None else cf)
    rt.synchronize()
    return tuple(t.cpu().numpy() for t in (l1, l0, c)) + (None if ncol is None else cf.cpu().numpy(),)


@pytest.mark.parametrize('N,D,K', SHAPES)
def test_every_entry_point_against_long_double_restatement(N, D, K):
    """Per quantity 8 times the deviation of the plain float64 evaluation from long double, floor
    4 ulp of the magnitude.  Two planes: trials per entry with zeros and 65534, a mask
    with a row and a column of nothing.  One plane: trials per column, no mask.  Each with and
    without labels.

    scal[2] of the two-plane form ('dots') is the sum the pass forms row by row (vmp_binm_dev.h)."""
    from binm_host import (host_pack, host_pass, host_tables, restate_pack, restate_pass,
                           restate_tables, tolerances, error, mixed_mask, pass_inputs,
                           dense_trials, PASS_QUANTITIES, MAX_TRIALS)
    for kind, masked in (('entry', True), ('column', False)):
        inp = pass_inputs(N, D, K, kind)
        x, n, rs = inp['x'], inp['n'], inp['rs']
        if kind == 'entry' and N > 9 and D > 2:
            assert n[9, 2, 0] == MAX_TRIALS and not n[8].any()
        mask = mixed_mask(N, D, rs, 64) if masked else None
        if mask is not None and N > 9 and D > 2:
            mask[9, 2] = True
        one = 0 if masked else 1
        pk = _device_pack(N, D, x, n, mask)
        hp = host_pack(x, n, mask)
        np.testing.assert_array_equal(pk['xp'], hp['xp'])
        np.testing.assert_array_equal(pk['np'], hp['np'])
        assert not pk['flags'].any()
        assert (pk['n_observed'], pk['n_hidden'], pk['constant']) \
            == (hp['n_observed'], hp['n_hidden'], hp['constant'])
        assert N == 0 or pk['constant'] == (1 if one or N == 1 else 0)
        ld, f64 = restate_pack(x, n, mask), restate_pack(x, n, mask, np.float64)
        tol, dev = tolerances(ld, f64, ('lcoef',))
        err = error(pk['lcoef'], ld['lcoef'])
        print('lcoef %s %s: float64 deviation %.3g, kernel %.3g, allowed %.3g'
              % ((N, D, K), kind, dev['lcoef'], err, tol['lcoef']))
        assert err <= tol['lcoef']
        # the tables: as they are and centred
        ncol = dense_trials(n, max(N, 1), D)[0].astype(np.float64) if one else None
        names = ('l1', 'l0', 'c', 'cf') if one else ('l1', 'l0', 'c')
        for form in (0, 1):
            got = _device_tables(D, K, form, inp['elog_p'], inp['elog_pi'], ncol)
            ldt = restate_tables(inp['elog_p'], inp['elog_pi'], D, K, form, ncol)
            f64t = restate_tables(inp['elog_p'], inp['elog_pi'], D, K, form, ncol, np.float64)
            tol, dev = tolerances(dict(zip(names, ldt)), dict(zip(names, f64t)), names)
            for nm, g_, r_ in zip(names, got, ldt):
                assert error(g_, r_) <= tol[nm], (nm, form)
        l1, l0, c, cf = got
        for g_, h_ in zip(got, host_tables(D, K, 1, inp['elog_p'], inp['elog_pi'], ncol)):
            if g_ is not None:
                np.testing.assert_array_equal(g_, h_)
        # Z under its prior: a null table
        z1, z0, zc, _ = _device_tables(D, K, 1, None, inp['elog_pi'])
        assert not z1.any() and not z0.any() and zc.max() == 0
        # the pass
        cc = cf if one else c
        got = _device_pass(N, D, K, one, pk['dev'], ncol, l1, l0, cc, want_r=True)
        ld = restate_pass(x, n, mask, l1, l0, cc, one)
        f64 = restate_pass(x, n, mask, l1, l0, cc, one, np.float64)
        tol, dev = tolerances(ld, f64, PASS_QUANTITIES)
        host = host_pass(N, D, K, one, hp['xp'], hp['np'], ncol, None, l1, l0, cc, want_r=True)
        for key in PASS_QUANTITIES:
            err, herr = error(got[key], ld[key]), error(host[key], ld[key])
            print('%s %s one_plane=%d: float64 deviation %.3g, kernel %.3g, host build %.3g, '
                  'allowed %.3g' % (key, (N, D, K), one, dev[key], err, herr, tol[key]))
            assert err <= tol[key], (key, one, err, tol[key])
        if N and K > 1:                         # soft rows: a condition on the inputs
            assert np.mean(np.asarray(ld['r'], dtype=np.float64).max(axis=1) < 0.99) >= 0.5
        if masked and N > 2:
            # the row of nothing: r = softmax(c); a column of nothing: exact zeros
            np.testing.assert_allclose(got['r'][2], np.exp(c) / np.exp(c).sum(), rtol=1e-13)
        if masked and D > 2 and N:
            assert np.all(got['S'][1] == 0) and np.all(got['T'][1] == 0)
        # fixed labels: exact integer counts, lse = 0
        got = _device_pass(N, D, K, one, pk['dev'], ncol, l1, l0, cc, labels=inp['labels'],
                           want_r=True)
        m = np.ones((N, D), dtype=bool) if mask is None else mask
        hot = np.eye(K)[inp['labels']]
        np.testing.assert_array_equal(got['r'], hot)
        hot = hot * m.any(axis=1)[:, None]
        np.testing.assert_array_equal(got['Nk'], hot.sum(0))
        np.testing.assert_array_equal(got['S'], np.where(m, x, 0).astype(float).T @ hot)
        np.testing.assert_array_equal(got['T'],
                                      np.where(m, dense_trials(n, N, D), 0).astype(float).T @ hot)
        np.testing.assert_array_equal(got['counts'].reshape(D, K, 2)[..., 1], got['T'] - got['S'])
        assert got['sum_lse'] == 0


@pytest.mark.parametrize('N,D,K', [MID, (763, 257, 64), (257, 129, 16), (65, 65, 17)])
def test_bit_identity(N, D, K):
    """Two calls, with and without r_out, different junk at hidden positions, a mask of ones
    against no mask, in both forms: the same bits."""
    from binm_host import mixed_mask, pass_inputs, host_tables, junk_at_hidden, dense_trials
    for kind in ('entry', 'column'):
        inp = pass_inputs(N, D, K, kind)
        x, n = inp['x'], inp['n']
        m = mixed_mask(N, D, inp['rs'], 64)
        ncol = dense_trials(n, N, D)[0].astype(np.float64)
        l1, l0, c, cf = host_tables(D, K, 1, inp['elog_p'], inp['elog_pi'], ncol)

        def run(xx, mask, want_r=True):
            pk = _device_pack(N, D, xx, n, mask)
            one = 1 if pk['constant'] and not pk['n_hidden'] else 0
            out = _device_pass(N, D, K, one, pk['dev'], ncol, l1, l0, cf if one else c,
                               want_r=want_r)
            out.update(xp=pk['xp'], np=pk['np'], lcoef=pk['lcoef'], one=one)
            return out
        a, b, nr = run(x, m), run(x, m), run(x, m, want_r=False)
        j1 = run(junk_at_hidden(x, m, np.nan), m)
        junk = junk_at_hidden(x, m, 0.0)
        junk[~m] = np.resize([-1.0, 1e300, np.nan, 0.5, 70000.0], int((~m).sum()))
        j2 = run(junk, m)
        assert a['one'] == 0
        for key in BITS + ('r', 'xp', 'np', 'lcoef'):
            for other in (b, j1, j2):
                np.testing.assert_array_equal(a[key], other[key], err_msg=key)
        for key in BITS:
            np.testing.assert_array_equal(a[key], nr[key], err_msg=key)
        u, o = run(x, None), run(x, np.ones((N, D), dtype=bool))
        w = run(x, None, want_r=False)
        assert u['one'] == o['one'] == (1 if kind == 'column' else 0)
        for key in BITS + ('r', 'xp', 'np', 'lcoef'):
            np.testing.assert_array_equal(u[key], o[key], err_msg=key)
        for key in BITS:
            np.testing.assert_array_equal(u[key], w[key], err_msg=key)


def test_pack_dtypes_every_flag_the_cap_and_strided_trials():
    from binm_host import host_pack, pass_inputs, HIDDEN, dense_trials
    N, D, K = MID
    inp = pass_inputs(N, D, K, 'entry')
    x, n, rs = inp['x'], inp['n'].copy(), inp['rs']
    mask = rs.rand(N, D) < 0.7
    mask[5, 6], mask[6, 6] = True, False
    n[5, 6, 0] = 20
    x[5, 6], x[9, 2] = 3, 5                         # (9, 2) has 65534 trials: below every n used here
    want = host_pack(x, n, mask)
    for a in (x.astype(np.float64), x.astype(np.int64), x.astype(np.int32), x.astype(np.uint8)):
        got = _device_pack(N, D, a, n, mask)
        np.testing.assert_array_equal(got['xp'], want['xp'])
        np.testing.assert_array_equal(got['np'], want['np'])
        assert got['lcoef'] == want['lcoef'] and got['n_hidden'] == want['n_hidden']
        assert got['constant'] == 0 and not got['flags'].any()
    # trials of every accepted shape, read in place
    for t in (np.array(65534), rs.randint(40, 50, size=(D, 1)), rs.randint(40, 50, size=(N, 1, 1)),
              rs.randint(40, 50, size=(N, D, 1))):
        got, h = _device_pack(N, D, x, t, mask), host_pack(x, t, mask)
        np.testing.assert_array_equal(got['np'], np.where(mask, dense_trials(t, N, D), HIDDEN))
        assert got['constant'] == h['constant'] == (1 if t.ndim < 3 else 0)
        assert got['lcoef'] == h['lcoef'] and not got['flags'].any()
    # flags: (negative, no integer, above the trials, trials above the cap); junk where hidden
    for v, flags in ((-1.0, (1, 0, 0, 0)), (0.5, (0, 1, 0, 0)), (np.nan, (0, 1, 0, 0)),
                     (1e300, (0, 0, 1, 0)), (21.0, (0, 0, 1, 0))):
        bad = x.astype(np.float64)
        bad[5, 6] = v
        got = _device_pack(N, D, bad, n, mask)
        assert tuple(got['flags']) == flags and got['np'][5, 6] == HIDDEN \
            and got['xp'][5, 6] == 0, v
        hid = x.astype(np.float64)
        hid[6, 6] = v
        got = _device_pack(N, D, hid, n, mask)
        assert not got['flags'].any() and got['np'][6, 6] == HIDDEN and got['xp'][6, 6] == 0
        np.testing.assert_array_equal(got['xp'], want['xp'])
    for v, flags in ((-1, (1, 0, 0, 0)), (21, (0, 0, 1, 0)), (2 ** 40, (0, 0, 1, 0))):
        bad = x.copy()
        bad[5, 6] = v
        got = _device_pack(N, D, bad, n, mask)
        assert tuple(got['flags']) == flags and got['np'][5, 6] == HIDDEN, v
    for a in (x.copy(), x.astype(np.float64)):
        a[5, 6] = 65534                             # exactly the cap: accepted
        n[5, 6, 0] = 65534
        got = _device_pack(N, D, a, n, mask)
        assert not got['flags'].any() and got['xp'][5, 6] == 65534 and got['np'][5, 6] == 65534
        n[5, 6, 0] = 65535                          # one above: flagged where observed only
        assert tuple(_device_pack(N, D, a, n, mask)['flags']) == (0, 0, 0, 1)
        n[5, 6, 0], n[6, 6, 0] = 65534, 65535
        assert not _device_pack(N, D, a, n, mask)['flags'].any()
        n[6, 6, 0] = 20


# -- end to end ------------------------------------------------------------------------------------------
def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    return dict(nodes=nodes, VB=VB, vb_kwargs=kw)


def test_fixtures_on_the_fused_block():
    """Fails without the feature: the model cannot be built."""
    from binm_models import run_binm_cases, FUSED_CASES
    from test_binm_host import check_fixture, _golden, PER_CASE
    from bayespy_amd.inference.plans.binm import BinomialMixturePlan
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_binm_cases(_mods(engine='fused'), gin, only=FUSED_CASES)
    for tag in FUSED_CASES:
        assert isinstance(res[tag + '_plan'].plans[0], BinomialMixturePlan)
    assert check_fixture(res, g, FUSED_CASES) == len(FUSED_CASES) * PER_CASE
    for k in ('L', 'Z_u0', 'P_u0', 'R_u0'):
        np.testing.assert_array_equal(res['g_' + k], res['a_' + k], err_msg=k)
    form = {t: res[t + '_plan'].plans[0].one_plane for t in FUSED_CASES}
    assert form == dict(a=1, b=1, c=1, d=0, e=0, f=0, g=1)


def test_the_fused_block_and_the_generic_engine_agree_on_case_d():
    from binm_models import run_binm_cases
    from test_binm_host import _golden
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        fused = run_binm_cases(_mods(engine='fused'), gin, only=('d',))
        generic = run_binm_cases(_mods(engine='generic'), gin, only=('d',))
    assert type(generic['d_plan'].plans[0]).__name__ == 'GenericPlan'
    np.testing.assert_allclose(fused['d_L'], generic['d_L'], rtol=L_RTOL)


def test_fixtures_on_the_generic_engine_with_every_trials_shape_and_mask():
    """Fails without the feature, when the node is built.  Trials of every accepted shape ((a),
    (c), (d), (e)), a full mask (f), the scalar mask (h) and a mask that broadcasts over the
    columns (i), which the fused block declines."""
    from binm_models import run_binm_cases
    from test_binm_host import check_fixture, _golden, PER_CASE
    g, gin = _golden()
    cases = ('a', 'c', 'd', 'e', 'f', 'h', 'i')
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = run_binm_cases(_mods(engine='generic'), gin, only=cases)
    for tag in cases:
        assert type(res[tag + '_plan'].plans[0]).__name__ == 'GenericPlan'
    assert check_fixture(res, g, cases) == len(cases) * PER_CASE
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = run_binm_cases(_mods(), gin, only=('a',))         # the default engine
    assert type(res['a_plan'].plans[0]).__name__ == 'GenericPlan'
    np.testing.assert_allclose(res['a_L'], g['a_L'], rtol=L_RTOL)


def test_a_device_tensor_a_device_mask_invalid_counts_and_the_example():
    import torch
    from binm_models import build_binm
    from test_binm_host import _golden
    from bayespy_amd.inference import VB
    g, gin = _golden()
    x, n, mask = gin['d_x'], gin['d_n'], gin['f_mask']
    m = build_binm(_mods(), x, n, 3, observe=False)
    m['X'].observe(np.where(mask, x, 0), mask=torch.from_numpy(mask).to('cuda'))
    m['P'].initialize_from_value(gin['d_p0'])
    Q = VB(m['Z'], m['R'], m['X'], m['P'], engine='fused')
    Q.ignore_bound_checks = True
    Q.update(repeat=4, verbose=False)
    assert type(Q.plans[0]).__name__ == 'BinomialMixturePlan'
    np.testing.assert_allclose(Q.L[:4], g['f_L'], rtol=L_RTOL)
    np.testing.assert_array_equal(m['Z'].mask, g['f_Z_mask'])
    np.testing.assert_array_equal(m['P'].mask, g['f_P_mask'])
    i, j = np.argwhere(mask)[7]                     # an observed entry
    for v, text in ((-1, 'Invalid count'), (70000, 'Invalid count')):
        bad = torch.from_numpy(np.where(mask, x, 0)).to('cuda')
        bad[i, j] = v
        m['X']._data = bad
        Q.plans[0].invalidate(m['X'])
        with pytest.raises(ValueError, match=text):
            Q.update(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, 'examples'))
    import binomial_mixture
    for missing in (False, True):
        out = binomial_mixture.run(N=500, D=12, K=3, sweeps=8, missing=missing, verbose=False)
        assert out['plan'] == 'BinomialMixturePlan' and np.all(np.diff(out['L']) > -1e-6)
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
    # x, n, ncol, labels, l1, l0, c, ws, S, T, Nk, counts, scal, r_out
    ok = [p] * 14
    for one, required in ((0, (0, 1, 4, 5, 6, 7, 8, 9, 10, 11, 12)),
                          (1, (0, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12))):
        for i in required:
            args = list(ok)
            args[i] = None
            assert lib.vmp_binm_pass(ctx, 4, 4, 4, one, *args) == _lib.VMP_ERR_INVALID, (one, i)
    assert lib.vmp_binm_pass(None, 4, 4, 4, 0, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_binm_pass(ctx, -1, 4, 4, 0, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_binm_pass(ctx, 4, 0, 4, 0, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_binm_pass(ctx, 4, 4, 4, 2, *ok) == _lib.VMP_ERR_INVALID
    assert lib.vmp_binm_pass(ctx, 4, 4, 65, 0, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_binm_pass(ctx, 4, 1025, 4, 1, *ok) == _lib.VMP_ERR_UNSUPPORTED
    assert lib.vmp_binm_pass(ctx, 4, 1025, 4, 0, *[None] * 14) == _lib.VMP_ERR_UNSUPPORTED
    seven = [p] * 7             # elog_p, elog_pi, ncol, l1, l0, c, cfold
    for i in (1, 3, 4, 5):
        args = list(seven)
        args[i] = None
        assert lib.vmp_binm_tables(ctx, 4, 4, 0, *args) == _lib.VMP_ERR_INVALID, i
    assert lib.vmp_binm_tables(ctx, 4, 4, 2, *seven) == _lib.VMP_ERR_INVALID
    assert lib.vmp_binm_tables(ctx, 4, 65, 0, *seven) == _lib.VMP_ERR_UNSUPPORTED
    # x, trials, (strides), mask, x_packed, n_packed, flags, counts, lcoef, ws
    for i in (0, 1, 3, 4, 5, 6, 7, 8):
        args = [p] * 9
        args[i] = None
        assert lib.vmp_binm_pack(ctx, 4, 4, 0, args[0], args[1], 4, 1, *args[2:]) \
            == _lib.VMP_ERR_INVALID, i
    nine = [p] * 9
    assert lib.vmp_binm_pack(ctx, 4, 4, 4, nine[0], nine[1], 4, 1, *nine[2:]) == _lib.VMP_ERR_INVALID
    assert lib.vmp_binm_pack(ctx, 4, 4, 0, nine[0], nine[1], -1, 1, *nine[2:]) \
        == _lib.VMP_ERR_INVALID
    assert lib.vmp_binm_pack(ctx, 4, 1025, 0, nine[0], nine[1], 0, 0, *nine[2:]) \
        == _lib.VMP_ERR_UNSUPPORTED
    rt.synchronize()
    assert np.all(z.cpu().numpy() == 7.0)                   # nothing was launched
