"""CPU: the fused binomial-mixture block without a device -- the plan's host logic on the kernel
double tests/binm_host.py (CPUBINMKernels) against every fixture of tests/golden/binm.npz (live
reference, tools/make_golden_binm.py), masks, the identities between the forms and with the
Bernoulli block, the g++ build of the device header csrc/vmp_binm_dev.h against a long-double
restatement, the same source under -fsanitize=address,undefined as a stand-alone program, a save /
load round trip and the C ABI."""
import ctypes
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

L_RTOL = 1e-9                               # DESIGN 4.22, as for every block
MOM_TOL = dict(rtol=1e-6, atol=1e-9)        # tests/test_pmm_host.py
PER_CASE = 1 + 4 + 3 + 2                    # L, four bound terms, three moments, two masks


def _mods(after=None, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    m = dict(nodes=nodes, VB=VB, vb_kwargs=kw)
    if after is not None:
        m['after_vb'] = after
    return m


def _on_double(Q):
    from bayespy_amd.device import Runtime
    from binm_host import CPUBINMKernels
    plan = Q.plans[0]
    assert type(plan).__name__ == 'BinomialMixturePlan'
    rt = Runtime(device='cpu')
    plan._rt, plan._kernels = rt, CPUBINMKernels(rt)


def _golden():
    g = np.load(os.path.join(GOLDEN, 'binm.npz'))
    gin = {k[3:]: (g[k].astype(np.int64) if k.endswith(('_x', '_n')) else g[k])
           for k in g.files if k.startswith('in_')}
    return g, gin


def _model(tag='d', **kw):
    from binm_models import build_binm
    gin = _golden()[1]
    return build_binm(_mods(), gin[tag + '_x'], gin[tag + '_n'], gin[tag + '_p0'].shape[1], **kw)


def _nodes(m):
    return [m['Z'], m['R'], m['X'], m['P']]


def check_fixture(res, g, cases):
    """Every stored quantity of the cases; returns how many were compared."""
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan') or k[0] not in cases:
            continue
        if k.endswith('_mask'):
            np.testing.assert_array_equal(*np.broadcast_arrays(v, g[k]), err_msg=k)
        elif k.endswith('_u0'):
            np.testing.assert_allclose(v, g[k], err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(v, g[k], err_msg=k, rtol=L_RTOL, atol=1e-9)
        checked += 1
    return checked


# -- the plan on the kernel double ---------------------------------------------------------------------
def test_plan_reproduces_every_fixture_on_the_kernel_double():
    """Fails without the feature: the model cannot be built."""
    from binm_models import run_binm_cases, FUSED_CASES
    g, gin = _golden()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = run_binm_cases(_mods(_on_double, engine='fused'), gin, only=FUSED_CASES)
    assert check_fixture(res, g, FUSED_CASES) == len(FUSED_CASES) * PER_CASE
    calls = res['a_plan'].plans[0].kernels.calls
    # scalar trials, nothing hidden: the one-plane form; set-up pass + one per sweep; the
    # responsibilities only on request
    assert calls.count('pass_one') == 1 + 4 and calls.count('pass_r_one') == 1
    assert calls.count('pack') == 1 and 'pass' not in calls
    # a mask of ones: the same form and the bits of the unmasked run
    assert res['g_plan'].plans[0].kernels.calls == calls
    for k in ('L', 'Z_u0', 'P_u0', 'R_u0', 'Z_Lterm', 'P_Lterm', 'X_Lterm'):
        np.testing.assert_array_equal(res['g_' + k], res['a_' + k], err_msg=k)
    # the forms of the other cases
    form = {t: res[t + '_plan'].plans[0].one_plane for t in FUSED_CASES}
    assert form == dict(a=1, b=1, c=1, d=0, e=0, f=0, g=1)
    # (f): the row of nothing has softmax(c), its column of P stays at the prior
    plan = res['f_plan'].plans[0]
    assert plan.n_hidden > 0 and 'pass' in plan.kernels.calls
    c = plan.c.numpy()                    # of the last Z update, which R's update followed
    np.testing.assert_allclose(res['f_Z_u0'][4, 0], np.exp(c) / np.exp(c).sum(), rtol=1e-12)
    assert np.all(plan.S.numpy()[2] == 0) and np.all(plan.T.numpy()[2] == 0)
    np.testing.assert_array_equal(plan.alpha_p.numpy().reshape(4, 3, 2)[2],
                                  np.broadcast_to([0.5, 0.5], (3, 2)))
    assert not res['f_Z_mask'][4, 0] and not res['f_P_mask'][2, 0]


def test_a_column_at_its_prior_has_a_bound_term_of_exactly_zero():
    from bayespy_amd.device import Runtime
    from binm_host import CPUBINMKernels
    import torch
    rs = np.random.RandomState(5)
    D, K = 6, 3
    k = CPUBINMKernels(Runtime(device='cpu'))
    prior = torch.from_numpy(rs.gamma(2.0, size=(D * K, 2)))
    counts = torch.from_numpy(rs.gamma(3.0, size=(D * K, 2)))
    alpha, elog, ws, b = (torch.zeros(n, dtype=torch.float64).reshape(s)
                          for n, s in ((2 * D * K, (D * K, 2)), (2 * D * K, (D * K, 2)),
                                       (1024, (1024,)), (1, (1,))))
    k.dirichlet(D * K, 2, 2, 1, prior, None, alpha, elog, ws, b)
    assert float(b[0]) == 0.0
    k.dirichlet(D * K, 2, 2, 1, prior, 0 * counts, alpha, elog, ws, b)
    assert float(b[0]) == 0.0
    k.dirichlet(D * K, 2, 2, 1, prior, counts, alpha, elog, ws, b)
    assert float(b[0]) != 0.0


def test_hidden_values_are_never_interpreted_and_reobserving_keeps_the_posteriors():
    from binm_models import run_binm_cases
    g, gin = _golden()
    Q = run_binm_cases(_mods(_on_double, engine='fused'), gin, only=('f',))['f_plan']
    plan = Q.plans[0]
    X, P = Q['X'], Q['P']
    u = P.get_moments()[0]
    S0, xp0, np0 = plan.S.numpy().copy(), plan.xp.numpy().copy(), plan.np_.numpy().copy()
    mask = gin['f_mask']
    junk = np.where(mask, gin['d_x'], np.nan).astype(np.float64)
    junk[~mask] = np.resize([np.nan, -1.0, 1e300], int((~mask).sum()))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        X._data, X._mask = junk, mask           # past the host check of observe, as a tensor is
        plan.invalidate(X)
        np.testing.assert_array_equal(P.get_moments()[0], u)
    assert Q.plans[0] is plan
    np.testing.assert_array_equal(plan.xp.numpy(), xp0)
    np.testing.assert_array_equal(plan.np_.numpy(), np0)
    np.testing.assert_array_equal(plan.S.numpy(), S0)
    # another mask of the full shape: packed again, the posteriors stay
    m2 = mask.copy()
    m2[4] = True
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        X.observe(np.where(m2, gin['d_x'], 0), mask=m2)
        np.testing.assert_array_equal(P.get_moments()[0], u)
    assert Q.plans[0] is plan and plan.kernels.calls.count('pack') == 3
    assert bool(Q['Z'].mask[4, 0]) is True
    X.observe(gin['d_x'])
    np.testing.assert_array_equal(P.get_moments()[0], u)
    assert plan.n_hidden == 0 and plan.one_plane == 0       # trials per entry: still two planes
    Q.update(repeat=1, verbose=False)
    assert np.isfinite(Q.L[4])


def test_reobserving_switches_between_the_forms():
    from binm_models import run_binm_cases
    g, gin = _golden()
    Q = run_binm_cases(_mods(_on_double, engine='fused'), gin, only=('a',), n_iter=2)['a_plan']
    plan, X = Q.plans[0], Q['X']
    assert plan.one_plane == 1
    r1 = Q['Z'].get_moments()[0]
    m = np.ones((300, 7), dtype=bool)
    m[5, 3] = False
    X.observe(np.where(m, gin['a_x'], 0), mask=m)
    r2 = Q['Z'].get_moments()[0]
    assert plan.one_plane == 0 and plan.kernels.calls[-1] == 'pass_r'
    # one hidden entry of 2100: the responsibilities of the other rows do not move
    np.testing.assert_allclose(np.delete(r2, 5, axis=0), np.delete(r1, 5, axis=0), rtol=0,
                               atol=1e-12)
    X.observe(gin['a_x'])
    Q.update(repeat=1, verbose=False)
    assert plan.one_plane == 1 and np.isfinite(Q.L[2])


def test_invalid_counts_raise_the_reference_exceptions():
    from bayespy_amd.inference import VB
    _, gin = _golden()
    for bad, text in ((0.5, 'Counts must be integer'), (np.nan, 'Counts must be integer'),
                      (-1.0, 'Invalid count'), (1e6, 'Invalid count')):
        m = _model()
        Q = VB(*_nodes(m), engine='fused')
        _on_double(Q)
        x = gin['d_x'].astype(np.float64)
        x[3, 0] = bad
        m['X']._data = x
        with pytest.raises(ValueError, match=text):
            Q.update(verbose=False)


def test_save_load_round_trip_and_a_differing_mask_is_refused(tmp_path):
    from binm_models import run_binm_cases
    g, gin = _golden()
    Q = run_binm_cases(_mods(_on_double, engine='fused'), gin, only=('f',))['f_plan']
    fn = str(tmp_path / 'binm.ckpt')
    Q.save(filename=fn)
    L4 = Q.L[:4].copy()
    Q.update(repeat=2, verbose=False)
    L6 = Q.L[:6].copy()
    Q.load(filename=fn)
    assert Q.iter == 4
    np.testing.assert_array_equal(Q.L[:4], L4)
    Q.update(repeat=2, verbose=False)
    np.testing.assert_array_equal(Q.L[:6], L6)
    other = run_binm_cases(_mods(_on_double, engine='fused'), gin, only=('d',))['d_plan']
    with pytest.raises(ValueError, match='checkpoint was saved with a mask on X'):
        other.load(filename=fn)


def test_one_trial_everywhere_is_the_bernoulli_block():
    """Binomial with n = 1 against the Bernoulli block's host double on the inputs of
    tests/golden/bmm_fused.npz: every bound term and moment to L_RTOL / MOM_TOL."""
    import bmm_models
    from bmm_host import CPUBMMKernels
    from bayespy_amd.device import Runtime
    import bayespy_amd.nodes as nodes
    f = np.load(os.path.join(GOLDEN, 'bmm_fused.npz'))
    gin = {k[3:]: f[k] for k in f.files if k.startswith('in_')}

    def bern_double(Q):
        rt = Runtime(device='cpu')
        Q.plans[0]._rt, Q.plans[0]._kernels = rt, CPUBMMKernels(rt)

    class AsBinomial:
        """The node module with Mixture(Z, Bernoulli, P) built as Mixture(Z, Binomial, 1, P)."""
        def __getattr__(self, name):
            return getattr(nodes, name)

        @staticmethod
        def Mixture(Z, cls, P, **kw):
            assert cls is nodes.Bernoulli
            return nodes.Mixture(Z, nodes.Binomial, 1, P, **kw)
    AsBinomial.Bernoulli = nodes.Bernoulli
    want = bmm_models.run_bmm_cases(_mods(bern_double, engine='fused'), gin)
    mods = _mods(_on_double, engine='fused')
    mods['nodes'] = AsBinomial()
    got = bmm_models.run_bmm_cases(mods, gin)
    n = 0
    for k, v in want.items():
        if k.endswith('_plan'):
            continue
        if k.endswith('_u0'):
            np.testing.assert_allclose(got[k], v, err_msg=k, **MOM_TOL)
        else:
            np.testing.assert_allclose(got[k], v, err_msg=k, rtol=L_RTOL, atol=1e-9)
        n += 1
    assert n == len(bmm_models.CASES) * 8


# -- the device header on the host ---------------------------------------------------------------------
def test_pack_dtypes_hidden_values_the_flags_the_cap_and_strided_trials():
    from binm_host import host_pack, restate_pack, HIDDEN
    rs = np.random.RandomState(7)
    N, D = 37, 9
    n = rs.randint(0, 30, size=(N, D, 1))
    n[0, 0, 0], n[1, 1, 0] = 0, 1
    nd = n[..., 0]
    x = rs.binomial(nd, 0.4)
    mask = rs.rand(N, D) < 0.7
    for a in (x.astype(np.int64), x.astype(np.float64), x.astype(np.int32), x.astype(np.uint8)):
        o = host_pack(a, n)
        assert not o['flags'].any() and (o['n_observed'], o['n_hidden']) == (x.size, 0)
        assert o['constant'] == 0
        np.testing.assert_array_equal(o['xp'], x)
        np.testing.assert_array_equal(o['np'], nd)
        o = host_pack(a, n, mask)
        assert not o['flags'].any()
        assert (o['n_observed'], o['n_hidden']) == (int(mask.sum()), int((~mask).sum()))
        np.testing.assert_array_equal(o['xp'], np.where(mask, x, 0))
        np.testing.assert_array_equal(o['np'], np.where(mask, nd, HIDDEN))
        r = restate_pack(a, n, mask)
        np.testing.assert_array_equal(r['xp'], o['xp'])
        np.testing.assert_array_equal(r['np'], o['np'])
        assert abs(o['lcoef'] - float(r['lcoef'])) <= 4 * np.spacing(float(r['lcoef']))
    # every accepted shape of the trials is read in place
    for t in (np.array(29), rs.randint(29, 40, size=(D, 1)), rs.randint(29, 40, size=(N, 1, 1))):
        o = host_pack(x, t, mask)
        want = np.broadcast_to(t.reshape((1,) * (3 - t.ndim) + t.shape)[..., 0], (N, D))
        np.testing.assert_array_equal(o['np'], np.where(mask, want, HIDDEN))
        assert o['constant'] == (0 if t.ndim == 3 else 1) and not o['flags'].any()
    assert host_pack(x, np.broadcast_to(n[:1], (N, D, 1)).copy() + 30)['constant'] == 1
    # flags: (negative, no integer, above the trials, trials above the cap)
    mask[5, 8], mask[6, 8] = True, False
    n[5, 8, 0] = 20
    wx, wn = np.where(mask, x, 0), np.where(mask, n[..., 0], HIDDEN)
    wx[5, 8], wn[5, 8] = 0, HIDDEN
    for v, flags in ((np.nan, (0, 1, 0, 0)), (-1.0, (1, 0, 0, 0)), (1e300, (0, 0, 1, 0)),
                     (0.5, (0, 1, 0, 0)), (-0.5, (0, 1, 0, 0)), (21.0, (0, 0, 1, 0)),
                     (np.inf, (0, 0, 1, 0)), (-np.inf, (1, 0, 0, 0))):
        hidden = x.astype(np.float64)
        hidden[6, 8] = v
        hidden[5, 8] = 3
        o = host_pack(hidden, n, mask)
        assert not o['flags'].any() and o['xp'][6, 8] == 0 and o['np'][6, 8] == HIDDEN
        bad = x.astype(np.float64)
        bad[5, 8] = v
        o = host_pack(bad, n, mask)
        assert tuple(o['flags']) == flags, (v, o['flags'])
        np.testing.assert_array_equal(o['xp'], wx)
        np.testing.assert_array_equal(o['np'], wn)
        np.testing.assert_array_equal(restate_pack(bad, n, mask)['flags'], flags)
    for v, flags in ((-1, (1, 0, 0, 0)), (21, (0, 0, 1, 0)), (2 ** 40, (0, 0, 1, 0)),
                     (-2 ** 40, (1, 0, 0, 0))):
        bad = x.astype(np.int64)
        bad[5, 8] = v
        o = host_pack(bad, n, mask)
        assert tuple(o['flags']) == flags and o['np'][5, 8] == HIDDEN
    # the cap of the trials: 65534 is taken, 65535 is flagged where observed and only there
    for dt in (np.int64, np.float64):
        ok = x.astype(dt)
        ok[5, 8] = 65534
        n[5, 8, 0] = 65534
        o = host_pack(ok, n, mask)
        assert not o['flags'].any() and o['xp'][5, 8] == 65534 and o['np'][5, 8] == 65534
        n[5, 8, 0] = 65535
        assert tuple(host_pack(ok, n, mask)['flags']) == (0, 0, 0, 1)
        ok[5, 8], ok[6, 8] = 3, 3
        n[5, 8, 0], n[6, 8, 0] = 20, 65535
        assert not host_pack(ok, n, mask)['flags'].any()
        n[6, 8, 0] = 20


HOST_SHAPES = [(0, 5, 3), (1, 1, 1), (65, 3, 2), (300, 70, 5), (257, 4, 16), (300, 129, 17),
               (515, 65, 2), (763, 257, 64)]


@pytest.mark.parametrize('N,D,K', HOST_SHAPES)
def test_host_build_of_the_device_header_against_long_double(N, D, K):
    """The rule of DESIGN 4.14: the host build may differ from the long-double restatement by 8
    times the deviation of the plain float64 evaluation, floor 4 ulp of the magnitude."""
    from binm_host import (host_pack, host_pass, host_tables, restate_pack, restate_pass,
                           restate_tables, tolerances, error, mixed_mask, pass_inputs, binm_host,
                           dense_trials, PASS_QUANTITIES)
    assert binm_host().binm_chunk_rows(N, D, K) == 256
    for kind, masked in (('entry', True), ('entry', False), ('column', False), ('scalar', True)):
        inp = pass_inputs(N, D, K, kind)
        x, n, rs = inp['x'], inp['n'], inp['rs']
        mask = mixed_mask(N, D, rs, binm_host().binm_dblock()) if masked else None
        pk = host_pack(x, n, mask)
        one = 1 if kind != 'entry' and not masked else 0
        assert not pk['flags'].any() and pk['n_hidden'] == (0 if mask is None else (~mask).sum())
        assert N == 0 or pk['constant'] == (0 if kind == 'entry' and N > 1 else 1)
        ld, f64 = restate_pack(x, n, mask), restate_pack(x, n, mask, np.float64)
        tol, _ = tolerances(ld, f64, ('lcoef',))
        assert error(pk['lcoef'], ld['lcoef']) <= tol['lcoef']
        ncol = dense_trials(n, max(N, 1), D)[0].astype(np.float64) if one else None
        for form in (0, 1):                     # as they are, centred (the pass)
            l1, l0, c, cf = host_tables(D, K, form, inp['elog_p'], inp['elog_pi'], ncol)
            want = restate_tables(inp['elog_p'], inp['elog_pi'], D, K, form, ncol, np.float64)
            for got, w in zip((l1, l0, c), want):
                np.testing.assert_allclose(got, w, rtol=1e-14, atol=1e-12)
            if one:
                ld = restate_tables(inp['elog_p'], inp['elog_pi'], D, K, form, ncol)
                tol, _ = tolerances(dict(cf=ld[3]), dict(cf=want[3]), ('cf',))
                assert error(cf, ld[3]) <= tol['cf']
        cc = cf if one else c
        got = host_pass(N, D, K, one, pk['xp'], pk['np'], ncol, None, l1, l0, cc, want_r=True)
        ld = restate_pass(x, n, mask, l1, l0, cc, one)
        f64 = restate_pass(x, n, mask, l1, l0, cc, one, np.float64)
        tol, dev = tolerances(ld, f64, PASS_QUANTITIES)
        for key in PASS_QUANTITIES:
            err = error(got[key], ld[key])
            assert err <= tol[key], (key, kind, masked, err, tol[key])
        if N and K > 1:                         # soft rows: a condition on the inputs
            assert np.mean(np.asarray(ld['r'], dtype=np.float64).max(axis=1) < 0.99) >= 0.5
        # fixed labels: one-hot statistics, lse = 0
        h = host_pass(N, D, K, one, pk['xp'], pk['np'], ncol, inp['labels'], l1, l0, cc,
                      want_r=True)
        m = np.ones((N, D), dtype=bool) if mask is None else mask
        hot = np.eye(K)[inp['labels']] * m.any(axis=1)[:, None]
        np.testing.assert_array_equal(h['Nk'], hot.sum(0))
        np.testing.assert_array_equal(h['S'], np.where(m, x, 0).astype(float).T @ hot)
        np.testing.assert_array_equal(h['T'], np.where(m, dense_trials(n, N, D), 0).astype(float).T
                                      @ hot)
        np.testing.assert_array_equal(h['counts'][:, 1], (h['T'] - h['S']).reshape(-1))
        assert h['sum_lse'] == 0
        # a mask of ones packs to the bits of no mask
        for key in ('xp', 'np'):
            np.testing.assert_array_equal(host_pack(x, n)[key],
                                          host_pack(x, n, np.ones((N, D)))[key])


@pytest.mark.parametrize('N,D,K', [(65, 3, 2), (300, 70, 5), (300, 129, 17)])
def test_the_two_forms_agree_on_constant_trials(N, D, K):
    """Both forms on trials per column with nothing hidden, each against the long-double
    restatement of the two-plane form under the rule above: r, the statistics, the message to P
    and the entropy sum lse - Nk . c - scal[2], which does not depend on where n l0 stands."""
    from binm_host import (host_pack, host_pass, host_tables, restate_pass, tolerances, error,
                           pass_inputs, dense_trials)
    inp = pass_inputs(N, D, K, 'column')
    x, n = inp['x'], inp['n']
    pk = host_pack(x, n)
    assert pk['constant'] == 1 and pk['n_hidden'] == 0
    ncol = dense_trials(n, N, D)[0].astype(np.float64)
    l1, l0, c, cf = host_tables(D, K, 1, inp['elog_p'], inp['elog_pi'], ncol)
    keys = ('r', 'Nk', 'S', 'T', 'counts', 'entropy')

    def with_entropy(o):
        o = dict(o)
        o['entropy'] = o['sum_lse'] - o['Nk_c'] - o['dots']
        return o
    ld = with_entropy(restate_pass(x, n, None, l1, l0, c, 0))
    f64 = with_entropy(restate_pass(x, n, None, l1, l0, c, 0, np.float64))
    tol, _ = tolerances(ld, f64, keys)
    # the entropy is a difference of three sums of the size of sum lse
    tol['entropy'] = max(tol['entropy'], 8 * 4 * float(np.spacing(abs(float(ld['sum_lse'])))))
    two = with_entropy(host_pass(N, D, K, 0, pk['xp'], pk['np'], None, None, l1, l0, c, True))
    one = with_entropy(host_pass(N, D, K, 1, pk['xp'], pk['np'], ncol, None, l1, l0, cf, True))
    for key in keys:
        for got in (two, one):
            assert error(got[key], ld[key]) <= tol[key], (key, error(got[key], ld[key]), tol[key])


def test_limits_chunks_and_workspace():
    from binm_host import binm_host
    from pmm_host import pmm_host
    lib, pmm = binm_host(), pmm_host()
    assert (lib.binm_max_k(), lib.binm_max_d(), lib.binm_max_trials()) == (64, 1024, 65534)
    assert lib.binm_dblock() == 64 == pmm.pmm_dblock(1)
    for N, D, K in ((0, 1, 1), (10 ** 6, 256, 32), (10 ** 9, 1024, 64), (257, 3, 2)):
        assert lib.binm_chunk_rows(N, D, K) == pmm.pmm_chunk_rows(N, D, K)
        assert lib.binm_workspace_doubles(N, D, K) == max(pmm.pmm_workspace_doubles(N, D, K), 3072)


def test_sanitized_stand_alone_program():
    """tests/host/binm_host_main.cpp under -fsanitize=address,undefined, never loaded into Python."""
    from binm_host import build_sanitized_program
    exe = build_sanitized_program()
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert out.stdout.count('flag=0') == 5 and 'runtime error' not in out.stdout
    assert out.stdout.count('one_plane=1') == 1


# -- the C ABI -----------------------------------------------------------------------------------------
ENTRY_POINTS = ('vmp_binm_limits', 'vmp_binm_plan', 'vmp_binm_pack', 'vmp_binm_tables',
                'vmp_binm_pass')


def test_cabi_declares_the_binm_entry_points_and_the_host_only_ones_answer():
    """Fails without the feature: the library has no such symbols."""
    from bayespy_amd import _lib
    from binm_host import binm_host
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    host = binm_host()
    v = [ctypes.c_int32() for _ in range(3)]
    assert lib.vmp_binm_limits(*[ctypes.byref(a) for a in v]) == _lib.VMP_OK
    assert tuple(a.value for a in v) == (host.binm_max_k(), host.binm_max_d(),
                                         host.binm_max_trials())
    assert lib.vmp_binm_limits(None, None, None) == _lib.VMP_ERR_INVALID
    c, w = ctypes.c_int64(), ctypes.c_int64()
    for N, D, K in ((0, 1, 1), (1000, 7, 5), (10 ** 6, 256, 32), (10 ** 6, 1024, 64)):
        assert lib.vmp_binm_plan(N, D, K, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_OK
        assert c.value == host.binm_chunk_rows(N, D, K)
        assert w.value == host.binm_workspace_doubles(N, D, K)
    for D, K in ((4, 65), (1025, 4)):
        assert lib.vmp_binm_plan(10, D, K, ctypes.byref(c), ctypes.byref(w)) \
            == _lib.VMP_ERR_UNSUPPORTED
        assert lib.vmp_binm_plan(10, D, K, None, None) == _lib.VMP_ERR_UNSUPPORTED   # shape first
    for N, D, K in ((-1, 4, 4), (4, 0, 4), (4, 4, 0)):
        assert lib.vmp_binm_plan(N, D, K, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_ERR_INVALID
    assert lib.vmp_binm_plan(10, 4, 4, None, None) == _lib.VMP_ERR_INVALID


def test_argument_rules_of_the_device_entry_points_without_a_context():
    """A null context is refused before anything else is looked at: VMP_ERR_INVALID, no launch."""
    from bayespy_amd import _lib
    lib = _lib.load()
    buf = np.zeros(16)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.vmp_binm_pack(None, 4, 4, 0, p, p, 0, 0, *[p] * 7) == _lib.VMP_ERR_INVALID
    assert lib.vmp_binm_tables(None, 4, 4, 0, *[p] * 7) == _lib.VMP_ERR_INVALID
    assert lib.vmp_binm_pass(None, 4, 4, 4, 0, *[p] * 14) == _lib.VMP_ERR_INVALID
    assert not buf.any()
