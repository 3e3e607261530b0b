"""GPU: stochastic variational inference on the two fused diagonal-Gaussian blocks -- the traces of
tests/golden/dgmm_svi.npz (live reference) through VB(..., engine='fused+batches+gaussian') with
host arrays and with device tensors as batches, and ``vmp_dgmm_natural_step`` alone through the C
ABI against the long-double restatement of tests/dgmm_svi_host.py."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ENGINE = 'fused+batches+gaussian'
TABLES = ('mu_par', 'mu_mom', 'tau_par', 'tau_mom')


def _mods(**kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB
    return dict(nodes=nodes, VB=VB, vb_kwargs=kw)


# -- the traces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('device_batches', [False, True])
@pytest.mark.parametrize('tag', ['par', 'value', 'mask'])
def test_golden_trace_on_the_device(tag, device_batches):
    import torch
    import dgmm_svi_models as M
    from dgmm_svi_host import PLAN
    from test_dgmm_svi_host import check_trace
    g = np.load(os.path.join(GOLDEN, 'dgmm_svi.npz'))

    def observe(Y, rows, mask):
        t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
        if mask is None:
            Y.observe(t)
        else:
            Y.observe(t, mask=torch.from_numpy(np.ascontiguousarray(mask)).cuda())
    res = M.run_case(_mods(engine=ENGINE), g, tag,
                     **(dict(observe=observe) if device_batches else {}))
    plan = res[tag + '_plan'].plans[0]
    assert type(plan).__name__ == PLAN[tag]
    assert check_trace(res, g, tag) == 6
    assert all(bool(torch.isfinite(getattr(plan, name)).all()) for name in TABLES)


# -- the step kernel through the C ABI ---------------------------------------------------------------
class _Step:
    def __init__(self):
        import torch
        from bayespy_amd.device import get_runtime
        from bayespy_amd.inference.plans.dgmm_masked import MaskedDGMMKernels
        self.torch, self.rt = torch, get_runtime()
        self.k = MaskedDGMMKernels(self.rt)

    def up(self, a):
        return None if a is None else \
            self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.rt.device)

    def run(self, D, K, nodes, x, mult, scale, per_element, stats=True, tables=None):
        """``x``: the dict of ``dgmm_svi_host.step_inputs``; ``tables``: replacements of the four
        tables.  dict of the four tables, alpha_r, elog_r and bound (3) as host arrays; what a node
        that is not named owns comes back as sent (elog_r and bound are sent as NaN)."""
        torch, rt, k = self.torch, self.rt, self.k
        t = dict({key: x[key] for key in TABLES}, **(tables or {}))
        d = {key: self.up(t[key]) for key in TABLES}
        pri = [self.up(x[key]) for key in ('m0', 'beta0', 'a0', 'b0')]
        st = [self.up(x[key]) if stats else None for key in ('S1', 'S2', 'cnt')]
        pr, nk, al = self.up(x['prior_r']), self.up(x['Nk']), self.up(x['alpha_r'])
        el = torch.full_like(pr, float('nan'))
        bound = torch.full((3,), float('nan'), dtype=torch.float64, device=rt.device)
        ws = rt.empty(k.natural_step_workspace(D, K))
        rt.sync_stream()
        k.natural_step(D, K, nodes, *pri, *st, per_element, d['mu_par'], d['mu_mom'], d['tau_par'],
                       d['tau_mom'], pr, nk if stats else None, al, el, mult, scale, ws, bound)
        rt.synchronize()
        out = {key: v.cpu().numpy() for key, v in d.items()}
        out.update(alpha_r=al.cpu().numpy(), elog_r=el.cpu().numpy(), bound=bound.cpu().numpy())
        return out


def _same(a, b):
    """Bit for bit, NaN included."""
    np.testing.assert_array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


@pytest.mark.parametrize('D,K', [(1, 1), (3, 2), (65, 5), (1024, 64)])
@pytest.mark.parametrize('per_element', [0, 1])
def test_step_against_long_double(D, K, per_element):
    """Every value of ``nodes`` at (mult, scale) = (1, 1), (400 / 70, 0.37) and (4, 1), with the rule
    of tests/test_dgmm_gpu.py: 8 times the deviation of the float64 evaluation of the reference's
    own form from long double, floor 4 ulp of the magnitude.  (65, 5) is 325 elements, more than
    one workgroup; (1024, 64) is the limit.  The inputs are made the way tests/test_mix_svi_gpu.py
    makes those of the Gamma table: statistics a pass could leave on a mini-batch of 70 rows."""
    from dgmm_svi_host import restate_step, step_inputs
    from dgmm_host import tolerances, error
    from test_mix_svi_gpu import _check_dirichlet
    st = _Step()
    x = step_inputs(D, K, per_element)
    nan = np.full((D * K, 2), np.nan)
    for mult, scale, stats in ((1.0, 1.0, True), (400 / 70, 0.37, True), (4.0, 1.0, True),
                               (2.5, 0.37, False)):
        args = [x[key] for key in ('m0', 'beta0', 'a0', 'b0')] \
            + [x[key] if stats else None for key in ('S1', 'S2', 'full')] + [x[key] for key in TABLES]
        ld = restate_step(*args, mult, scale)
        f64 = restate_step(*args, mult, scale, np.float64)
        keys = TABLES + ('mu_bound', 'tau_bound')
        tol, _ = tolerances(ld, f64, keys)
        for nodes in range(1, 8):
            # what a node that is not named owns is sent as NaN (its moments are an input)
            sent = dict(mu_par=x['mu_par'] if nodes & 1 else nan,
                        tau_par=x['tau_par'] if nodes & 2 else nan)
            got = st.run(D, K, nodes, x, mult, scale, per_element, stats, sent)
            got['mu_bound'], got['tau_bound'] = got['bound'][:2]
            for bit, name in ((1, 'mu'), (2, 'tau')):
                for key in (name + '_par', name + '_mom', name + '_bound'):
                    if nodes & bit:
                        err = error(got[key], ld[key])
                        print('D K = %d %d per_element %d mult %.3g scale %s nodes %d %s: error '
                              '%.3g allowed %.3g' % (D, K, per_element, mult, scale, nodes, key,
                                                     err, tol[key]))
                        assert err <= tol[key], (key, nodes, mult, scale, err, tol[key])
                    elif key.endswith('_bound'):
                        assert np.isnan(got[key]), (key, nodes)
                    else:
                        _same(got[key], nan if key.endswith('_par') else x[key])
            if nodes & 4:
                _check_dirichlet(got['alpha_r'][None], got['elog_r'][None], got['bound'][2],
                                 x['prior_r'][None], x['Nk'][None] if stats else None,
                                 x['alpha_r'][None], mult, scale, 'weights')
            else:
                _same(got['alpha_r'], x['alpha_r'])
                assert np.all(np.isnan(got['elog_r'])) and np.isnan(got['bound'][2])


@pytest.mark.parametrize('D,K', [(3, 2), (65, 5), (1024, 64)])
@pytest.mark.parametrize('per_element', [0, 1])
def test_step_bits(D, K, per_element):
    """mult = scale = 1 leaves the bits of vmp_dgmm_update / vmp_dgmm_update_masked (NaN in the old
    parameters: they are not read); the simultaneous step is each node's step from the entry state;
    two launches give the same bits."""
    from dgmm_svi_host import step_inputs
    st = _Step()
    x = step_inputs(D, K, per_element)
    nan = np.full((D * K, 2), np.nan)
    got = st.run(D, K, 7, x, 1.0, 1.0, per_element, True,
                 dict(mu_par=nan, tau_par=nan), )
    assert all(np.all(np.isfinite(got[key])) for key in TABLES + ('alpha_r', 'elog_r', 'bound'))
    up, rt = st.up, st.rt
    S1, S2, cnt = up(x['S1']), up(x['S2']), up(x['cnt'])
    for which, name, pa, pb, other in ((0, 'mu', 'm0', 'beta0', 'tau_mom'),
                                       (1, 'tau', 'a0', 'b0', 'mu_mom')):
        par, mom, out = rt.empty(D * K, 2), rt.empty(D * K, 2), rt.empty(1)
        rt.sync_stream()
        (st.k.update_masked if per_element else st.k.update)(
            D, K, which, up(x[pa]), up(x[pb]), S1, S2, cnt, up(x[other]), par, mom, out)
        rt.synchronize()
        _same(got[name + '_par'], par.cpu().numpy())
        _same(got[name + '_mom'], mom.cpu().numpy())
        _same(got['bound'][which], out.cpu().numpy()[0])
    both = st.run(D, K, 7, x, 2.5, 0.37, per_element)
    again = st.run(D, K, 7, x, 2.5, 0.37, per_element)
    for key in both:
        _same(both[key], again[key])
    for nodes, mine in ((1, ('mu_par', 'mu_mom')), (2, ('tau_par', 'tau_mom')),
                        (4, ('alpha_r', 'elog_r'))):
        one = st.run(D, K, nodes, x, 2.5, 0.37, per_element)
        for key in mine:
            _same(one[key], both[key])
        slot = nodes.bit_length() - 1
        _same(one['bound'][slot], both['bound'][slot])


def test_status_codes_leave_the_outputs_untouched():
    from bayespy_amd import _lib
    from bayespy_amd.device import get_runtime
    rt = get_runtime()
    lib, ctx = rt.lib, rt.ctx
    z = rt.zeros(4096)
    z.fill_(1.5)
    out = rt.empty(3)
    out.fill_(float('nan'))
    p, o = ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(out.data_ptr())
    step = lib.vmp_dgmm_natural_step
    nan = float('nan')
    rt.sync_stream()

    def call(ctx_=ctx, D=4, K=2, nodes=7, m0=p, beta0=p, a0=p, b0=p, S1=p, S2=p, cnt=p, per=0,
             mu_par=p, mu_mom=p, tau_par=p, tau_mom=p, prior_r=p, Nk=p, alpha_r=p, elog_r=p,
             mult=2.0, scale=0.5, ws=p, bound=o):
        return step(ctx_, D, K, nodes, m0, beta0, a0, b0, S1, S2, cnt, per, mu_par, mu_mom, tau_par,
                    tau_mom, prior_r, Nk, alpha_r, elog_r, mult, scale, ws, bound)
    bad = [dict(ctx_=None), dict(D=0), dict(K=0), dict(D=-1), dict(nodes=0), dict(nodes=8),
           dict(per=2), dict(per=-1), dict(mult=0.0), dict(mult=-2.0), dict(mult=nan),
           dict(scale=nan), dict(ws=None), dict(bound=None), dict(m0=None), dict(beta0=None),
           dict(a0=None), dict(b0=None), dict(mu_par=None), dict(mu_mom=None), dict(tau_par=None),
           dict(tau_mom=None), dict(prior_r=None), dict(alpha_r=None), dict(elog_r=None),
           dict(S1=None), dict(S2=None), dict(cnt=None), dict(S1=None, S2=None)]
    for kw in bad:
        assert call(**kw) == _lib.VMP_ERR_INVALID, kw
    for kw in (dict(K=65), dict(D=1025), dict(D=1025, m0=None)):     # the limits come before the pointers
        assert call(**kw) == _lib.VMP_ERR_UNSUPPORTED, kw
    rt.synchronize()
    assert bool((z == 1.5).all()) and bool(out.isnan().all())
    # what a node that is not named would need may be null
    assert call(nodes=4, m0=None, beta0=None, a0=None, b0=None, S1=None, mu_par=None, mu_mom=None,
                tau_par=None, tau_mom=None) == _lib.VMP_OK
    rt.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[0]) and np.isnan(got[1]) and np.isfinite(got[2])
    out.fill_(float('nan'))
    z.fill_(1.5)
    t = [rt.zeros(8, 2) for _ in range(4)]
    for a in t:
        a.fill_(2.0)
    q = [ctypes.c_void_p(a.data_ptr()) for a in t]
    rt.sync_stream()
    assert call(nodes=1, a0=None, b0=None, prior_r=None, alpha_r=None, elog_r=None, S1=None,
                S2=None, cnt=None, mu_par=q[0], mu_mom=q[1], tau_par=q[2], tau_mom=q[3]) == _lib.VMP_OK
    rt.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got[0]) and np.isnan(got[1]) and np.isnan(got[2])
    # phi* is the prior (1.5, 1.5): lambda = 2 + 0.5 (1.5 - 2), lambda m = 4 + 0.5 (2.25 - 4)
    np.testing.assert_allclose(t[0].cpu().numpy(), np.tile([3.125 / 1.75, 1.75], (8, 1)), rtol=1e-15)
    assert bool((t[2] == 2.0).all()) and bool((t[3] == 2.0).all())
