"""GPU: the maximum-likelihood nodes GammaShape / Concentration (csrc/vmp_ml.hip) -- the C ABI
kernels against NumPy restatements of the reference, the models of tests/ml_models.py against the
live-reference fixtures (tests/golden/ml_nodes.npz), eager against recorded sweeps, save / load, and
the error flags.  Tolerances as in test_generic_engine_gpu.py: ELBO rtol 1e-9, moments 1e-7."""
import ctypes
import os
import warnings

import numpy as np
import pytest

from ml_host import concentration_fixed_point, invpsi

pytestmark = pytest.mark.gpu

ELBO_RTOL = 1e-9
MOM_RTOL = 1e-7


def _rt():
    from bayespy_amd.device import get_runtime
    return get_runtime()


def _vp(t):
    return ctypes.c_void_p(t.data_ptr())


def _dev(a):
    rt = _rt()
    return rt.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(rt.device)


def test_invpsi_kernel_matches_the_reference_recipe():
    from bayespy_amd.utils import misc
    x = np.concatenate([np.linspace(-30, 12, 4001), [-2.22, 0.0, np.nan]])
    y = misc.invpsi(x).numpy()
    r = invpsi(x)
    ok = ~np.isnan(r)
    np.testing.assert_allclose(y[ok], r[ok], rtol=1e-12, atol=1e-300)
    assert np.isnan(y[-1])


def test_gamma_shape_kernel():
    rt = _rt()
    rs = np.random.RandomState(3)
    n = 5000
    m0, m1 = -rs.rand(n) * 50, -rs.rand(n) * 30 - 1
    r0, r1 = rs.rand(n) - 0.5, np.full(n, 0.5)
    ins = [_dev(v) for v in (m0, m1, r0, r1)]
    a, lga = _dev(np.zeros(n)), _dev(np.zeros(n))
    rt.sync_stream()
    rt.check(rt.lib.vmp_ml_gamma_shape(rt.ctx, n, *[_vp(t) for t in ins], _vp(a), _vp(lga)))
    from scipy import special
    ar = invpsi(-(m0 + r0) / (m1 + r1))
    np.testing.assert_allclose(a.cpu().numpy(), ar, rtol=1e-12)
    np.testing.assert_allclose(lga.cpu().numpy(), special.gammaln(ar), rtol=1e-12, atol=1e-13)


@pytest.mark.parametrize('rows', [1, 7, 4096])
def test_concentration_kernel_matches_the_reference(rows):
    rt = _rt()
    rs = np.random.RandomState(rows)
    K = 4
    n = rs.randint(5, 60, size=rows).astype(np.float64)
    conc = rs.gamma(2.0, 1.0, size=(rows, K))
    m0 = np.stack([np.log(rs.dirichlet(conc[i], size=int(n[i]))).sum(0) for i in range(rows)])
    r0, r1 = np.full((rows, K), np.log(1 / K)), np.ones(rows)
    ar, it, capped = concentration_fixed_point(m0, n, r0, r1)
    assert not capped
    ins = [_dev(v) for v in (m0, n, r0, r1)]
    alpha, work, z = _dev(np.zeros((rows, K))), _dev(np.zeros((rows, K))), _dev(np.zeros(rows))
    st = rt.torch.full((3,), -1, dtype=rt.torch.int32, device=rt.device)
    rt.sync_stream()
    rt.check(rt.lib.vmp_ml_concentration(rt.ctx, rows, K, *[_vp(t) for t in ins], 1000000,
                                         _vp(alpha), _vp(work), _vp(z), _vp(st)))
    st = st.cpu().numpy()
    assert list(st[:2]) == [0, 0]
    assert st[2] == it                        # the global stopping rule, iteration for iteration
    np.testing.assert_allclose(alpha.cpu().numpy(), ar, rtol=1e-10)
    from scipy import special
    np.testing.assert_allclose(z.cpu().numpy(),
                               special.gammaln(ar.sum(-1)) - special.gammaln(ar).sum(-1),
                               rtol=1e-9, atol=1e-9)


def _golden(golden_dir):
    f = np.load(os.path.join(golden_dir, 'ml_nodes.npz'))
    return f, {k[3:]: f[k] for k in f.files if k.startswith('in_')}


@pytest.mark.parametrize('tag', ['gs', 'gp', 'cc', 'cn', 'cu', 'cp', 'bc', 'gm'])
def test_models_match_reference(golden_dir, tag):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    from ml_models import run_ml_cases
    f, g = _golden(golden_dir)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        res = run_ml_cases(N_, VB, g, only=[tag])
    if tag == 'gm':
        # the Gaussian mixture runs on the generic engine and is told why
        assert any('concentration of the assignment prior is a node' in str(x.message) for x in w)
    np.testing.assert_allclose(res[tag + '_L'], f[tag + '_L'], rtol=ELBO_RTOL)
    for k, v in res.items():
        if isinstance(v, list):
            for i, vi in enumerate(v):
                np.testing.assert_allclose(vi, f['%s_%d' % (k, i)], rtol=MOM_RTOL, atol=1e-12)


def _demo(g):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    a = N_.GammaShape(name='a')
    b = N_.Gamma(1e-5, 1e-5, name='b')
    tau = N_.Gamma(a, b, plates=(1000,), name='tau')
    tau.observe(g['gs_tau'])
    Q = VB(tau, a, b)
    return Q, ['a', 'b']


def _plates(g):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    c = N_.Concentration(5, plates=(3, 1, 1), name='c')
    p = N_.Dirichlet(c, plates=(3, 12, 1), name='p')
    z = N_.Categorical(p, plates=(3, 12, 80), name='z')
    z.observe(g['cp_z'])
    Q = VB(z, p, c)
    return Q, ['c', 'p']


@pytest.mark.parametrize('build', [_demo, _plates])
def test_eager_and_recorded_sweeps_are_bit_identical(golden_dir, monkeypatch, build):
    """The fixed point runs inside the kernel: the sweep is recordable (no host read), and a replay
    is the eager sweep launch for launch."""
    _, g = _golden(golden_dir)

    def run():
        Q, track = build(g)
        Q.ignore_bound_checks = True
        Q.update(repeat=8, verbose=False)
        info = Q[track[0]]._plan.graph_info()
        return [Q.L[:8].copy()] + [np.array(u) for nm in track for u in Q[nm].u], info
    monkeypatch.setenv('BAYESPY_AMD_GRAPH', '0')
    eager, _ = run()
    monkeypatch.setenv('BAYESPY_AMD_GRAPH', '1')
    graph, info = run()
    assert info['recorded'] and info['disabled'] is None, info
    assert info['replays'] >= 3, info
    for a, b in zip(eager, graph):
        assert np.array_equal(a, b)


def test_save_load_round_trip(golden_dir, tmp_path):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    _, g = _golden(golden_dir)

    def build():
        a = N_.GammaShape(name='a')
        b = N_.Gamma(1e-5, 1e-5, name='b')
        tau = N_.Gamma(a, b, plates=(1000,), name='tau')
        tau.observe(g['gs_tau'])
        c = N_.Concentration(4, name='c')
        p = N_.Dirichlet(c, plates=(30, 1), name='p')
        z = N_.Categorical(p, plates=(30, 200), name='z')
        z.observe(g['cc_z'])
        Q = VB(tau, a, b, z, p, c)
        Q.ignore_bound_checks = True
        return Q
    Q = build()
    Q.update(repeat=2, verbose=False)
    fn = str(tmp_path / 'ml.bin')
    Q.save(filename=fn)
    Q.update(repeat=3, verbose=False)
    Q2 = build()
    Q2.load(filename=fn)
    Q2.update(repeat=3, verbose=False)
    assert np.array_equal(Q2.L[:5], Q.L[:5])
    for nm in ('a', 'b', 'c', 'p'):
        for x, y in zip(Q2[nm].u, Q[nm].u):
            np.testing.assert_array_equal(x, y)


def test_errors_raise_without_a_fault(monkeypatch):
    import bayespy_amd.nodes as N_
    from bayespy_amd.inference import VB
    from bayespy_amd.inference.plans.families.ml import ConcentrationFamily
    # a numerically zero probability in the child: the reference's ValueError
    c = N_.Concentration(3, name='c')
    p = N_.Dirichlet(c, plates=(2,), name='p')
    p.observe(np.array([[0.5, 0.5, 0.0], [0.2, 0.3, 0.5]]))
    VB(p, c)
    with pytest.raises(ValueError, match='infs'):
        c.update()
    # the iteration cap
    monkeypatch.setattr(ConcentrationFamily, 'max_iter', 3)
    c = N_.Concentration(3, name='c')
    p = N_.Dirichlet(c, plates=(2,), name='p')
    p.observe(np.array([[0.1, 0.6, 0.3], [0.2, 0.3, 0.5]]))
    VB(p, c)
    with pytest.raises(RuntimeError, match='did not converge in 3 iterations'):
        c.update()
    st = c._plan.family[id(c)].status.cpu().numpy()
    assert list(st) == [0, 1, 3]
    # the device is fine afterwards
    monkeypatch.setattr(ConcentrationFamily, 'max_iter', 1000000)
    c.update()
    assert np.all(np.isfinite(c.u[0]))
