"""GPU: deterministic annealing (``VB.set_annealing``) on the fused full-covariance Gaussian-mixture
block -- the scripts of tests/anneal_models.py against the live-reference fixtures
(tests/golden/anneal.npz, tools/make_golden_anneal.py) at the tolerances of tests/test_gmm_gpu.py,
the annealed entry points at a coefficient of 1 against the plain ones bit for bit, the annealed
Wishart that is none, and the fused plans that decline."""
import os

import numpy as np
import pytest

import anneal_models

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'anneal.npz')


def _mods(**vb_kwargs):
    import bayespy_amd.nodes
    from bayespy_amd.inference import VB
    return dict(nodes=bayespy_amd.nodes, VB=VB, vb_kwargs=vb_kwargs)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


def _inputs(golden):
    return {k[3:]: golden[k] for k in golden.files if k.startswith('in_')}


def _compare(res, ref, tag, pre=''):
    """The tolerances tests/test_gmm_gpu.py applies to the same quantities."""
    np.testing.assert_allclose(res[tag + '_L'], ref[tag + '_L'], rtol=1e-9)
    for nm in anneal_models.NODES:
        k = '%s_%s_Lterm' % (tag, nm)
        np.testing.assert_allclose(res[k], ref[k], rtol=1e-9, atol=1e-4, err_msg=k)
    np.testing.assert_allclose(res[tag + '_z_u0'], ref[tag + '_z_u0'], rtol=1e-7, atol=1e-12)
    np.testing.assert_allclose(res[tag + '_mu_u0'], ref[tag + '_mu_u0'], rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(res[tag + '_mu_u1'], ref[tag + '_mu_u1'], rtol=1e-7, atol=1e-10)
    lam = ref[tag + '_Lambda_u0']
    np.testing.assert_allclose(res[tag + '_Lambda_u0'], lam, rtol=1e-7,
                               atol=1e-10 + 1e-11 * np.abs(lam).max())
    np.testing.assert_allclose(res[tag + '_Lambda_u1'], ref[tag + '_Lambda_u1'], rtol=1e-9)
    np.testing.assert_allclose(res[tag + '_alpha_u0'], ref[tag + '_alpha_u0'], rtol=1e-9)


@pytest.mark.parametrize('tag', anneal_models.CASES)
def test_annealed_block_vs_reference(golden, tag):
    res = anneal_models.run_cases(_mods(), _inputs(golden), only=(tag,))
    assert type(res[tag + '_plan'].plans[0]).__name__ == 'GMMPlan'
    _compare(res, golden, tag)
    if tag == 'two':
        # the bound at 0.5 of the q the schedule left, no update in between: the temperature of
        # a term is the node's at the request, and the cached terms of 1.0 are not returned
        np.testing.assert_allclose(res['two_after_L'], golden['two_after_L'], rtol=1e-9)
        assert abs(res['two_after_L'] - res['two_L'][-1]) > 1.0
        for nm in anneal_models.NODES:
            k = 'two_after_%s_Lterm' % nm
            np.testing.assert_allclose(res[k], golden[k], rtol=1e-9, atol=1e-4, err_msg=k)


def test_annealed_block_vs_generic_engine(golden):
    g = _inputs(golden)
    res = anneal_models.run_cases(_mods(), g, only=('one',))
    gen = anneal_models.run_cases(_mods(engine='generic'), g, only=('one',))
    assert type(gen['one_plan'].plans[0]).__name__ == 'GenericPlan'
    _compare(res, gen, 'one')


@pytest.mark.parametrize('D,K', [(2, 3), (17, 33)])
def test_annealed_entry_points_at_one_are_the_plain_ones_bit_for_bit(golden, D, K):
    """On copies of one state block: every annealed entry point with a coefficient (a temperature)
    of 1.0 and the entry point it stands beside leave the same bits in the WHOLE state."""
    import torch
    from bayespy_amd.inference.plans.gmm import STEP_MU, STEP_LAMBDA, STEP_ALPHA
    tag = 'one' if D == 2 else 'three'
    g = _inputs(golden)
    Q, m = anneal_models.build(_mods(), g[tag + '_y'], K, anneal_models.N0[tag],
                               z0=g[tag + '_z0'])
    Q.update(repeat=1, verbose=False)
    plan = Q.plans[0]
    k, rt = plan.kernels, plan.rt
    a, b = plan.state.clone(), plan.state.clone()
    steps = [
        ('update_mu', lambda s: k.update_mu(D, K, s),
         lambda s: k.update_annealed(D, K, STEP_MU, 1.0, s)),
        ('update_lambda', lambda s: k.update_lambda(D, K, s),
         lambda s: k.update_annealed(D, K, STEP_LAMBDA, 1.0, s)),
        ('update_alpha', lambda s: k.update_alpha(D, K, s),
         lambda s: k.update_annealed(D, K, STEP_ALPHA, 1.0, s)),
        ('prepare_z', lambda s: k.prepare_z(D, K, False, s),
         lambda s: k.prepare_z_annealed(D, K, False, 1.0, s)),
        ('lower_bound', lambda s: k.lower_bound(D, K, s),
         lambda s: k.lower_bound_annealed(D, K, (1.0, 1.0, 1.0, 1.0), s)),
        ('prepare_z from the prior', lambda s: k.prepare_z(D, K, True, s),
         lambda s: k.prepare_z_annealed(D, K, True, 0.5, s)),
    ]
    for name, plain, annealed in steps:
        before = a.clone()
        plain(a)
        annealed(b)
        rt.sync_stream()
        torch.cuda.synchronize()
        # (alpha was the last node of the iteration above and the statistics have not moved since:
        # its update writes the values that are there)
        assert name == 'update_alpha' or not torch.equal(a, before), name + ' wrote nothing'
        assert torch.equal(a, b), name
    # and a temperature that is not 1 moves every q term, the Y term not at all
    L = plan.layout
    k.lower_bound_annealed(D, K, (2.0, 2.0, 2.0, 2.0), b)
    torch.cuda.synchronize()
    ta = a[L.off_L:L.off_L + 5].cpu().numpy()
    tb = b[L.off_L:L.off_L + 5].cpu().numpy()
    assert ta[0] == tb[0] and np.all(ta[1:] != tb[1:])


def test_annealed_wishart_below_its_degrees_raises():
    """D = 3, n0 = 3, coefficient 0.1: 0.1 (n0 + R_k) <= D - 1 for a cluster that holds few rows.
    The reference goes on with NaN; the block raises at the bound request."""
    from bayespy_amd.nodes import (GaussianARD, Gaussian, Wishart, Dirichlet, Categorical,
                                   Mixture)
    from bayespy_amd.inference import VB
    rs = np.random.RandomState(5)
    N, D, K = 40, 3, 4
    y = rs.normal(size=(N, D))
    alpha = Dirichlet(np.ones(K), name='alpha')
    z = Categorical(alpha, plates=(N,), name='z')
    mu = GaussianARD(0, 1e-2, shape=(D,), plates=(K,), name='mu')
    Lam = Wishart(3, np.identity(D), plates=(K,), name='Lambda')
    Y = Mixture(z, Gaussian, mu, Lam, plates=(N,), name='Y')
    z.initialize_from_value(rs.randint(K, size=N))
    Y.observe(y)
    Q = VB(Y, mu, Lam, z, alpha)
    Q.ignore_bound_checks = True
    assert type(Q.plans[0]).__name__ == 'GMMPlan'
    Q.set_annealing(0.1)
    with pytest.raises(ValueError, match='degrees of freedom'):
        Q.update(repeat=1, verbose=False)


def test_other_fused_plans_still_decline():
    from bayespy_amd.nodes import GaussianARD, Gaussian, Dirichlet, Categorical, Mixture
    from bayespy_amd.inference import VB
    from dgmm_masked_models import build_dgmm_masked
    rs = np.random.RandomState(6)
    N, D, K = 30, 4, 3
    y = rs.normal(size=(N, D))
    m = build_dgmm_masked(_mods(), N, D, K, y, rs.rand(N, D) < 0.8)
    Q = VB(m['Y'], m['Z'], m['mu'], m['tau'], m['alpha'], engine='fused')
    assert type(Q.plans[0]).__name__ == 'MaskedDiagGaussianMixturePlan'
    with pytest.raises(NotImplementedError, match='annealing is not built into the fused'):
        Q.set_annealing(0.5)
    Q.set_annealing(1.0)

    NB = 10
    mu = GaussianARD(0, 0.001, shape=(D,), plates=(K,), name='means')
    alpha = Dirichlet(np.ones(K), name='class probabilities')
    Z = Categorical(alpha, plates=(NB,), plates_multiplier=(N / NB,), name='classes')
    Y = Mixture(Z, Gaussian, mu, np.identity(D), name='observations')
    mu.initialize_from_value(rs.normal(size=(K, D)))
    Q = VB(Y, Z, mu, alpha, engine='fused')
    assert type(Q.plans[0]).__name__ == 'GMMSVIPlan'
    with pytest.raises(NotImplementedError, match='annealing is not built into the fused'):
        Q.set_annealing(0.5)
    Q.set_annealing(1.0)


# ---- the diagonal block (engine='fused') ----------------------------------------------------------------

@pytest.mark.parametrize('tag', anneal_models.DIAG_CASES)
def test_annealed_diag_block_vs_reference(golden, tag):
    from test_anneal_host import check_diag
    res = anneal_models.run_diag_cases(_mods(engine='fused'), _inputs(golden), only=(tag,))
    assert type(res[tag + '_plan'].plans[0]).__name__ == 'DiagGaussianMixturePlan'
    check_diag(res, golden, tag)


@pytest.mark.parametrize('D,K', [(5, 3), (70, 17)])
def test_annealed_diag_entry_points_at_one_are_the_plain_ones_bit_for_bit(D, K):
    """vmp_dgmm_tables_annealed and vmp_dgmm_update_annealed with a coefficient of 1.0 against
    vmp_dgmm_tables and vmp_dgmm_update: the same bits in h, q, c, gsum, par and mom; A - B is the
    plain bound term up to the rounding of its other form."""
    import torch
    from dgmm_host import make_inputs, host_tables, host_pass
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference.plans.dgmm import DGMMKernels
    rt = get_runtime()
    rt.sync_stream()
    k = DGMMKernels(rt)
    g = make_inputs(300, D, K)
    up = lambda a: rt.torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(rt.device)  # noqa: E731
    mu_mom, tau_mom, elog = up(g['mu_mom']), up(g['tau_mom']), up(g['elog_pi'])
    outs = []
    for annealed in (False, True):
        h, q, c, gs = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K), rt.zeros(K)
        if annealed:
            k.tables_annealed(D, K, 1.0, mu_mom, tau_mom, elog, h, q, c, gs)
        else:
            k.tables(D, K, mu_mom, tau_mom, elog, h, q, c, gs)
        outs.append((h, q, c, gs))
    rt.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    hh, hq, hc, _ = host_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])
    st = host_pass(300, D, K, g['y'], None, hh, hq, hc)
    S1, S2, Nk = up(st['S1']), up(st['S2']), up(st['Nk'])
    for which, pa, pb, other in ((0, 'm0', 'beta0', tau_mom), (1, 'a0', 'b0', mu_mom)):
        prior_a, prior_b = up(g[pa]), up(g[pb])
        par0, mom0, bound = rt.zeros(D * K, 2), rt.zeros(D * K, 2), rt.zeros(1)
        par1, mom1, ab = rt.zeros(D * K, 2), rt.zeros(D * K, 2), rt.zeros(2)
        k.update(D, K, which, prior_a, prior_b, S1, S2, Nk, other, par0, mom0, bound)
        k.update_annealed(D, K, which, 1.0, prior_a, prior_b, S1, S2, Nk, other, par1, mom1, ab)
        rt.synchronize()
        assert torch.equal(par0, par1) and torch.equal(mom0, mom1)
        A, B = ab.cpu().numpy()
        np.testing.assert_allclose(A - B, float(bound.cpu().numpy()[0]), rtol=1e-9, atol=1e-9)
        # the parts alone of the same q
        ab2 = rt.zeros(2)
        k.update_annealed(D, K, which + 2, 1.0, prior_a, prior_b, None, None, None, None, par1, mom1,
                          ab2)
        rt.synchronize()
        assert torch.equal(ab, ab2)
