"""CPU: deterministic annealing on the fused Gaussian-mixture plan -- the gate of
``VB.set_annealing``, the plan's choice between the plain and the annealed kernel forms, its bound
cache, and the annealed formulas themselves (restated in NumPy on the kernel double below) against
the live-reference fixtures of tools/make_golden_anneal.py."""
import os

import numpy as np
import pytest
from scipy import special

import anneal_models
from fake_kernels import CPUGMMKernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'anneal.npz')


class AnnealedCPUGMMKernels(CPUGMMKernels):
    """TEST DOUBLE: CPUGMMKernels + the annealed forms of ``GMMKernels`` (vmp_gmm_*_annealed), the
    formulas of include/vmp_hip.h in NumPy."""

    _z_annealing = 1.0

    def prepare_z(self, D, K, prior_only, state):
        super().prepare_z(D, K, prior_only, state)
        self._z_annealing = 1.0

    def prepare_z_annealed(self, D, K, prior_only, annealing, state):
        self.calls.append('prepare_z_annealed')
        self._prior_only = bool(prior_only)
        self._z_annealing = 1.0 if prior_only else annealing

    def pass_(self, Y, N, D, K, R, state, ws):
        b = self._z_annealing
        if b == 1.0:
            return super().pass_(Y, N, D, K, R, state, ws)
        self.calls.append('pass')
        v = self._v(state, D, K)
        y = Y.numpy()[:N, :D]
        c, bb = self._coefficients(v, D)
        phi = b * ((v['logpi'] + c)[None, :] + y @ bb.T
                   - 0.5 * np.einsum('ni,kij,nj->nk', y, v['Lam'], y))
        lse = special.logsumexp(phi, axis=1, keepdims=True)
        p = np.exp(phi - lse)
        p /= p.sum(axis=1, keepdims=True)
        R.numpy()[:N, :K] = p
        self._set_stats(v, p, y)
        v['zs'][0] = float(lse.sum())
        v['zs'][1] = float((p * phi).sum())

    def update_annealed(self, D, K, node, annealing, state):
        self.calls.append('update_annealed_%d' % node)
        v = self._v(state, D, K)
        b = annealing
        if node == 1:
            Lmu = b * (v['hdr'][0] * np.eye(D) + v['R'][:, None, None] * v['Lam'])
            v['Cmu'][:] = np.linalg.inv(Lmu)
            v['ldLmu'][:] = np.linalg.slogdet(Lmu)[1]
            v['mu'][:] = np.einsum('kij,kj->ki', v['Cmu'],
                                   b * np.einsum('kij,kj->ki', v['Lam'], v['S1']))
        elif node == 2:
            mm = v['Cmu'] + v['mu'][:, :, None] * v['mu'][:, None, :]
            sm = v['S1'][:, :, None] * v['mu'][:, None, :]
            v['nk'][:] = b * (v['hdr'][1] + v['R'])
            v['Vk'][:] = b * (v['V0'] + v['S2'] - sm - np.swapaxes(sm, 1, 2)
                              + v['R'][:, None, None] * mm)
            self._lambda_moments(v, D)
        else:
            v['alpha'][:] = b * (v['alpha0'] + v['R'])
            v['logpi'][:] = special.digamma(v['alpha']) - special.digamma(v['alpha'].sum())

    def lower_bound_annealed(self, D, K, temperatures, state):
        self.calls.append('lower_bound_annealed')
        Tz, Ta, Tm, TL = temperatures
        v = self._v(state, D, K)
        c, b = self._coefficients(v, D)
        beta0, n0, ldV0 = v['hdr'][0], v['hdr'][1], v['hdr'][2]
        L_Y = float(np.sum(v['R'] * c) + np.sum(b * v['S1'])
                    - 0.5 * np.einsum('kij,kij->', v['Lam'], v['S2']))
        L_z = float(Tz * (v['zs'][0] - v['zs'][1]) + np.sum(v['R'] * v['logpi']))
        a0, a = v['alpha0'], v['alpha']
        L_pi = float(special.gammaln(a0.sum()) - special.gammaln(a0).sum() + np.sum(a0 * v['logpi'])
                     - Ta * (special.gammaln(a.sum()) - special.gammaln(a).sum()
                             + np.sum(a * v['logpi'])))
        mm = v['Cmu'] + v['mu'][:, :, None] * v['mu'][:, None, :]
        L_mu = float(np.sum(-0.5 * beta0 * np.einsum('kii->k', mm) + 0.5 * D * np.log(beta0)
                            - Tm * (0.5 * v['ldLmu'] - 0.5 * D)))
        g_p = 0.5 * n0 * ldV0 - 0.5 * D * n0 * np.log(2.0) - self._multigammaln(0.5 * n0, D)
        g_q = 0.5 * v['nk'] * v['ldV'] - 0.5 * D * v['nk'] * np.log(2.0) \
            - self._multigammaln(0.5 * v['nk'], D)
        A = g_p - 0.5 * np.einsum('ij,kij->k', v['V0'], v['Lam']) + 0.5 * n0 * v['ldLam']
        B = g_q - 0.5 * np.einsum('kij,kij->k', v['Vk'], v['Lam']) + 0.5 * v['nk'] * v['ldLam']
        L_Lam = float(np.sum(A - TL * B))
        v['Lout'][:6] = [L_Y, L_z, L_pi, L_mu, L_Lam, L_Y + L_z + L_pi + L_mu + L_Lam]
        v['scal'][3] = 0.0


def _mods():
    import bayespy_amd.nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.device import Runtime

    class HostVB(VB):
        def __init__(self, *nodes, **kw):
            super().__init__(*nodes, **kw)
            plan = self.plans[0]
            assert type(plan).__name__ == 'GMMPlan'
            rt = Runtime(device='cpu')
            plan._rt, plan._kernels = rt, AnnealedCPUGMMKernels(rt)

    return dict(nodes=bayespy_amd.nodes, VB=HostVB)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize('tag', anneal_models.CASES)
def test_plan_reproduces_annealed_reference_trace(golden, tag):
    """The plan reads node.annealing at every update and at every bound request; with the NumPy
    restatement of the annealed kernels it reproduces the reference's bound, every node's term and
    the final moments (the tolerances of tests/test_gmm_plan_host.py)."""
    g = {k[3:]: golden[k] for k in golden.files if k.startswith('in_')}
    res = anneal_models.run_cases(_mods(), g, only=(tag,))
    keys = [k for k in res if not k.endswith('_plan')]
    assert keys
    for k in keys:
        if k.endswith('_L'):
            np.testing.assert_allclose(res[k], golden[k], rtol=1e-10, err_msg=k)
        elif k.endswith('_Lterm'):
            np.testing.assert_allclose(res[k], golden[k], rtol=1e-8, atol=1e-7, err_msg=k)
        elif k.endswith('Lambda_u1') or k.endswith('alpha_u0'):
            np.testing.assert_allclose(res[k], golden[k], rtol=1e-10, err_msg=k)
        else:
            np.testing.assert_allclose(res[k], golden[k], rtol=1e-8, atol=1e-10, err_msg=k)


def _small(golden):
    g = {k[3:]: golden[k] for k in golden.files if k.startswith('in_')}
    Q, m = anneal_models.build(_mods(), g['one_y'], 3, anneal_models.N0['one'], z0=g['one_z0'])
    return Q, m


def test_plain_kernels_at_one_annealed_forms_otherwise(golden):
    Q, m = _small(golden)
    Q.update(repeat=1, verbose=False)
    calls = Q.plans[0].kernels.calls
    assert calls[2:] == ['update_mu', 'update_lambda', 'prepare_z', 'pass', 'update_alpha',
                         'lower_bound']
    n = len(calls)
    Q.set_annealing(0.5)
    Q.update(repeat=1, verbose=False)
    assert calls[n:] == ['update_annealed_1', 'update_annealed_2', 'prepare_z_annealed', 'pass',
                         'update_annealed_4', 'lower_bound_annealed']
    # a single node, as in the reference: only its update and its temperature change
    n = len(calls)
    Q.set_annealing(1.0)
    m['mu'].annealing = 0.25
    Q.update(repeat=1, verbose=False)
    assert calls[n:] == ['update_annealed_1', 'update_lambda', 'prepare_z', 'pass', 'update_alpha',
                         'lower_bound_annealed']


def test_bound_cache_includes_the_coefficients(golden):
    """After set_annealing with no update the terms are formed again -- the state did not change,
    the temperatures did -- and asking twice at the same coefficients launches nothing."""
    Q, m = _small(golden)
    Q.update(repeat=2, verbose=False)
    calls = Q.plans[0].kernels.calls
    n = len(calls)
    L1 = Q.compute_lowerbound()
    assert len(calls) == n
    Q.set_annealing(0.5)
    L2 = Q.compute_lowerbound()
    assert calls[n:] == ['lower_bound_annealed'] and L2 != L1
    Q.compute_lowerbound()
    assert calls[n:] == ['lower_bound_annealed']
    Q.set_annealing(1.0)
    assert Q.compute_lowerbound() == L1 and calls[n:] == ['lower_bound_annealed', 'lower_bound']


class _Node:
    def __init__(self, plan):
        self._plan, self.annealing, self.name = plan, 1.0, 'x'


def test_set_annealing_gate():
    """``VB.set_annealing`` takes nodes whose plan declares ANNEALING = True and declines any other
    fused plan; 1.0 is always allowed."""
    from bayespy_amd.inference import VB

    class Takes:
        ANNEALING = True

    class Declines:
        pass

    class DeclinesByFlag:
        ANNEALING = False

    Q = VB.__new__(VB)
    Q.model = [_Node(Takes()), _Node(Takes())]
    Q.set_annealing(0.5)
    assert [n.annealing for n in Q.model] == [0.5, 0.5] and Q.annealing_changed
    for plan in (Declines(), DeclinesByFlag()):
        Q.model = [_Node(Takes()), _Node(plan)]
        with pytest.raises(NotImplementedError, match='annealing is not built into the fused'):
            Q.set_annealing(0.5)
        assert [n.annealing for n in Q.model] == [1.0, 1.0]      # nothing half set
        Q.set_annealing(1.0)
    with pytest.raises(ValueError):
        Q.set_annealing(0.0)


def test_which_plans_declare_annealing():
    from bayespy_amd.inference.plans.gmm import GMMPlan, GMMSVIPlan
    from bayespy_amd.inference.plans.dgmm import DiagGaussianMixturePlan
    from bayespy_amd.inference.plans.dgmm_masked import MaskedDiagGaussianMixturePlan
    assert GMMPlan.ANNEALING is True
    assert not GMMSVIPlan.ANNEALING
    assert DiagGaussianMixturePlan.ANNEALING is True
    assert not getattr(MaskedDiagGaussianMixturePlan, 'ANNEALING', False)


# ---- the diagonal block ------------------------------------------------------------------------------

def _diag_mods():
    import bayespy_amd.nodes
    from bayespy_amd.inference import VB
    from bayespy_amd.device import Runtime
    from anneal_host import AnnealedCPUDGMMKernels

    class HostVB(VB):
        def __init__(self, *nodes, **kw):
            super().__init__(*nodes, engine='fused', **kw)
            plan = self.plans[0]
            assert type(plan).__name__ == 'DiagGaussianMixturePlan'
            rt = Runtime(device='cpu')
            plan._rt, plan._kernels = rt, AnnealedCPUDGMMKernels(rt)

    return dict(nodes=bayespy_amd.nodes, VB=HostVB)


def check_diag(res, golden, tag):
    """The tolerances of the fixture tests of the block (tests/test_dgmm_host.py check_fixture)."""
    from test_dgmm_host import L_RTOL, MOM_TOL
    checked = 0
    for k, v in res.items():
        if k.endswith('_plan'):
            continue
        if k.endswith('_u0') or k.endswith('_u1'):
            assert np.shape(v) == golden[k].shape, k
            np.testing.assert_allclose(v, golden[k], err_msg=k, **MOM_TOL)
        elif k.endswith('_L'):
            np.testing.assert_allclose(v, golden[k], err_msg=k, rtol=L_RTOL)
        else:
            np.testing.assert_allclose(v, golden[k], err_msg=k, rtol=L_RTOL, atol=1e-9)
        checked += 1
    assert checked == (1 + 5 + 6) + (6 if tag == 'five' else 0)


@pytest.mark.parametrize('tag', anneal_models.DIAG_CASES)
def test_diag_plan_reproduces_annealed_reference_trace(golden, tag):
    g = {k[3:]: golden[k] for k in golden.files if k.startswith('in_')}
    res = anneal_models.run_diag_cases(_diag_mods(), g, only=(tag,))
    check_diag(res, golden, tag)
    calls = res[tag + '_plan'].plans[0].kernels.calls
    assert 'tables_annealed' in calls and 'update_mu_annealed' in calls
    if tag == 'five':
        # the last stage of the schedule ran the plain entry points; the bound at 0.5 after it
        # formed the parts of that q
        assert 'parts_mu' in calls and 'parts_tau' in calls


def test_diag_bound_cache_includes_the_coefficients(golden):
    g = {k[3:]: golden[k] for k in golden.files if k.startswith('in_')}
    from dgmm_models import build_dgmm
    mods = _diag_mods()
    m = build_dgmm(mods, 300, 5, 3, g['four_y'])
    m['Z'].initialize_from_value(g['four_z0'][:, None])
    Q = mods['VB'](m['Y'], m['Z'], m['mu'], m['tau'], m['alpha'])
    Q.ignore_bound_checks = True
    Q.update(m['mu'], m['tau'], m['alpha'], m['Z'], repeat=2, verbose=False)
    calls = Q.plans[0].kernels.calls
    L1 = Q.compute_lowerbound()
    n = len(calls)
    assert Q.compute_lowerbound() == L1 and len(calls) == n
    Q.set_annealing(0.5)
    L2 = Q.compute_lowerbound()
    assert L2 != L1 and 'parts_mu' in calls[n:] and 'parts_tau' in calls[n:]
    n = len(calls)
    assert Q.compute_lowerbound() == L2 and len(calls) == n
    Q.set_annealing(1.0)
    assert Q.compute_lowerbound() == L1


@pytest.mark.parametrize('beta', [1.0, 0.5, 0.1])
@pytest.mark.parametrize('N,D,K', [(300, 5, 3), (300, 70, 17)])
def test_annealed_device_functions_against_long_double(N, D, K, beta):
    """The annealed updates of vmp_dgmm_dev.h (g++) and their parts A, B against the long-double
    restatement of phi_q = beta (...), within 8 times the deviation of the float64 NumPy
    evaluation of the same formulas, floor 4 ulp (dgmm_host.tolerances)."""
    from dgmm_host import make_inputs, host_tables, host_pass, host_update, tolerances, error
    from anneal_host import (host_update_annealed, host_tables_annealed, restate_annealed,
                             ANNEALED_QUANTITIES)
    g = make_inputs(N, D, K)
    h, q, c, _ = host_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])
    st = host_pass(N, D, K, g['y'], None, h, q, c)
    args = (beta, g['m0'], g['beta0'], g['a0'], g['b0'], st['S1'], st['S2'], st['Nk'], g['mu_mom'],
            g['tau_mom'])
    ld, f64 = restate_annealed(*args), restate_annealed(*args, dtype=np.float64)
    tol, dev = tolerances(ld, f64, ANNEALED_QUANTITIES)
    got = {}
    got['mu_par'], got['mu_mom'], got['mu_A'], got['mu_B'] = host_update_annealed(
        D, K, 0, beta, g['m0'], g['beta0'], st['S1'], st['S2'], st['Nk'], g['tau_mom'])
    got['tau_par'], got['tau_mom'], got['tau_A'], got['tau_B'] = host_update_annealed(
        D, K, 1, beta, g['a0'], g['b0'], st['S1'], st['S2'], st['Nk'], g['mu_mom'])
    for key in ANNEALED_QUANTITIES:
        assert error(got[key], ld[key]) <= tol[key], (key, error(got[key], ld[key]), tol[key])
    # the parts alone, from the tables the update left, are the update's own
    _, _, A, B = host_update_annealed(D, K, 2, 1.0, g['m0'], g['beta0'], None, None, None, None,
                                      got['mu_par'], got['mu_mom'])
    assert (A, B) == (got['mu_A'], got['mu_B'])
    _, _, A, B = host_update_annealed(D, K, 3, 1.0, g['a0'], g['b0'], None, None, None, None,
                                      got['tau_par'], got['tau_mom'])
    assert (A, B) == (got['tau_A'], got['tau_B'])
    if beta == 1.0:
        # the plain forms bit for bit
        for which, pa, pb, other, key in ((0, 'm0', 'beta0', 'tau_mom', 'mu'),
                                          (1, 'a0', 'b0', 'mu_mom', 'tau')):
            par, mom, _ = host_update(D, K, which, g[pa], g[pb], st['S1'], st['S2'], st['Nk'],
                                      g[other])
            assert np.array_equal(par, got[key + '_par']) and np.array_equal(mom, got[key + '_mom'])
        for a, b in zip(host_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi']),
                        host_tables_annealed(D, K, 1.0, g['mu_mom'], g['tau_mom'], g['elog_pi'])):
            assert np.array_equal(a, b)
    else:
        hb, qb, cb, gb = host_tables_annealed(D, K, beta, g['mu_mom'], g['tau_mom'], g['elog_pi'])
        h1, q1, c1, g1 = host_tables(D, K, g['mu_mom'], g['tau_mom'], g['elog_pi'])
        assert np.array_equal(hb, beta * h1) and np.array_equal(qb, beta * q1)
        assert np.array_equal(gb, g1) and cb.max() == 0
        np.testing.assert_allclose(cb, beta * (c1 - c1[np.argmax(cb)]), rtol=0, atol=1e-12)


def test_declining_plans_raise_on_a_coefficient_set_directly():
    """node.annealing can be set without VB.set_annealing: the plans that decline say so at the
    update or bound request instead of running half annealed."""
    from bayespy_amd.inference.plans.gmm import GMMSVIPlan
    from bayespy_amd.inference.plans.dgmm_masked import MaskedDiagGaussianMixturePlan
    node = _Node(None)
    assert GMMSVIPlan._annealing(node) == 1.0
    node.annealing = 0.5
    with pytest.raises(NotImplementedError, match='annealing is not built into the fused'):
        GMMSVIPlan._annealing(node)
    with pytest.raises(NotImplementedError, match='annealing is not built into the fused'):
        MaskedDiagGaussianMixturePlan._annealing(
            MaskedDiagGaussianMixturePlan.__new__(MaskedDiagGaussianMixturePlan), node)
