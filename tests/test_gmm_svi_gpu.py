"""GPU: the fused Gaussian-mixture block under stochastic variational inference -- the traces of the
live reference through ``VB(..., engine='fused')`` (GMMSVIPlan), and ``vmp_gmm_natural_step`` alone
at the shapes where it can go wrong (both edges of each wavefronts-per-cluster instance, a ragged
last workgroup, the largest K)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import gmm_svi_models as M                                          # noqa: E402
from gmm_svi_host import natural_step_reference                     # noqa: E402

EPS = 2.0 ** -52
N_ROWS = 257


def _mods():
    import bayespy_amd.nodes
    from bayespy_amd.inference import VB
    return dict(nodes=bayespy_amd.nodes, VB=VB, vb_kwargs=dict(engine='fused'))


@pytest.fixture(scope='module')
def golden():
    return dict(np.load(os.path.join(GOLDEN, 'gmm_svi.npz')))


@pytest.mark.parametrize('tag', M.CASES)
def test_fixture_traces_on_the_block(golden, tag):
    res = M.run_case(_mods(), golden, tag)
    assert type(res[tag + '_plan'].plans[0]).__name__ == 'GMMSVIPlan'
    M.check_case(res, golden, tag)


def test_generic_engines_trace_on_the_block():
    """tests/golden/svi_gmm.npz (the trace of test_generic_engine_gpu.py) on the fused block, at
    that test's tolerances."""
    from bayespy_amd.nodes import GaussianARD, Gaussian, Dirichlet, Categorical, Mixture
    from bayespy_amd.inference import VB
    g = np.load(os.path.join(GOLDEN, 'svi_gmm.npz'))
    data, batches = g['data'], g['batches']
    N, NB = int(g['N']), int(g['NB'])
    K, D = g['mu0'].shape
    mu = GaussianARD(0, 0.001, shape=(D,), plates=(K,), name='means')
    alpha = Dirichlet(np.ones(K), name='class probabilities')
    Z = Categorical(alpha, plates=(NB,), plates_multiplier=(N / NB,), name='classes')
    Y = Mixture(Z, Gaussian, mu, np.identity(D), name='observations')
    mu.initialize_from_value(g['mu0'])
    Q = VB(Y, Z, mu, alpha, engine='fused')
    Q.ignore_bound_checks = True
    assert type(Q.plans[0]).__name__ == 'GMMSVIPlan'
    for n in range(len(batches)):
        Y.observe(data[batches[n], :])
        Q.update(Z, verbose=False)
        Q.gradient_step(mu, alpha, scale=(n + 1) ** (-0.7))
        np.testing.assert_allclose(Q.compute_lowerbound(), g['L'][n], rtol=1e-9)
        np.testing.assert_allclose(mu.u[0], g['mu_u0'][n], rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(alpha.u[0], g['alpha_u0'][n], rtol=1e-7)
    np.testing.assert_allclose(Z.u[0], g['Z_u0_last'], rtol=1e-7, atol=1e-12)
    terms = [Y.lower_bound_contribution(), Z.lower_bound_contribution(),
             mu.lower_bound_contribution(), alpha.lower_bound_contribution()]
    np.testing.assert_allclose(terms, g['L_terms_last'], rtol=1e-9, atol=1e-9)


def test_observe_uses_device_tensor_in_place_and_reuses_host_buffer(golden):
    import torch
    res = {}

    def observe(Y, rows, n):
        if n % 2 == 0:
            t = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
            Y.observe(t)
            res['dev'] = t
        else:
            Y.observe(rows)
        res['n'] = n

    def on_step(Q, m, n):
        p = Q.plans[0]
        if n % 2 == 0:
            assert p.Yd.data_ptr() == res['dev'].data_ptr()
        else:
            res.setdefault('host_ptr', p.Yd.data_ptr())
            assert p.Yd.data_ptr() == res['host_ptr']
            assert p.Yd.data_ptr() != res['dev'].data_ptr()
        res.setdefault('state_ptr', p.state.data_ptr())
        assert p.state.data_ptr() == res['state_ptr']
    out = M.run_case(_mods(), golden, 'wishart_d3', observe=observe, on_step=on_step)
    M.check_case(out, golden, 'wishart_d3')


def test_one_device_tensor_filled_again_keeps_the_state(golden):
    """One resident batch tensor, filled in place and observed again at every step: used in place,
    the state stays, the trace is the reference's."""
    import torch
    import warnings
    res = {}

    def observe(Y, rows, n):
        if 'buf' not in res:
            res['buf'] = torch.empty(rows.shape, dtype=torch.float64, device='cuda')
        res['buf'].copy_(torch.from_numpy(np.ascontiguousarray(rows)))
        Y.observe(res['buf'])

    def on_step(Q, m, n):
        p = Q.plans[0]
        assert p.Yd.data_ptr() == res['buf'].data_ptr()
        res.setdefault('state', p.state)
        res.setdefault('phi', p.phi_mu)
        assert p.state is res['state'] and p.phi_mu is res['phi'] and p._ready
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        out = M.run_case(_mods(), golden, 'wishart_d3', observe=observe, on_step=on_step)
    M.check_case(out, golden, 'wishart_d3')


# ---- the kernel alone ---------------------------------------------------------------------------

def _spd(rs, D, cond):
    q, _ = np.linalg.qr(rs.normal(size=(D, D)))
    e = np.exp(rs.uniform(0.0, np.log(cond), size=D)) / np.sqrt(cond)
    a = (q * e) @ q.T
    return 0.5 * (a + a.T)


class _Bench:
    """A packed state with T from ONE vmp_gmm_pass over seeded rows, after a labelled start."""

    def __init__(self, D, K):
        import torch
        from bayespy_amd.device import get_runtime
        from bayespy_amd.inference.plans.gmm import GMMKernels
        self.D, self.K, self.torch = D, K, torch
        rs = np.random.RandomState(1000 * D + K)
        self.rt = rt = get_runtime()
        self.k = k = GMMKernels(rt)
        rt.sync_stream()
        self.L = L = k.layout(D, K)
        self.beta0, self.n0 = 0.7, D + 2.0
        self.V0 = _spd(rs, D, 1e3)
        self.alpha0 = rs.uniform(0.5, 2.0, size=K)
        y = rs.normal(size=(N_ROWS, D)) + 2.0 * rs.normal(size=(K, D))[rs.randint(K, size=N_ROWS)]
        self.Y = torch.from_numpy(y).cuda()
        self.R = rt.empty(N_ROWS, K)
        self.ws = rt.empty(int(k.workspace_doubles(D, K)))
        st = rt.zeros(int(L.total))
        k.init_state(D, K, self.alpha0, self.beta0, self.n0, self.V0, st)
        lab = torch.from_numpy(rs.randint(K, size=N_ROWS).astype(np.int64)).cuda()
        k.stats_from_labels(self.Y, N_ROWS, D, K, lab, self.R, st, self.ws)
        k.update_mu(D, K, st)
        k.update_lambda(D, K, st)
        k.update_alpha(D, K, st)
        k.prepare_z(D, K, False, st)
        k.pass_(self.Y, N_ROWS, D, K, self.R, st, self.ws)
        self.state = st
        self.phi = rt.empty(K * (D + D * D))
        k.natural_init(D, K, st, self.phi)
        # natural parameters of q(mu) that match the moments in the state: one full step of mu on
        # a copy gives (h, Lambda_mu) of exactly those moments' update; keep the moments it wrote
        k.natural_step(D, K, 1, 1.0, 1.0, st, self.phi)
        k.pass_(self.Y, N_ROWS, D, K, self.R, st, self.ws)

    def fields(self, st, phi):
        L, D, K = self.L, self.D, self.K
        s = st.cpu().numpy()
        KP, FS = int(L.KP), int(L.FS)
        T = s[L.off_T:L.off_T + KP * FS].reshape(KP, FS)[:K]

        def blk(off, shape):
            return s[off:off + int(np.prod(shape))].reshape(shape).copy()
        return dict(R=T[:, 0].copy(), S1=T[:, 1:1 + D].copy(), S2=T[:, 1 + D:].reshape(K, D, D).copy(),
                    mu=blk(L.off_mu, (K, D)), Cmu=blk(L.off_Cmu, (K, D, D)),
                    Lam=blk(L.off_Lam, (K, D, D)), nk=blk(L.off_nk, (K,)),
                    Vk=blk(L.off_Vk, (K, D, D)), alpha=blk(L.off_alpha, (K,)),
                    phi=phi.cpu().numpy().reshape(K, D + D * D).copy(),
                    status=float(s[L.off_scal + 3]))

    def step(self, nodes, mult, scale, st=None, phi=None):
        st = self.state.clone() if st is None else st
        phi = self.phi.clone() if phi is None else phi
        self.k.natural_step(self.D, self.K, nodes, mult, scale, st, phi)
        return st, phi

    def restate(self, f, nodes, mult, scale):
        return natural_step_reference(self.D, self.K, nodes, mult, scale, f['R'], f['S1'], f['S2'],
                                      f['mu'], f['Cmu'], f['Lam'], f['nk'], f['Vk'], f['alpha'],
                                      f['phi'], self.beta0, self.n0, self.V0, self.alpha0)

    def abs_terms(self, f, mult, scale):
        """Sum of the absolute values of the terms of every natural parameter of a step."""
        D, K = self.D, self.K
        a = {k: np.abs(v) for k, v in f.items() if isinstance(v, np.ndarray)}
        I = np.identity(D)
        mR = mult * a['R']
        Lmu = self.beta0 * I + mR[:, None, None] * a['Lam']
        h = np.einsum('kij,kj->ki', a['Lam'], mult * a['S1'])
        mm = a['Cmu'] + a['mu'][:, :, None] * a['mu'][:, None, :]
        sm = (mult * a['S1'])[:, :, None] * a['mu'][:, None, :]
        V = np.abs(self.V0) + mult * a['S2'] + sm + np.swapaxes(sm, 1, 2) + mR[:, None, None] * mm

        def step(old, new):
            return old + scale * (new + old)
        return dict(Lmu=step(a['phi'][:, D:].reshape(K, D, D), Lmu), h=step(a['phi'][:, :D], h),
                    nk=step(a['nk'], self.n0 + mR), Vk=step(a['Vk'], V),
                    alpha=step(a['alpha'], self.alpha0 + mR))

    def check_parameters(self, got, want, terms, keys):
        D, K = self.D, self.K
        have = dict(Lmu=got['phi'][:, D:].reshape(K, D, D), h=got['phi'][:, :D], nk=got['nk'],
                    Vk=got['Vk'], alpha=got['alpha'])
        for key in keys:
            err = np.abs(have[key] - want[key])
            bound = 8.0 * (D + 4) * EPS * terms[key]
            worst = float(np.max(err / np.maximum(bound, 1e-300)))
            print('D=%d K=%d %s: max error / bound = %.3g' % (D, K, key, worst))
            assert np.all(err <= bound), (key, worst)


SHAPES = [(D, K) for D in (1, 2, 8, 9, 16, 17) for K in (1, 5, 64)] + [(32, 5)]


@pytest.mark.parametrize('D, K', SHAPES)
def test_natural_step_kernel(D, K):
    torch = pytest.importorskip('torch')
    b = _Bench(D, K)
    k, L = b.k, b.L
    # (a) one node, scale = 1, mult = 1: the bits of the update kernels, in every slot of the state
    for bit, update in ((1, k.update_mu), (2, k.update_lambda), (4, k.update_alpha)):
        want = b.state.clone()
        update(D, K, want)
        got, _ = b.step(bit, 1.0, 1.0)
        same = torch.equal(got, want)
        if not same:
            d = (got != want).nonzero().reshape(-1).cpu().numpy()
            print('D=%d K=%d bit %d: %d words differ, first at %s' % (D, K, bit, len(d), d[:8]))
        assert same, 'nodes=%d differs from the update kernel' % bit
    # (b) all three nodes, scale = 0.3, mult = 7.5, against the float64 restatement
    f0 = b.fields(b.state, b.phi)
    st, phi = b.step(7, 7.5, 0.3)
    got = b.fields(st, phi)
    assert got['status'] == 0.0
    want = b.restate(f0, 7, 7.5, 0.3)
    terms = b.abs_terms(f0, 7.5, 0.3)
    b.check_parameters(got, want, terms, ('Lmu', 'h', 'nk', 'Vk', 'alpha'))
    # the inverses of the matrices the kernel holds: Lambda_mu Cov = I and V <Lambda> / n = I, the
    # condition numbers from the restated matrices
    I = np.identity(D)
    Lg = got['phi'][:, D:].reshape(K, D, D)
    Vg = 0.5 * (got['Vk'] + np.swapaxes(got['Vk'], 1, 2))
    Vs = 0.5 * (want['Vk'] + np.swapaxes(want['Vk'], 1, 2))
    for c in range(K):
        r1 = np.max(np.abs(Lg[c] @ got['Cmu'][c] - I))
        b1 = 8.0 * D * EPS * np.linalg.cond(want['Lmu'][c])
        r2 = np.max(np.abs(Vg[c] @ got['Lam'][c] / got['nk'][c] - I))
        b2 = 8.0 * D * EPS * np.linalg.cond(Vs[c])
        if c == 0 or r1 > b1 or r2 > b2:
            print('D=%d K=%d k=%d: residuals %.3g (bound %.3g), %.3g (bound %.3g)'
                  % (D, K, c, r1, b1, r2, b2))
        assert r1 <= b1 and r2 <= b2, (c, r1, b1, r2, b2)
    # (c) the simultaneous rule: mu and Lambda together read the OLD moments of each other
    st12, phi12 = b.step(3, 7.5, 0.3)
    sq, pq = b.step(1, 7.5, 0.3)
    sq, pq = b.step(2, 7.5, 0.3, sq, pq)
    g12, gq = b.fields(st12, phi12), b.fields(sq, pq)
    assert not np.array_equal(g12['Vk'], gq['Vk'])
    b.check_parameters(g12, b.restate(f0, 3, 7.5, 0.3), terms, ('Lmu', 'h', 'nk', 'Vk'))
    np.testing.assert_array_equal(g12['alpha'], f0['alpha'])
    # (d) two identical calls on copies: equal bits
    st2, phi2 = b.step(7, 7.5, 0.3)
    assert torch.equal(st, st2) and torch.equal(phi, phi2)


@pytest.mark.parametrize('D', [2, 9, 17])
def test_indefinite_scale_matrix_sets_the_status(D):
    """A V* with a negative pivot: S1 of cluster 0 is scaled so that -2 m S1_0 <mu_0> dominates the
    first diagonal element.  A status, not a fault."""
    from bayespy_amd import _lib
    K = 5
    b = _Bench(D, K)
    f0 = b.fields(b.state, b.phi)
    st = b.state.clone()
    sign = 1.0 if f0['mu'][0, 0] >= 0 else -1.0
    big = (np.abs(f0['Vk'][0]).max() + np.abs(f0['S2'][0]).max() + 1.0) * 1e6 \
        / max(abs(f0['mu'][0, 0]), 1e-3)
    st[b.L.off_T + 1] = sign * big
    st, _ = b.step(2, 7.5, 1.0, st)
    assert b.fields(st, b.phi)['status'] == float(_lib.VMP_ERR_NOT_POSDEF)


def test_plan_raises_on_indefinite_scale_matrix(golden):
    from bayespy_amd import _lib
    m_ = _mods()
    tag = 'wishart_d3'
    m = M.build(m_, golden, tag)
    Q = m_['VB'](m['Y'], m['Z'], m['mu'], m['alpha'], m['Lambda'], engine='fused')
    Q.ignore_bound_checks = True
    m['Y'].observe(golden[tag + '_data'].astype(np.float64)[golden[tag + '_batches'][0]])
    Q.update(m['Z'], verbose=False)
    p = Q.plans[0]
    mu00 = float(m['mu'].u[0][0, 0])
    p.state[p.layout.off_T + 1] = (1.0 if mu00 >= 0 else -1.0) * 1e9 / max(abs(mu00), 1e-3)
    Q.gradient_step(m['Lambda'], scale=1.0)
    with pytest.raises(_lib.NotPositiveDefiniteError):
        Q.compute_lowerbound()
