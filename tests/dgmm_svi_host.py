"""TEST INFRASTRUCTURE for stochastic variational inference on the two diagonal-Gaussian blocks.

* ``dgmm_svi_host()``: ctypes library of tests/host/dgmm_svi_host.cpp, built with g++ from
  csrc/vmp_dgmm_svi_dev.h -- the arithmetic and the order of additions of csrc/vmp_dgmm_svi.hip.
* ``restate_step``: NumPy restatement of the step of mu and tau in a dtype of the caller's choice, in
  the reference's own form: the optimum in the natural parameters, phi <- phi + scale (phi* - phi),
  the moments from phi and the bound terms as cgf of the prior - cgf of q + sum (phi_p - phi_q) u
  (expfamily.py:400-480).  Long double is the yardstick (digamma and ln Gamma of
  tests/mix_svi_host.py), float64 the reference's own arithmetic.  The weights row is
  ``restate_dirichlet_step`` of tests/mix_svi_host.py.
* ``SVIStepDouble``: ``natural_step`` / ``natural_step_workspace`` for the kernel doubles of the two
  blocks, and ``on_double(tag)``: the double of a case of tests/dgmm_svi_models.py with them.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np

from host_build import build_host_library, special_functions_text
from mix_svi_host import restate_dirichlet_step, special

STEP_QUANTITIES = ('mu_par', 'mu_mom', 'mu_bound', 'tau_par', 'tau_mom', 'tau_bound')


@functools.lru_cache(None)
def dgmm_svi_host():
    lib = build_host_library('dgmm_svi', ['tests/host/dgmm_svi_host.cpp',
                                          'bayespy_amd/csrc/vmp_dgmm_svi_dev.h',
                                          'bayespy_amd/csrc/vmp_dgmm_masked_dev.h',
                                          'bayespy_amd/csrc/vmp_dgmm_dev.h'],
                             prelude=special_functions_text())
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.dgmm_svi_step.argtypes = [i32] * 4 + [vp] * 11 + [f64, f64, vp]
    lib.dgmm_svi_step.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def host_step(D, K, nodes, per_element, m0, beta0, a0, b0, S1, S2, cnt, mu_par, mu_mom, tau_par,
              tau_mom, mult, scale, bound=None):
    """The host build on copies of the four tables: dict of mu_par, mu_mom, tau_par, tau_mom
    ((D K, 2) each) and bound (2; what it held where a node is not named)."""
    t = [np.array(a, dtype=np.float64, order='C').reshape(D * K, 2)
         for a in (mu_par, mu_mom, tau_par, tau_mom)]
    b = np.full(2, np.nan) if bound is None else np.array(bound, dtype=np.float64)[:2].copy()
    bufs = [_c(np.broadcast_to(a, (D, K))) for a in (m0, beta0, a0, b0)] \
        + [_c(S1), _c(S2), _c(cnt)]
    dgmm_svi_host().dgmm_svi_step(D, K, nodes, per_element, *[_p(a) for a in bufs],
                                  *[_p(a) for a in t], float(mult), float(scale), _p(b))
    return dict(mu_par=t[0], mu_mom=t[1], tau_par=t[2], tau_mom=t[3], bound=b)


def restate_step(m0, beta0, a0, b0, S1, S2, cnt, mu_par, mu_mom, tau_par, tau_mom, mult, scale,
                 dtype=np.longdouble):
    """Priors, statistics and ``cnt`` as (D, K) arrays (``cnt`` broadcast by the caller; statistics
    None: phi* is the prior), tables (D K, 2).  Both nodes step from the state given; scale == 1
    does not look at the old parameters.  dict of STEP_QUANTITIES."""
    psi, lgam = special(dtype)
    D, K = np.shape(m0)
    t = lambda a: np.array(np.broadcast_to(a, (D, K)), dtype=dtype)     # noqa: E731
    m0, beta0, a0, b0 = (t(a) for a in (m0, beta0, a0, b0))
    zero = np.zeros((D, K), dtype=dtype)
    S1, S2, cnt = (zero if a is None else t(a) for a in (S1, S2, cnt))
    mu, tau = (np.asarray(a, dtype=dtype).reshape(D, K, 2) for a in (mu_mom, tau_mom))
    half, mult, scale_ = dtype(1) / 2, dtype(mult), dtype(scale)
    # the optima in the natural parameters: (lambda m, -lambda / 2) and (-b, a)
    f1 = beta0 * m0 + mult * tau[..., 0] * S1
    f2 = -half * (beta0 + mult * tau[..., 0] * cnt)
    a_s = a0 + mult * cnt / 2
    b_s = b0 + mult * (S2 - 2 * mu[..., 0] * S1 + mu[..., 1] * cnt) / 2
    if scale != 1:
        mo, to = (np.asarray(a, dtype=dtype).reshape(D, K, 2) for a in (mu_par, tau_par))
        o1, o2 = mo[..., 1] * mo[..., 0], -half * mo[..., 1]
        f1, f2 = o1 + scale_ * (f1 - o1), o2 + scale_ * (f2 - o2)
        a_s, b_s = to[..., 0] + scale_ * (a_s - to[..., 0]), to[..., 1] + scale_ * (b_s - to[..., 1])
    lam = -2 * f2
    m = f1 / lam
    u = np.stack([m, m * m + 1 / lam], -1)
    Lmu = (-half * beta0 * m0 * m0 + half * np.log(beta0)) - (-half * lam * m * m + half * np.log(lam)) \
        + (beta0 * m0 - f1) * u[..., 0] + (-half * beta0 - f2) * u[..., 1]
    a, b = a_s, b_s
    v = np.stack([a / b, psi(a) - np.log(b)], -1)
    Ltau = (a0 * np.log(b0) - lgam(a0)) - (a * np.log(b) - lgam(a)) \
        + (-b0 + b) * v[..., 0] + (a0 - a) * v[..., 1]
    return dict(mu_par=np.stack([m, lam], -1).reshape(D * K, 2), mu_mom=u.reshape(D * K, 2),
                mu_bound=Lmu.sum(), tau_par=np.stack([a, b], -1).reshape(D * K, 2),
                tau_mom=v.reshape(D * K, 2), tau_bound=Ltau.sum())


def step_inputs(D, K, per_element, rows=70):
    """Inputs of one step at (D, K): the data, the priors and the moment tables of
    ``dgmm_host.make_inputs`` for a mini-batch of ``rows`` rows, and statistics a pass could leave
    on them -- soft responsibilities r, N_k = sum r, S1 = y^T r, S2 = (y o y)^T r and, with hidden
    entries (``per_element``), the same over the seen entries and M = m^T r.  The old parameters
    are those the moment tables belong to.  dict of m0, beta0, a0, b0, S1, S2 (D, K), cnt (K, or
    (D, K) per element), full (cnt as (D, K)), mu_par, mu_mom, tau_par, tau_mom (D K, 2) and the
    weights row prior_r, Nk, alpha_r (K)."""
    from dgmm_host import make_inputs
    from scipy.special import digamma
    g = make_inputs(rows, D, K)
    rs = np.random.RandomState(4000 * K + 40 * D + per_element)
    r = rs.dirichlet(np.ones(K), size=rows)
    seen = (rs.rand(rows, D) < 0.7) if per_element else np.ones((rows, D), dtype=bool)
    y = g['y'] * seen
    S1, S2 = y.T @ r, (y * y).T @ r
    cnt = seen.astype(np.float64).T @ r if per_element else r.sum(axis=0)
    m, mu2 = g['mu_mom'].reshape(D, K, 2)[..., 0], g['mu_mom'].reshape(D, K, 2)[..., 1]
    tau = g['tau_mom'].reshape(D, K, 2)[..., 0]
    a = rs.gamma(50.0, 2.0, size=(D, K))
    b = a / tau
    return dict(m0=g['m0'], beta0=g['beta0'], a0=g['a0'], b0=g['b0'], S1=S1, S2=S2, cnt=cnt,
                full=np.array(np.broadcast_to(cnt, (D, K))),
                mu_par=np.stack([m, 1 / (mu2 - m * m)], -1).reshape(D * K, 2), mu_mom=g['mu_mom'],
                tau_par=np.stack([a, b], -1).reshape(D * K, 2),
                tau_mom=np.stack([tau, digamma(a) - np.log(b)], -1).reshape(D * K, 2),
                prior_r=rs.gamma(1.0, 1.0, size=K) + 0.01, Nk=r.sum(axis=0),
                alpha_r=rs.gamma(2.0, 2.0, size=K) + 0.01)


class SVIStepDouble:
    """Mixin of a kernels double of the block that has ``calls``: the tables through the host build,
    the weights row in float64 NumPy / SciPy."""

    def natural_step_workspace(self, D, K):
        return 2 * D * K + 1

    def natural_step(self, D, K, nodes, m0, beta0, a0, b0, S1, S2, cnt, per_element, mu_par, mu_mom,
                     tau_par, tau_mom, prior_r, Nk, alpha_r, elog_r, mult, scale, ws, bound):
        self.calls.append('natural_step_%d' % nodes)
        assert mult > 0 and 1 <= nodes <= 7
        n = lambda t: None if t is None else t.numpy()       # noqa: E731
        # every optimum is formed before anything is written
        w = None
        if nodes & 4:
            w = restate_dirichlet_step(n(prior_r).reshape(1, K),
                                       None if Nk is None else n(Nk).reshape(1, K),
                                       n(alpha_r).reshape(1, K).copy(), mult, scale, np.float64)
        if nodes & 3:
            o = host_step(D, K, nodes & 3, per_element, n(m0), n(beta0), n(a0), n(b0), n(S1), n(S2),
                          n(cnt), n(mu_par), n(mu_mom), n(tau_par), n(tau_mom), mult, scale,
                          bound.numpy())
            for key, t in (('mu_par', mu_par), ('mu_mom', mu_mom), ('tau_par', tau_par),
                           ('tau_mom', tau_mom)):
                t.numpy()[...] = o[key]
            bound.numpy()[:2] = o['bound']
        if w is not None:
            alpha_r.numpy()[...] = w['par'].reshape(K)
            elog_r.numpy()[...] = w['mom'].reshape(K)
            bound.numpy()[2] = float(w['bound'])


PLAN = dict(par='DiagGaussianMixtureSVIPlan', value='DiagGaussianMixtureSVIPlan',
            mask='MaskedDiagGaussianMixtureSVIPlan')


def double_class(tag):
    if tag == 'mask':
        from dgmm_masked_host import CPUDGMMMaskedKernels as Base
    else:
        from dgmm_host import CPUDGMMKernels as Base
    return type('SVI' + Base.__name__, (SVIStepDouble, Base), {})


def on_double(tag):
    """``after_vb`` of the model scripts: the plan of case ``tag`` on its kernel double."""
    def go(Q):
        from bayespy_amd.device import Runtime
        plan = Q.plans[0]
        assert type(plan).__name__ == PLAN[tag], type(plan).__name__
        rt = Runtime(device='cpu')
        plan._rt, plan._kernels = rt, double_class(tag)(rt)
    return go
