"""TEST INFRASTRUCTURE for deterministic annealing on the fused diagonal-Gaussian-mixture block.

* ``anneal_host()``: ctypes library of tests/host/anneal_host.cpp, built with g++ from
  csrc/vmp_dgmm_dev.h -- the annealed arithmetic of csrc/vmp_dgmm.hip.
* ``restate_annealed``: the annealed updates and the parts A, B of their bound terms in a dtype of
  the caller's choice, in the reference's own form (expfamily.py:343-350, :400-480).
* ``AnnealedCPUDGMMKernels``: CPUDGMMKernels (tests/dgmm_host.py) + the annealed entry points.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np

from dgmm_host import CPUDGMMKernels, _c, _p, _special
from host_build import build_host_library, special_functions_text


@functools.lru_cache(None)
def anneal_host():
    lib = build_host_library('anneal', ['tests/host/anneal_host.cpp',
                                        'bayespy_amd/csrc/vmp_dgmm_dev.h'],
                             prelude=special_functions_text())
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    lib.anneal_tables.argtypes = [i32, i32, f64] + [vp] * 7
    lib.anneal_tables.restype = None
    lib.anneal_update.argtypes = [i32, i32, i32, f64] + [vp] * 9
    lib.anneal_update.restype = None
    return lib


def host_tables_annealed(D, K, beta, mu_mom, tau_mom, elog_pi):
    h, q, c, gsum = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K), np.zeros(K)
    bufs = (_c(mu_mom), _c(tau_mom), _c(elog_pi))
    anneal_host().anneal_tables(D, K, beta, *[_p(b) for b in bufs], _p(h), _p(q), _p(c), _p(gsum))
    return h, q, c, gsum


def host_update_annealed(D, K, which, beta, prior_a, prior_b, S1, S2, Nk, other, par=None,
                         mom=None):
    """(par, mom (D K, 2), A, B) of the host build; which 2 / 3 read the given par and mom."""
    par = np.zeros((D * K, 2)) if par is None else np.array(par, dtype=np.float64, order='C')
    mom = np.zeros((D * K, 2)) if mom is None else np.array(mom, dtype=np.float64, order='C')
    ab = np.zeros(2)
    bufs = [_c(np.broadcast_to(prior_a, (D, K))), _c(np.broadcast_to(prior_b, (D, K))), _c(S1),
            _c(S2), _c(Nk), _c(other)]
    anneal_host().anneal_update(D, K, which, beta, *[_p(b) for b in bufs], _p(par), _p(mom), _p(ab))
    return par, mom, float(ab[0]), float(ab[1])


def restate_annealed(beta, m0, beta0, a0, b0, S1, S2, Nk, mu_mom, tau_mom, dtype=np.longdouble):
    """phi_q = beta (phi from the parents + the messages), the moments and g from phi_q, and per
    node A = cgf_p + phi_p . u, B = phi_q . u + g_q, each summed over the (D, K) elements."""
    psi, lgam = _special(dtype)
    D, K = np.shape(S1)
    t = lambda a: np.array(np.broadcast_to(a, (D, K)), dtype=dtype)     # noqa: E731
    m0, beta0, a0, b0, S1, S2 = (t(a) for a in (m0, beta0, a0, b0, S1, S2))
    Nk = np.asarray(Nk, dtype=dtype)
    mu, tau = (np.asarray(a, dtype=dtype).reshape(D, K, 2) for a in (mu_mom, tau_mom))
    beta, half = dtype(beta), dtype(1) / 2
    # mu: phi_q = beta [beta0 m0 + <tau> S1, -1/2 (beta0 + <tau> N_k)]
    p0, p1 = beta * (beta0 * m0 + tau[..., 0] * S1), -half * beta * (beta0 + tau[..., 0] * Nk)
    lam = -2 * p1
    m = p0 / lam
    u = np.stack([m, m * m + 1 / lam], -1)
    A_mu = (-half * beta0 * m0 * m0 + half * np.log(beta0)) + beta0 * m0 * u[..., 0] \
        - half * beta0 * u[..., 1]
    B_mu = p0 * u[..., 0] + p1 * u[..., 1] + (-half * lam * m * m + half * np.log(lam))
    # tau: phi_q = beta [-(b0 + ...), a0 + N_k / 2]
    a = beta * (a0 + Nk / 2)
    b = beta * (b0 + (S2 - 2 * mu[..., 0] * S1 + mu[..., 1] * Nk) / 2)
    v = np.stack([a / b, psi(a) - np.log(b)], -1)
    A_tau = (a0 * np.log(b0) - lgam(a0)) - b0 * v[..., 0] + a0 * v[..., 1]
    B_tau = -b * v[..., 0] + a * v[..., 1] + (a * np.log(b) - lgam(a))
    return dict(mu_par=np.stack([m, lam], -1).reshape(D * K, 2), mu_mom=u.reshape(D * K, 2),
                mu_A=A_mu.sum(), mu_B=B_mu.sum(),
                tau_par=np.stack([a, b], -1).reshape(D * K, 2), tau_mom=v.reshape(D * K, 2),
                tau_A=A_tau.sum(), tau_B=B_tau.sum())


ANNEALED_QUANTITIES = ('mu_par', 'mu_mom', 'mu_A', 'mu_B', 'tau_par', 'tau_mom', 'tau_A', 'tau_B')


class AnnealedCPUDGMMKernels(CPUDGMMKernels):
    """Double of DGMMKernels with the annealed entry points, on CPU tensors."""

    def tables_annealed(self, D, K, annealing, mu_mom, tau_mom, elog_pi, h, q, c, gsum=None):
        self.calls.append('tables_annealed')
        hh, qq, cc, gg = host_tables_annealed(D, K, annealing, mu_mom.numpy(), tau_mom.numpy(),
                                              elog_pi.numpy())
        h.numpy()[...] = hh
        q.numpy()[...] = qq
        c.numpy()[...] = cc
        if gsum is not None:
            gsum.numpy()[...] = gg

    def update_annealed(self, D, K, which, annealing, prior_a, prior_b, S1, S2, Nk, other, par, mom,
                        ab):
        self.calls.append(('update_mu_annealed', 'update_tau_annealed', 'parts_mu',
                           'parts_tau')[which])
        p, m, A, B = host_update_annealed(D, K, which, annealing, prior_a.numpy(), prior_b.numpy(),
                                          self._np(S1), self._np(S2), self._np(Nk), self._np(other),
                                          par.numpy(), mom.numpy())
        par.numpy()[...] = p
        mom.numpy()[...] = m
        ab.numpy()[...] = [A, B]
