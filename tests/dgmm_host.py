"""TEST INFRASTRUCTURE for the fused diagonal-Gaussian-mixture block.

* ``dgmm_host()``: ctypes library of tests/host/dgmm_host.cpp, built with g++ from
  csrc/vmp_dgmm_dev.h -- the arithmetic and the order of additions of csrc/vmp_dgmm.hip.
* ``restate_pass`` / ``restate_update``: NumPy restatements in a dtype of the caller's choice (no
  chunks, no tiles; the updates and their bound terms in the reference's own form,
  expfamily.py:400-480): long double is the yardstick, float64 is the reference's own arithmetic.
* ``CPUDGMMKernels``: the double of the plan's kernel object (inference/plans/dgmm.py DGMMKernels)
  on CPU tensors.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np

from host_build import build_host_library, special_functions_text
from lda_host import CPUDirichletKernels

PASS_QUANTITIES = ('r', 'Nk', 'S1', 'S2', 'sum_lse', 'Nk_c', 'S_hq')
UPDATE_QUANTITIES = ('mu_mom', 'mu_bound', 'tau_mom', 'tau_bound')


@functools.lru_cache(None)
def dgmm_host():
    lib = build_host_library('dgmm', ['tests/host/dgmm_host.cpp', 'bayespy_amd/csrc/vmp_dgmm_dev.h'],
                             prelude=special_functions_text())
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    for name in ('dgmm_chunk_rows', 'dgmm_chunks'):
        getattr(lib, name).argtypes = [i64, i32, i32]
        getattr(lib, name).restype = i64
    lib.dgmm_partial_doubles.argtypes = [i32, i32]
    lib.dgmm_partial_doubles.restype = i64
    lib.dgmm_tables.argtypes = [i32, i32] + [vp] * 7
    lib.dgmm_tables.restype = None
    lib.dgmm_pass.argtypes = [i64, i32, i32] + [vp] * 10
    lib.dgmm_pass.restype = None
    lib.dgmm_update.argtypes = [i32, i32, i32] + [vp] * 9
    lib.dgmm_update.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def host_tables(D, K, mu_mom, tau_mom, elog_pi):
    """(h, q (D, K), c (K), gsum (K)) of the host build; moment tables (D K, 2) or None."""
    h, q, c, gsum = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K), np.zeros(K)
    bufs = (_c(mu_mom), _c(tau_mom), _c(elog_pi))
    dgmm_host().dgmm_tables(D, K, _p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(h), _p(q), _p(c),
                            _p(gsum))
    return h, q, c, gsum


def host_pass(N, D, K, y, labels, h, q, c, want_r=False):
    """dict of S1, S2 (D, K), Nk (K), sum_lse, Nk_c, S_hq, r or None of the host build."""
    S1, S2, Nk, scal = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K), np.zeros(1)
    r = np.full((N, K), np.nan) if want_r else None
    bufs = (_c(y), None if labels is None else np.ascontiguousarray(labels, dtype=np.int32),
            _c(h), _c(q), _c(c))
    dgmm_host().dgmm_pass(N, D, K, *[_p(b) for b in bufs], _p(S1), _p(S2), _p(Nk), _p(scal), _p(r))
    return dict(S1=S1, S2=S2, Nk=Nk, sum_lse=float(scal[0]), r=r, Nk_c=float(np.sum(Nk * bufs[4])),
                S_hq=float(np.sum(S1 * bufs[2]) + np.sum(S2 * bufs[3])))


def host_update(D, K, which, prior_a, prior_b, S1, S2, Nk, other):
    """(par (D K, 2), mom (D K, 2), bound) of the host build; statistics None: the prior."""
    par, mom, bound = np.zeros((D * K, 2)), np.zeros((D * K, 2)), np.zeros(1)
    bufs = [_c(np.broadcast_to(prior_a, (D, K))), _c(np.broadcast_to(prior_b, (D, K))), _c(S1),
            _c(S2), _c(Nk), _c(other)]
    dgmm_host().dgmm_update(D, K, which, *[_p(b) for b in bufs], _p(par), _p(mom), _p(bound))
    return par, mom, float(bound[0])


def restate_tables(mu_mom, tau_mom, elog_pi, D, K, dtype=np.longdouble):
    """h, q, c (less its maximum) and gsum from the moment tables, in ``dtype``."""
    mu, tau = (np.asarray(a, dtype=dtype).reshape(D, K, 2) for a in (mu_mom, tau_mom))
    h, q = tau[..., 0] * mu[..., 0], -tau[..., 0] / 2
    gsum = (tau[..., 1] / 2 - tau[..., 0] * mu[..., 1] / 2).sum(axis=0)
    c = gsum + np.asarray(elog_pi, dtype=dtype)
    return h, q, c - c.max(), gsum


def restate_pass(y, h, q, c, dtype=np.longdouble):
    """The pass on y (N, D) in ``dtype``, the way mixture.py / gaussian.py / categorical.py
    evaluate it: dict of r (N, K), lse (N), Nk, S1, S2 (D, K), sum_lse and the dot products of the
    bound, Nk . c and S1 . h + S2 . q."""
    y = np.asarray(y, dtype=dtype)
    h, q, c = (np.asarray(a, dtype=dtype) for a in (h, q, c))
    logit = c + y @ h + (y * y) @ q
    mx = logit.max(axis=1, keepdims=True) if len(y) else np.zeros((0, 1), dtype=dtype)
    lse = mx[:, 0] + np.log(np.exp(logit - mx).sum(axis=1))
    r = np.exp(logit - lse[:, None])
    Nk, S1, S2 = r.sum(axis=0), y.T @ r, (y * y).T @ r
    return dict(r=r, lse=lse, Nk=Nk, S1=S1, S2=S2, sum_lse=lse.sum(), Nk_c=np.sum(Nk * c),
                S_hq=np.sum(S1 * h) + np.sum(S2 * q))


def _special(dtype):
    """(digamma, gammaln) on arrays of ``dtype``: SciPy in float64, mpmath at 40 digits otherwise."""
    if dtype == np.float64:
        from scipy.special import digamma, gammaln
        return digamma, gammaln
    import mpmath
    mpmath.mp.dps = 40

    def lift(fn):
        def go(a):
            a = np.asarray(a, dtype=dtype)
            out = [np.longdouble(mpmath.nstr(fn(mpmath.mpf(np.format_float_positional(v))), 30))
                   for v in a.reshape(-1)]
            return np.array(out, dtype=dtype).reshape(a.shape)
        return go
    return lift(mpmath.digamma), lift(mpmath.loggamma)


def restate_update(m0, beta0, a0, b0, S1, S2, Nk, mu_mom, tau_mom, dtype=np.longdouble):
    """q(mu) from the statistics and the moments of tau, q(tau) from the statistics and the moments
    of mu (both from the SAME given moments, as two independent calls of vmp_dgmm_update), with
    the bound terms in the reference's form: cgf of the prior - cgf of q + sum (phi_p - phi_q) u."""
    psi, lgam = _special(dtype)
    D, K = np.shape(S1)
    t = lambda a: np.array(np.broadcast_to(a, (D, K)), dtype=dtype)     # noqa: E731
    m0, beta0, a0, b0, S1, S2 = (t(a) for a in (m0, beta0, a0, b0, S1, S2))
    Nk = np.asarray(Nk, dtype=dtype)
    mu, tau = (np.asarray(a, dtype=dtype).reshape(D, K, 2) for a in (mu_mom, tau_mom))
    half = dtype(1) / 2
    lam = beta0 + tau[..., 0] * Nk
    m = (beta0 * m0 + tau[..., 0] * S1) / lam
    u = np.stack([m, m * m + 1 / lam], -1)
    Lmu = (-half * beta0 * m0 * m0 + half * np.log(beta0)) - (-half * lam * m * m + half * np.log(lam)) \
        + (beta0 * m0 - lam * m) * u[..., 0] + (-half * beta0 + half * lam) * u[..., 1]
    a = a0 + Nk / 2
    b = b0 + (S2 - 2 * mu[..., 0] * S1 + mu[..., 1] * Nk) / 2
    v = np.stack([a / b, psi(a) - np.log(b)], -1)
    Ltau = (a0 * np.log(b0) - lgam(a0)) - (a * np.log(b) - lgam(a)) \
        + (-b0 + b) * v[..., 0] + (a0 - a) * v[..., 1]
    return dict(mu_mom=u.reshape(D * K, 2), mu_bound=Lmu.sum(), tau_mom=v.reshape(D * K, 2),
                tau_bound=Ltau.sum(), mu_par=np.stack([m, lam], -1).reshape(D * K, 2),
                tau_par=np.stack([a, b], -1).reshape(D * K, 2))


def tolerances(ld, f64, keys):
    """Per quantity 8 times the largest deviation of the float64 NumPy evaluation (the reference's
    arithmetic) from long double, with a floor of 4 ulp of the quantity's magnitude:
    (allowance, float64 deviation) per quantity."""
    tol, dev = {}, {}
    for key in keys:
        ref = np.asarray(ld[key], dtype=np.longdouble)
        d = float(np.max(np.abs(np.asarray(f64[key], dtype=np.longdouble) - ref))) if ref.size \
            else 0.0
        mag = float(np.max(np.abs(ref))) if ref.size else 0.0
        dev[key] = d
        tol[key] = max(8 * d, 4 * float(np.spacing(mag)))
    return tol, dev


def error(val, ref):
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.max(np.abs(np.asarray(val) - ref))) if ref.size else 0.0


def make_inputs(N, D, K, seed=None):
    """y = unit normals plus per-cluster offsets of a few units; moment tables of plausible
    posteriors (means near the offsets, precisions near one, a few hundred pseudo-observations);
    priors as (D, K) arrays; seeded per shape.  The offset of a cluster is a vector of D normals
    scaled by 3 / sqrt(D), so two centres lie about four units apart at every D: the clusters
    overlap and the responsibilities are soft.  (With 3 units per DIMENSION the wrong clusters of
    a row have r near 1e-200 at D = 70 and Nk . c, sum lse and the softmax are exercised on
    one-hot rows only.)"""
    rs = np.random.RandomState(1000 * K + 10 * D + N if seed is None else seed)
    off = 3.0 * rs.normal(size=(K, D)) / np.sqrt(D)
    z = rs.randint(K, size=N)
    y = rs.normal(size=(N, D)) + off[z]
    m = off.T + 0.1 * rs.normal(size=(D, K))
    lam = rs.gamma(50.0, 2.0, size=(D, K))
    mu_mom = np.stack([m, m * m + 1 / lam], -1).reshape(D * K, 2)
    a = rs.gamma(50.0, 2.0, size=(D, K))
    b = a / rs.gamma(20.0, 0.05, size=(D, K))
    from scipy.special import digamma
    tau_mom = np.stack([a / b, digamma(a) - np.log(b)], -1).reshape(D * K, 2)
    alpha = rs.gamma(5.0, 10.0, size=K)
    elog_pi = digamma(alpha) - digamma(alpha.sum())
    priors = dict(m0=rs.normal(size=(D, K)), beta0=rs.gamma(2.0, 0.5, size=(D, K)) + 0.01,
                  a0=rs.gamma(2.0, 0.5, size=(D, K)) + 0.01, b0=rs.gamma(2.0, 0.5, size=(D, K)) + 0.01)
    return dict(y=y, mu_mom=mu_mom, tau_mom=tau_mom, elog_pi=elog_pi, labels=z.astype(np.int32),
                **priors)


class CPUDGMMKernels(CPUDirichletKernels):
    """Double of DGMMKernels on CPU tensors; ``calls`` lists the entry points in call order."""

    def __init__(self, rt):
        self.rt = rt
        self.calls = []

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def plan(self, N, D, K):
        lib = dgmm_host()
        if K > lib.dgmm_max_k() or D > lib.dgmm_max_d():
            raise NotImplementedError('above the limits')
        return (lib.dgmm_chunk_rows(N, D, K),
                lib.dgmm_chunks(N, D, K) * lib.dgmm_partial_doubles(D, K) + 1024 + 2)

    def tables(self, D, K, mu_mom, tau_mom, elog_pi, h, q, c, gsum=None):
        self.calls.append('tables')
        hh, qq, cc, gg = host_tables(D, K, self._np(mu_mom), self._np(tau_mom), self._np(elog_pi))
        h.numpy()[...] = hh
        q.numpy()[...] = qq
        c.numpy()[...] = cc
        if gsum is not None:
            gsum.numpy()[...] = gg

    def pass_(self, N, D, K, y, labels, h, q, c, ws, S1, S2, Nk, scal, r_out=None):
        self.calls.append('pass' if r_out is None else 'pass_r')
        o = host_pass(N, D, K, y.numpy().reshape(N, D), self._np(labels), h.numpy(), q.numpy(),
                      c.numpy(), r_out is not None)
        S1.numpy()[...] = o['S1']
        S2.numpy()[...] = o['S2']
        Nk.numpy()[...] = o['Nk']
        scal.numpy()[:3] = [o['sum_lse'], o['Nk_c'], o['S_hq']]
        if r_out is not None:
            r_out.numpy()[...] = o['r']

    def update(self, D, K, which, prior_a, prior_b, S1, S2, Nk, other, par, mom, bound):
        self.calls.append('update_mu' if which == 0 else 'update_tau')
        p, m, b = host_update(D, K, which, prior_a.numpy(), prior_b.numpy(), self._np(S1),
                              self._np(S2), self._np(Nk), self._np(other))
        par.numpy()[...] = p
        mom.numpy()[...] = m
        bound.numpy()[...] = b
