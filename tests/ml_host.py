"""TEST INFRASTRUCTURE for the maximum-likelihood nodes (GammaShape, Concentration).

* ``ml_host()``: ctypes library of tests/host/ml_host.cpp, built with g++ from csrc/vmp_ml_dev.h and
  the host+device special functions of csrc/vmp_common.h -- the arithmetic of csrc/vmp_ml.hip.
* ``invpsi`` / ``concentration_fixed_point``: NumPy + SciPy restatements of the reference
  (utils/misc.py:1404-1429, dirichlet.py:284-318) with an iteration count.
* ``install()``: the NumPy double of the generic entry points (tests/host_generic.py) plus the ML
  entry points of this library, so that the generic engine runs models with these nodes on a CPU.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np
from scipy import special

from host_build import build_host_library, special_functions_text



@functools.lru_cache(None)
def ml_host():
    lib = build_host_library('ml', ['tests/host/ml_host.cpp', 'bayespy_amd/csrc/vmp_ml_dev.h'],
                             prelude=special_functions_text())
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.ml_invpsi.argtypes = [i64, vp, vp]
    lib.ml_gamma_shape.argtypes = [i64, vp, vp, vp, vp, vp, vp]
    lib.ml_concentration.argtypes = [i64, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_invpsi(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    ml_host().ml_invpsi(x.size, _p(x), _p(y))
    return y


def host_concentration(m0, m1, r0, r1, max_iter=10000):
    """(alpha, z, status) of the host build; m0, r0: (rows, K), m1, r1: (rows,)."""
    m0 = np.ascontiguousarray(m0, dtype=np.float64)
    rows, K = m0.shape
    m1, r0, r1 = [np.ascontiguousarray(np.broadcast_to(v, s), dtype=np.float64)
                  for v, s in ((m1, (rows,)), (r0, (rows, K)), (r1, (rows,)))]
    a, work, z = np.empty((rows, K)), np.empty((rows, K)), np.empty(rows)
    st = np.zeros(3, dtype=np.int32)
    ml_host().ml_concentration(rows, K, _p(m0), _p(m1), _p(r0), _p(r1), max_iter, _p(a), _p(work),
                               _p(z), _p(st))
    return a, z, st


# -- NumPy restatements of the reference ---------------------------------------------------------
def invpsi(x):
    """utils/misc.py:1404-1429."""
    x = np.asanyarray(x)
    with np.errstate(all='ignore'):
        y = np.where(x >= -2.22, np.exp(x) + 0.5, -1 / (x - special.psi(1)))
        for _ in range(5):
            y = y - (special.psi(y) - x) / special.polygamma(1, y)
    return y


def concentration_fixed_point(m0, m1, r0, r1, max_iter=10000):
    """dirichlet.py:284-318 with an iteration count; raises ValueError on infs like the reference.
    Returns (alpha, iterations, capped)."""
    logp = m0 + r0
    N = m1 + r1
    with np.errstate(all='ignore'):
        mean_logp = logp / N[..., None]
    if np.any(np.isinf(mean_logp)):
        raise ValueError("Cannot estimate DirichletConcentration because of infs.")
    a = np.ones(np.shape(mean_logp))
    da = np.inf
    it = 0
    with np.errstate(all='ignore'):
        while np.any(np.abs(da / a) > 1e-5):
            if it == max_iter:
                return a, it, True
            a_new = invpsi(special.psi(np.sum(a, axis=-1, keepdims=True)) + mean_logp)
            da = a_new - a
            a = a_new
            it += 1
    return a, it, False


# -- the generic engine on the host ---------------------------------------------------------------
def install():
    """A CPU runtime whose library is the generic NumPy double plus the ML entry points."""
    import host_generic
    from bayespy_amd import device
    from host_generic import _dense

    class HostMLLib(host_generic.HostGenericLib):

        def vmp_ml_invpsi(self, ctx, n, x, y):
            self._count('vmp_ml_invpsi')
            n = int(n)
            _dense(y, (n,))[...] = host_invpsi(_dense(x, (n,)))
            return 0

        def vmp_ml_gamma_shape(self, ctx, n, m0, m1, r0, r1, a, lga):
            self._count('vmp_ml_gamma_shape')
            n = int(n)
            ins = [np.ascontiguousarray(_dense(p, (n,))) for p in (m0, m1, r0, r1)]
            oa, ol = np.empty(n), np.empty(n)
            ml_host().ml_gamma_shape(n, *[_p(v) for v in ins], _p(oa), _p(ol))
            _dense(a, (n,))[...] = oa
            _dense(lga, (n,))[...] = ol
            return 0

        def vmp_ml_concentration(self, ctx, rows, K, m0, m1, r0, r1, max_iter, alpha, work, z,
                                 status):
            self._count('vmp_ml_concentration')
            rows, K = int(rows), int(K)
            a, zz, st = host_concentration(_dense(m0, (rows, K)), _dense(m1, (rows,)),
                                           _dense(r0, (rows, K)), _dense(r1, (rows,)),
                                           int(max_iter))
            _dense(alpha, (rows, K))[...] = a
            _dense(z, (rows,))[...] = zz
            _dense(status, (3,), np.int32)[...] = st
            return 0

    rt = device.Runtime(device='cpu')
    rt.lib = HostMLLib()
    device.set_runtime(rt)
    return rt
