"""TEST INFRASTRUCTURE for the time-varying GaussianMarkovChain.

* ``chain_tv_host()``: ctypes library of tests/host/chain_tv_host.cpp, built with g++ from
  csrc/vmp_chain_tv_dev.h -- the arithmetic of csrc/vmp_chain_tv.hip.
* ``host_pair_stats(x)``: (Sxx, Sxp) of the host build.
* ``reference_pair_stats(x)``: the same sums in long double, with sum_b |x_i x_j| for the bound.
* ``install()``: the NumPy double of the generic entry points (tests/host_generic.py) plus
  ``vmp_chain_pair_stats`` / ``vmp_chain_pair_stats_limits`` of this library, so that the generic
  engine runs models with such chains on a CPU.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np

from host_build import build_host_library



@functools.lru_cache(None)
def chain_tv_host():
    lib = build_host_library('chain_tv', ['tests/host/chain_tv_host.cpp',
                                          'bayespy_amd/csrc/vmp_chain_tv_dev.h'])
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.chain_tv_max_d.restype = i32
    lib.chain_tv_work_doubles.argtypes = [i64, i32, i32]
    lib.chain_tv_work_doubles.restype = i64
    lib.chain_tv_nslice.argtypes = [i64, i32, i32]
    lib.chain_tv_nslice.restype = i64
    lib.chain_tv_pair_stats.argtypes = [i64, i32, i32, vp, vp, vp, vp, i64]
    lib.chain_tv_pair_stats.restype = i32
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_pair_stats(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    ny, N, D = x.shape
    lib = chain_tv_host()
    nw = lib.chain_tv_work_doubles(ny, N, D)
    Sxx, Sxp, work = np.empty((N, D, D)), np.empty((max(N - 1, 0), D, D)), np.empty(max(nw, 1))
    rc = lib.chain_tv_pair_stats(ny, N, D, _p(x), _p(Sxx), _p(Sxp), _p(work), nw)
    assert rc == 0, rc
    return Sxx, Sxp


def reference_pair_stats(x):
    """(Sxx, Sxp, sum_b |x_t,i x_t,j|, sum_b |x_t,i x_t+1,j|) in long double, sequence blocks at a
    time (the (ny, N, D, D) array of products is never whole in memory)."""
    ny, N, D = x.shape
    acc = [np.zeros((N, D, D), np.longdouble), np.zeros((max(N - 1, 0), D, D), np.longdouble),
           np.zeros((N, D, D), np.longdouble), np.zeros((max(N - 1, 0), D, D), np.longdouble)]
    step = max(1, int(2e6 // max(N * D * D, 1)))
    for b in range(0, ny, step):
        xl = x[b:b + step].astype(np.longdouble)
        pxx = xl[:, :, :, None] * xl[:, :, None, :]
        pxp = xl[:, :-1, :, None] * xl[:, 1:, None, :]
        acc[0] += pxx.sum(0)
        acc[1] += pxp.sum(0)
        acc[2] += np.abs(pxx).sum(0)
        acc[3] += np.abs(pxp).sum(0)
    return acc


def install(enabled=True):
    """A CPU runtime whose library is the generic NumPy double plus the pair-statistics entry
    points; ``lib.pair_stats_enabled`` plays the tune key chain_pair_stats."""
    import host_generic
    from bayespy_amd import device
    from host_generic import _dense, _ptr

    class HostChainTVLib(host_generic.HostGenericLib):
        pair_stats_enabled = bool(enabled)

        def vmp_tune_set(self, key, value):
            if key == b'chain_pair_stats':
                self.pair_stats_enabled = bool(value)
            return 0

        def vmp_chain_pair_stats_limits(self, ny, N, D, max_d, enabled_, work):
            lib = chain_tv_host()
            max_d._obj.value = lib.chain_tv_max_d()
            enabled_._obj.value = int(self.pair_stats_enabled)
            work._obj.value = 0
            if D > lib.chain_tv_max_d():
                return 3
            work._obj.value = lib.chain_tv_work_doubles(int(ny), int(N), int(D))
            return 0

        def vmp_chain_pair_stats(self, ctx, ny, N, D, x, Sxx, Sxp, work, nwork):
            self._count('vmp_chain_pair_stats')
            ny, N, D = int(ny), int(N), int(D)
            a, b = host_pair_stats(_dense(x, (ny, N, D)))
            _dense(Sxx, (N, D, D))[...] = a
            if N > 1:
                _dense(Sxp, (N - 1, D, D))[...] = b
            return 0

    rt = device.Runtime(device='cpu')
    rt.lib = HostChainTVLib()
    device.set_runtime(rt)
    return rt
