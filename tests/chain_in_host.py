"""TEST INFRASTRUCTURE for the GaussianMarkovChain with input signals.

* ``chain_in_host()``: ctypes library of tests/host/chain_in_host.cpp, built with g++ from
  csrc/vmp_chain_in_dev.h -- the arithmetic of csrc/vmp_chain_in.hip.
* ``host_input_stats(x, z, with_zz)``: (Snz, Spz, Szz) of the host build.
* ``reference_input_stats(x, z)``: the same sums in long double, each with its sum of absolute
  terms for the bound.
* ``check_against_long_double(S, x, z)``: the rule of the pair statistics, per element
  |S - ref| <= (ny + 2) 2^-53 sum_b |terms|: one rounding per accumulated term plus the slice
  additions (derived from recursive summation in any fixed order, not measured).
* ``install()``: the NumPy double of the generic entry points (tests/host_generic.py) plus the
  pair-statistics and input-statistics entry points, so that the generic engine runs models with
  driven chains on a CPU.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np

from host_build import build_host_library
import chain_tv_host

U = 2.0 ** -53


@functools.lru_cache(None)
def chain_in_host():
    lib = build_host_library('chain_in', ['tests/host/chain_in_host.cpp',
                                          'bayespy_amd/csrc/vmp_chain_in_dev.h'])
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    lib.chain_in_max_d.restype = i32
    lib.chain_in_max_k.restype = i32
    lib.chain_in_tile.argtypes = [i32, i32]
    lib.chain_in_tile.restype = i32
    lib.chain_in_work_doubles.argtypes = [i64, i32, i32, i32]
    lib.chain_in_work_doubles.restype = i64
    lib.chain_in_nslice.argtypes = [i64, i32, i32, i32]
    lib.chain_in_nslice.restype = i64
    lib.chain_in_input_stats.argtypes = [i64, i64, i32, i32, i32, vp, vp, vp, vp, vp, vp, i64]
    lib.chain_in_input_stats.restype = i32
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_input_stats(x, z, with_zz=True):
    """x (ny, N, D), z (zrows, N-1, K) -> (Snz, Spz, Szz or None)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    z = np.ascontiguousarray(z, dtype=np.float64)
    ny, N, D = x.shape
    zrows, _, K = z.shape
    lib = chain_in_host()
    nw = lib.chain_in_work_doubles(ny, N, D, K)
    Snz, Spz = np.full((N - 1, D, K), np.nan), np.full((N - 1, D, K), np.nan)
    Szz = np.full((N - 1, K, K), np.nan) if with_zz else None
    work = np.empty(max(nw, 1))
    rc = lib.chain_in_input_stats(ny, zrows, N, D, K, _p(x), _p(z), _p(Snz), _p(Spz),
                                  _p(Szz) if with_zz else None, _p(work), nw)
    assert rc == 0, rc
    return Snz, Spz, Szz


def reference_input_stats(x, z):
    """[(sum, sum of |terms|)] for Snz, Spz, Szz in long double, sequence blocks at a time."""
    ny, N, D = x.shape
    zrows, _, K = z.shape
    shapes = [(N - 1, D, K), (N - 1, D, K), (N - 1, K, K)]
    acc = [[np.zeros(s, np.longdouble), np.zeros(s, np.longdouble)] for s in shapes]
    step = max(1, int(2e6 // max(N * max(D, K) * K, 1)))
    for b in range(0, ny, step):
        xl = x[b:b + step].astype(np.longdouble)
        zl = (z[b:b + step] if zrows == ny and ny != 1 else
              np.broadcast_to(z[:1], (xl.shape[0],) + z.shape[1:])).astype(np.longdouble)
        terms = [xl[:, 1:, :, None] * zl[:, :, None, :], xl[:, :-1, :, None] * zl[:, :, None, :],
                 zl[:, :, :, None] * zl[:, :, None, :]]
        for a, p in zip(acc, terms):
            a[0] += p.sum(0)
            a[1] += np.abs(p).sum(0)
    return acc


def check_against_long_double(S, x, z):
    """Every given sum of ``S`` = (Snz, Spz, Szz or None) within (ny + 2) u sum |terms| of the
    long-double sum, and finite."""
    ny = x.shape[0]
    for name, s, (ref, mag) in zip(('Snz', 'Spz', 'Szz'), S, reference_input_stats(x, z)):
        if s is None:
            continue
        assert s.shape == ref.shape, (name, s.shape, ref.shape)
        assert np.all(np.isfinite(s)), name
        excess = np.abs(s - ref) - (ny + 2) * U * mag
        assert np.all(excess <= 0), (name, x.shape, z.shape, float(excess.max()))
        if ny == 0:
            assert not s.any(), name


def make_xz(ny, zrows, N, D, K, scale=1.0, seed=None):
    rs = np.random.RandomState(ny % 1000 + 7 * N + 31 * D + K if seed is None else seed)
    x = scale * rs.normal(size=(ny, N, D)) * np.exp(rs.normal(size=(ny, 1, 1)))
    z = rs.normal(size=(zrows, N - 1, K)) * np.exp(0.5 * rs.normal(size=(zrows, 1, 1)))
    return x, z


def install(enabled=True):
    """A CPU runtime whose library is the generic NumPy double plus the pair- and input-statistics
    entry points; ``lib.input_stats_enabled`` plays the tune key chain_input_stats."""
    import host_generic
    from bayespy_amd import device
    from host_generic import _dense

    class HostChainInLib(host_generic.HostGenericLib):
        input_stats_enabled = bool(enabled)
        pair_stats_enabled = True

        def vmp_tune_set(self, key, value):
            if key == b'chain_input_stats':
                self.input_stats_enabled = bool(value)
            if key == b'chain_pair_stats':
                self.pair_stats_enabled = bool(value)
            return 0

        def vmp_chain_pair_stats_limits(self, ny, N, D, max_d, enabled_, work):
            lib = chain_tv_host.chain_tv_host()
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
            a, b = chain_tv_host.host_pair_stats(_dense(x, (ny, N, D)))
            _dense(Sxx, (N, D, D))[...] = a
            if N > 1:
                _dense(Sxp, (N - 1, D, D))[...] = b
            return 0

        def vmp_chain_input_stats_limits(self, ny, zrows, N, D, K, max_d, max_k, enabled_, work):
            lib = chain_in_host()
            max_d._obj.value = lib.chain_in_max_d()
            max_k._obj.value = lib.chain_in_max_k()
            enabled_._obj.value = int(self.input_stats_enabled)
            work._obj.value = 0
            if D > lib.chain_in_max_d() or K > lib.chain_in_max_k():
                return 3
            work._obj.value = lib.chain_in_work_doubles(int(ny), int(N), int(D), int(K))
            return 0

        def vmp_chain_input_stats(self, ctx, ny, zrows, N, D, K, x, z, Snz, Spz, Szz, work, nwork):
            self._count('vmp_chain_input_stats')
            ny, zrows, N, D, K = int(ny), int(zrows), int(N), int(D), int(K)
            a, b, c = host_input_stats(_dense(x, (ny, N, D)), _dense(z, (zrows, N - 1, K)),
                                       with_zz=Szz is not None)
            _dense(Snz, (N - 1, D, K))[...] = a
            _dense(Spz, (N - 1, D, K))[...] = b
            if Szz is not None:
                _dense(Szz, (N - 1, K, K))[...] = c
            return 0

    rt = device.Runtime(device='cpu')
    rt.lib = HostChainInLib()
    device.set_runtime(rt)
    return rt
