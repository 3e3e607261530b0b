"""TEST INFRASTRUCTURE for the fused hidden-Markov-model block.

* ``hmmf_host()``: ctypes library of tests/host/hmm_fused_host.cpp, built with g++ from
  csrc/vmp_hmm_fused_dev.h -- the arithmetic and the order of additions of csrc/vmp_hmm_fused.hip,
  of its MASKED instances when a mask is given.
* ``restate``: the reference arithmetic in a dtype of the caller's choice: oracle/hmm.py's
  ``alpha_beta_recursion`` on an explicitly built ``logP`` plus the plain sums over its ``zz``;
  long double is the yardstick, float64 is the reference's own arithmetic.  With a mask the
  emission term is zeroed at masked steps and the sums are weighted as the reference weights them;
  y at masked steps is never read.
* ``CPUHMMKernels``: the double of the plan's kernel object (inference/plans/hmm.py HMMKernels) on
  CPU tensors: the pass through the host build, the Dirichlet rows and the dot products in NumPy /
  SciPy (tests/lda_host.py).
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np

from host_build import build_host_library
from lda_host import CPUDirichletKernels
from fake_kernels import CPUGMMKernels


@functools.lru_cache(None)
def hmmf_host():
    lib = build_host_library('hmmf', ['tests/host/hmm_fused_host.cpp',
                                      'bayespy_amd/csrc/vmp_hmm_fused_dev.h'])
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.hmmf_kpad.argtypes = [i32]
    lib.hmmf_max_k.argtypes = lib.hmmf_max_d.argtypes = []
    lib.hmmf_nfeat.argtypes = [i32]
    lib.hmmf_partial_doubles.argtypes = [i32, i32]
    lib.hmmf_partial_doubles.restype = i64
    for name in ('hmmf_chains_per_wg', 'hmmf_wgs', 'hmmf_workspace_doubles'):
        getattr(lib, name).argtypes = [i64, i32, i32, i32]
        getattr(lib, name).restype = i64
    lib.hmmf_pass.argtypes = [i64, i32, i32, i32, vp, vp, i32] + [vp] * 11
    lib.hmmf_pass.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_pass(Y, C, la0, lA, labels=None, want=False, mask=None):
    """dict of z0sum, xisum, T (K, FS), logZ, ge and (want) gamma, z0, zz of the host build;
    ``mask`` (B, T), 1 = observed, or None."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    B, T, D = Y.shape
    K = len(la0)
    z0sum, xisum, Ts, scal = np.zeros(K), np.zeros((K, K)), np.zeros((K, 1 + D + D * D)), np.zeros(2)
    g = np.full((B, T, K), np.nan) if want else None
    z0 = np.full((B, K), np.nan) if want else None
    zz = np.full((B, T - 1, K, K), np.nan) if want else None
    Cc = None if C is None else np.ascontiguousarray(C, dtype=np.float64)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
    mk = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(B, T) != 0,
                                                        dtype=np.uint8)
    hmmf_host().hmmf_pass(B, T, D, K, _p(Y), _p(Cc), 0 if Cc is None else Cc.shape[1],
                          _p(np.ascontiguousarray(la0, dtype=np.float64)),
                          _p(np.ascontiguousarray(lA, dtype=np.float64)), _p(lab), _p(mk),
                          _p(z0sum), _p(xisum), _p(Ts), _p(scal), _p(g), _p(z0), _p(zz))
    return dict(z0sum=z0sum, xisum=xisum, T=Ts, logZ=float(scal[0]), ge=float(scal[1]), gamma=g,
                z0=z0, zz=zz)


def features(Y, dtype):
    """(..., NF) compact features y_a y_b (a <= b), y_d, 1."""
    Y = np.asarray(Y, dtype=dtype)
    D = Y.shape[-1]
    cols = [Y[..., a] * Y[..., b] for a in range(D) for b in range(a, D)]
    cols += [Y[..., d] for d in range(D)] + [np.ones(Y.shape[:-1], dtype=dtype)]
    return np.stack(cols, -1)


def _lse(x, axis):
    m = np.max(x, axis=axis, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        m0 = np.where(np.isfinite(m), m, 0)
        return np.squeeze(m0, axis) + np.log(np.sum(np.exp(x - m0), axis=axis))


def restate(Y, C, la0, lA, dtype=np.longdouble, mask=None):
    """oracle/hmm.py's alpha_beta_recursion on logp0 = la0 + e_0, logP[n] = lA + e_{n+1} in
    ``dtype``, and the plain sums over its zz: the same keys as ``host_pass``.  With ``mask``:
    e = 0 at the masked steps; sum gamma_0, sum xi and sum log Z over the chains with an observed
    step, T and sum gamma . e over the observed steps; gamma, z0 and zz of every chain."""
    if mask is None:
        Y = np.asarray(Y, dtype=dtype)
    else:
        mask = np.asarray(mask) != 0
        Y = np.where(mask[..., None], np.asarray(Y, dtype=np.float64), 0.0).astype(dtype)
    B, T, D = Y.shape
    la0, lA = np.asarray(la0, dtype=dtype), np.asarray(lA, dtype=dtype)
    K = len(la0)
    if C is None:
        e = np.zeros((B, T, K), dtype=dtype)
    else:
        e = features(Y, dtype) @ np.asarray(C, dtype=dtype).T
    if mask is not None:
        e = np.where(mask[..., None], e, np.zeros((), dtype=dtype))
    logp0 = la0 + e[:, 0]
    logP = lA[None, None] + e[:, 1:, None, :]
    N = T - 1
    la = np.empty((B, N, K), dtype=dtype)
    la[:, 0] = logp0
    g = np.zeros(B, dtype=dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        for n in range(N):
            v = la[:, n, :, None] + logP[:, n]
            c = _lse(v.reshape(B, K * K), -1)
            g -= c
            if n + 1 < N:
                la[:, n + 1] = _lse(v - c[:, None, None], -2)
        zz = np.empty((B, N, K, K), dtype=dtype)
        lb = np.zeros((B, K), dtype=dtype)
        for n in range(N - 1, -1, -1):
            w = la[:, n, :, None] + lb[:, None, :] + logP[:, n]
            m = np.max(w.reshape(B, K * K), axis=-1)[:, None, None]
            ex = np.exp(w - m)
            zz[:, n] = ex / np.sum(ex, axis=(-1, -2), keepdims=True)
            if n > 0:
                v = lb[:, None, :] + logP[:, n]
                c = _lse(v.reshape(B, K * K), -1)
                lb = _lse(v - c[:, None, None], -1)
        z0 = np.sum(zz[:, 0], axis=-1)
        z0 = z0 / np.sum(z0, axis=-1, keepdims=True)
    gamma = np.concatenate([z0[:, None], zz.sum(axis=-2)], axis=1)
    Yn = np.concatenate([np.ones((B, T, 1), dtype=dtype), Y,
                         (Y[..., :, None] * Y[..., None, :]).reshape(B, T, D * D)], -1)
    ob, gm = (slice(None), gamma) if mask is None else (mask.any(axis=1), gamma * mask[..., None])
    return dict(z0sum=z0[ob].sum(0), xisum=zz[ob].sum((0, 1)), T=np.einsum('btk,btf->kf', gm, Yn),
                logZ=-g[ob].sum(), ge=np.sum(gm * e), gamma=gamma, z0=z0, zz=zz)


PER_CHAIN = ('gamma', 'z0', 'zz')


def compare(got, Y, C, la0, lA, keys=('z0sum', 'xisum', 'T', 'logZ', 'ge'), label='', out=print,
            mask=None):
    """The rule of DESIGN 4.14 / 4.15: per quantity the allowance is 8 times the largest deviation
    of the float64 evaluation of the reference formulas from the long-double one, with a floor of
    4 ulp of the quantity's magnitude.  With ``mask``, gamma, z0 and zz are compared on the chains
    with an observed step, the sums as they are.  Prints the three figures; returns the failures."""
    ld, f64 = restate(Y, C, la0, lA, mask=mask), restate(Y, C, la0, lA, np.float64, mask=mask)
    ob = None if mask is None else (np.asarray(mask) != 0).any(axis=1)

    def sel(a, key):
        a = np.asarray(a, dtype=np.longdouble)
        return a if ob is None or key not in PER_CHAIN else a[ob]
    bad = []
    for key in keys:
        ref = sel(ld[key], key)
        if ref.size == 0:
            continue
        dev = float(np.max(np.abs(sel(f64[key], key) - ref)))
        mag = float(np.max(np.abs(ref)))
        tol = max(8 * dev, 4 * float(np.spacing(mag)))
        err = float(np.max(np.abs(sel(got[key], key) - ref)))
        out('%s %-6s float64 deviation %.3e  error %.3e  allowance %.3e' % (label, key, dev, err, tol))
        if not err <= tol:
            bad.append((key, err, tol))
    return bad


def mixed_mask(B, T, rs):
    """One mask that mixes, across its chains (cyclically): fully observed, nothing observed, a
    masked first step, a masked last step, a ragged tail and random holes at 50 %."""
    m = np.ones((B, T), dtype=bool)
    for b in range(B):
        kind = b % 6
        if kind == 1:
            m[b] = False
        elif kind == 2:
            m[b, 0] = False
        elif kind == 3:
            m[b, -1] = False
        elif kind == 4:
            m[b, rs.randint(1, T):] = False
        elif kind == 5:
            m[b] = rs.rand(T) < 0.5
    return m


def nan_fill(Y, mask, fill=np.nan):
    return np.where((np.asarray(mask) != 0)[..., None], Y, fill)


class CPUEmissionKernels(CPUGMMKernels):
    """The mixture block's double (tests/fake_kernels.py) for the state of mu and Lambda;
    ``prepare_z`` writes the C table of the state as ``vmp_gmm_prepare_z`` does: row k = the
    coefficients of y_a y_b (a <= b), y_d and 1, the last with the <log pi> slot added."""

    def prepare_z(self, D, K, prior_only, state):
        self.calls.append('prepare_z')
        assert not prior_only
        v = self._v(state, D, K)
        L = v['L']
        c, b = self._coefficients(v, D)
        F2P = int(L.F2P)
        C = v['s'][L.off_C:L.off_C + int(L.KP) * F2P].reshape(int(L.KP), F2P)
        C[:] = 0.0
        for k in range(K):
            f = 0
            for a in range(D):
                for bb in range(a, D):
                    lam = v['Lam'][k]
                    C[k, f] = -0.5 * lam[a, a] if a == bb else -0.5 * (lam[a, bb] + lam[bb, a])
                    f += 1
            C[k, f:f + D] = b[k]
            C[k, f + D] = v['logpi'][k] + c[k]
        C[K:, D * (D + 1) // 2 + D] = -np.inf


class CPUHMMKernels(CPUDirichletKernels):
    """Double of HMMKernels on CPU tensors; ``calls`` lists the entry points in call order."""

    def __init__(self, rt):
        self.rt = rt
        self.calls = []
        self.gmm = CPUEmissionKernels(rt)

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def plan(self, B, T, D, K):
        lib = hmmf_host()
        if K > lib.hmmf_max_k() or D > lib.hmmf_max_d() or T < 2:
            raise NotImplementedError('above the limits')
        return lib.hmmf_chains_per_wg(B, T, D, K), lib.hmmf_workspace_doubles(B, T, D, K)

    def pass_(self, B, T, D, K, Y, C, ldc, elog_a0, elog_A, labels, ws, z0sum, xisum, Tstat, scal,
              gamma=None, z0=None, zz=None, mask=None):
        name = 'pass' if gamma is None else 'pass_out' if zz is not None else 'pass_gamma'
        self.calls.append(name if mask is None else 'm' + name)
        assert mask is None or (mask.dtype == self.rt.torch.uint8 and tuple(mask.shape) == (B, T))
        Cn = None if C is None else C.numpy().reshape(-1, ldc)[:K]
        r = host_pass(Y.numpy().reshape(B, T, D), Cn, elog_a0.numpy(), elog_A.numpy(),
                      self._np(labels), want=gamma is not None, mask=self._np(mask))
        z0sum.numpy()[...] = r['z0sum']
        xisum.numpy()[...] = r['xisum']
        Tstat.numpy()[...] = r['T']
        scal.numpy()[:4] = [r['logZ'], r['ge'], float(np.sum(r['z0sum'] * elog_a0.numpy())),
                            float(np.sum(r['xisum'] * elog_A.numpy()))]
        if gamma is not None:
            gamma.numpy()[...] = r['gamma']
            z0.numpy()[...] = r['z0']
        if zz is not None:
            zz.numpy()[...] = r['zz']
