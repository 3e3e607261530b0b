"""TEST INFRASTRUCTURE for masks on the fused hidden-Markov-model block.

* ``hmmf_masked_host()``: ctypes library of tests/host/hmm_masked_host.cpp, built with g++ from
  csrc/vmp_hmm_fused_dev.h -- the arithmetic and the order of additions of the MASKED instances of
  csrc/vmp_hmm_fused.hip.
* ``restate_masked``: the reference arithmetic (tests/hmm_fused_host.py ``restate``) with the
  emission term zeroed at masked steps and the sums weighted as the reference weights them, in a
  dtype of the caller's choice; y at masked steps is never read.
* ``CPUMaskedHMMKernels``: tests/hmm_fused_host.py's ``CPUHMMKernels`` plus ``pass_masked``.
It lives under tests/ and is never imported by the product."""
import ctypes
import hashlib
import os
import subprocess
import tempfile

import numpy as np

from hmm_fused_host import CPUHMMKernels, features, _lse, _p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'bayespy_amd', 'csrc')
_LIB = []


def hmmf_masked_host():
    if _LIB:
        return _LIB[0]
    srcs = [os.path.join(ROOT, 'tests', 'host', 'hmm_masked_host.cpp'),
            os.path.join(CSRC, 'vmp_hmm_fused_dev.h')]
    h = hashlib.sha256()
    for p in srcs:
        with open(p, 'rb') as f:
            h.update(f.read())
    d = os.path.join(tempfile.gettempdir(), 'bayespy_amd_hmmfm_%s' % h.hexdigest()[:16])
    so = os.path.join(d, 'libhmmf_masked_host.so')
    if not os.path.exists(so):
        os.makedirs(d, exist_ok=True)
        tmp = so + '.%d.tmp' % os.getpid()
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-shared', '-fPIC', '-ffp-contract=off',
                               srcs[0], '-o', tmp])
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.hmmf_pass_masked.argtypes = [i64, i32, i32, i32, vp, vp, i32] + [vp] * 11
    lib.hmmf_pass_masked.restype = None
    _LIB.append(lib)
    return lib


def host_pass_masked(Y, C, la0, lA, mask, labels=None, want=False):
    """tests/hmm_fused_host.py ``host_pass`` with ``mask`` (B, T), 1 = observed, or None."""
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
    hmmf_masked_host().hmmf_pass_masked(
        B, T, D, K, _p(Y), _p(Cc), 0 if Cc is None else Cc.shape[1],
        _p(np.ascontiguousarray(la0, dtype=np.float64)),
        _p(np.ascontiguousarray(lA, dtype=np.float64)), _p(lab), _p(mk), _p(z0sum), _p(xisum),
        _p(Ts), _p(scal), _p(g), _p(z0), _p(zz))
    return dict(z0sum=z0sum, xisum=xisum, T=Ts, logZ=float(scal[0]), ge=float(scal[1]), gamma=g,
                z0=z0, zz=zz)


def restate_masked(Y, C, la0, lA, mask, dtype=np.longdouble):
    """oracle/hmm.py's alpha_beta_recursion on logp0 = la0 + e_0, logP[n] = lA + e_{n+1} with
    e = 0 at the masked steps, in ``dtype``; sum gamma_0, sum xi and sum log Z over the chains with
    an observed step, T and sum gamma . e over the observed steps.  The same keys as
    ``restate``; gamma, z0 and zz of every chain."""
    mask = np.asarray(mask) != 0
    B, T, D = np.shape(Y)
    Y = np.where(mask[..., None], np.asarray(Y, dtype=np.float64), 0.0).astype(dtype)
    la0, lA = np.asarray(la0, dtype=dtype), np.asarray(lA, dtype=dtype)
    K = len(la0)
    if C is None:
        e = np.zeros((B, T, K), dtype=dtype)
    else:
        e = features(Y, dtype) @ np.asarray(C, dtype=dtype).T
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
    ob = mask.any(axis=1)
    gm = gamma * mask[..., None]
    return dict(z0sum=z0[ob].sum(0), xisum=zz[ob].sum((0, 1)), T=np.einsum('btk,btf->kf', gm, Yn),
                logZ=-g[ob].sum(), ge=np.sum(gm * e), gamma=gamma, z0=z0, zz=zz)


PER_CHAIN = ('gamma', 'z0', 'zz')


def compare_masked(got, Y, C, la0, lA, mask, keys=('z0sum', 'xisum', 'T', 'logZ', 'ge'), label='',
                   out=print):
    """The rule of DESIGN 4.14 / 4.15 (tests/hmm_fused_host.py ``compare``): allowance = 8 times
    the float64 deviation of the reference formulas from long double, floor 4 ulp of the
    quantity's magnitude.  gamma, z0 and zz are compared on the chains with an observed step,
    the sums as they are.  Prints the three figures; returns the failures."""
    ld = restate_masked(Y, C, la0, lA, mask)
    f64 = restate_masked(Y, C, la0, lA, mask, np.float64)
    ob = (np.asarray(mask) != 0).any(axis=1)
    bad = []
    for key in keys:
        sel = (lambda a: np.asarray(a)[ob]) if key in PER_CHAIN else np.asarray
        ref = sel(ld[key]).astype(np.longdouble)
        if ref.size == 0:
            continue
        dev = float(np.max(np.abs(sel(f64[key]).astype(np.longdouble) - ref)))
        mag = float(np.max(np.abs(ref)))
        tol = max(8 * dev, 4 * float(np.spacing(mag)))
        err = float(np.max(np.abs(sel(got[key]).astype(np.longdouble) - ref)))
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


class CPUMaskedHMMKernels(CPUHMMKernels):
    """Double of HMMKernels with the masked pass through the host build."""

    def pass_masked(self, B, T, D, K, Y, C, ldc, elog_a0, elog_A, labels, mask, ws, z0sum, xisum,
                    Tstat, scal, gamma=None, z0=None, zz=None):
        self.calls.append('mpass' if gamma is None else 'mpass_out' if zz is not None
                          else 'mpass_gamma')
        assert mask.dtype == self.rt.torch.uint8 and tuple(mask.shape) == (B, T)
        Cn = None if C is None else C.numpy().reshape(-1, ldc)[:K]
        r = host_pass_masked(Y.numpy().reshape(B, T, D), Cn, elog_a0.numpy(), elog_A.numpy(),
                             mask.numpy(), self._np(labels), want=gamma is not None)
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
