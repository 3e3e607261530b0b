"""TEST INFRASTRUCTURE for the fused hidden-Markov-model block with categorical emissions.

* ``hmmc_host()``: ctypes library of tests/host/hmm_cat_host.cpp, built with g++ from
  csrc/vmp_hmm_fused_dev.h -- the arithmetic and the order of additions of csrc/vmp_hmm_cat.hip.
* ``restate``: the reference arithmetic in a dtype of the caller's choice: oracle/hmm.py's
  ``alpha_beta_recursion`` on an explicitly built ``logP`` (the recursion of
  tests/hmm_fused_host.py ``restate`` with the emission term looked up in <log P>) plus the plain
  sums over its ``zz``; long double is the yardstick, float64 the reference's own arithmetic.
* ``CPUCatHMMKernels``: the double of the plan's kernel object (inference/plans/hmm_cat.py
  CatHMMKernels) on CPU tensors.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from host_build import build_host_library, ROOT, FLAGS
from hmm_fused_host import _lse, PER_CHAIN
from lda_host import CPUDirichletKernels

SOURCES = ['tests/host/hmm_cat_host.cpp', 'bayespy_amd/csrc/vmp_hmm_fused_dev.h']


@functools.lru_cache(None)
def hmmc_host():
    lib = build_host_library('hmmc', SOURCES)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.hmmc_max_k.argtypes = lib.hmmc_max_m.argtypes = []
    lib.hmmc_partial_doubles.argtypes = [i32, i32]
    lib.hmmc_partial_doubles.restype = i64
    for name in ('hmmc_chains_per_wg', 'hmmc_wgs'):
        getattr(lib, name).argtypes = [i64, i32, i32]
        getattr(lib, name).restype = i64
    lib.hmmc_workspace_doubles.argtypes = [i64, i32, i32, i32]
    lib.hmmc_workspace_doubles.restype = i64
    lib.hmmc_pass.argtypes = [i64, i32, i32, i32] + [vp] * 13
    lib.hmmc_pass.restype = None
    return lib


def build_sanitized_program():
    """tests/host/hmm_cat_host_main.cpp (which includes the host source) as a stand-alone program
    built with -fsanitize=address,undefined; returns its path."""
    d = tempfile.mkdtemp(prefix='bayespy_amd_hmmc_san_')
    exe = os.path.join(d, 'hmm_cat_host_main')
    flags = [f for f in FLAGS if f not in ('-shared', '-fPIC')]
    subprocess.check_call(['g++'] + flags + ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all',
                                             os.path.join(ROOT, 'tests/host/hmm_cat_host_main.cpp'),
                                             '-o', exe])
    return exe


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_pass(y, Pt, la0, lA, labels=None, want=False, mask=None):
    """dict of z0sum, xisum, S (M, K), logZ, ge and (want) gamma, z0, zz of the host build; ``Pt``
    (M, K) word-major, or an integer M for the pass without an emission term; ``mask`` (B, T),
    1 = observed, or None."""
    y = np.ascontiguousarray(y, dtype=np.int32)
    B, T = y.shape
    K = len(la0)
    M = Pt.shape[0] if not isinstance(Pt, int) else Pt
    table = None if isinstance(Pt, int) else np.ascontiguousarray(Pt, dtype=np.float64)
    z0sum, xisum, S, scal = np.zeros(K), np.zeros((K, K)), np.zeros((M, K)), np.zeros(2)
    g = np.full((B, T, K), np.nan) if want else None
    z0 = np.full((B, K), np.nan) if want else None
    zz = np.full((B, T - 1, K, K), np.nan) if want else None
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
    mk = None if mask is None else np.ascontiguousarray(np.asarray(mask).reshape(B, T) != 0,
                                                        dtype=np.uint8)
    hmmc_host().hmmc_pass(B, T, M, K, _p(y), _p(table),
                          _p(np.ascontiguousarray(la0, dtype=np.float64)),
                          _p(np.ascontiguousarray(lA, dtype=np.float64)), _p(lab), _p(mk),
                          _p(z0sum), _p(xisum), _p(S), _p(scal), _p(g), _p(z0), _p(zz))
    return dict(z0sum=z0sum, xisum=xisum, S=S, logZ=float(scal[0]), ge=float(scal[1]), gamma=g,
                z0=z0, zz=zz)


def restate(y, Pt, la0, lA, dtype=np.longdouble, mask=None):
    """oracle/hmm.py's alpha_beta_recursion on logp0 = la0 + e_0, logP[n] = lA + e_{n+1} in
    ``dtype`` with e_t[k] = Pt[y_t, k] (0 at a masked step, whose word is never used; 0 throughout
    for an integer ``Pt`` = M), and the plain sums over its zz: the keys of ``host_pass``.  With
    ``mask``: sum gamma_0, sum xi and sum log Z over the chains with an observed step, S and
    sum gamma . e over the observed steps; gamma, z0 and zz of every chain."""
    y = np.asarray(y)
    B, T = y.shape
    obs = np.ones((B, T), dtype=bool) if mask is None else (np.asarray(mask) != 0)
    la0, lA = np.asarray(la0, dtype=dtype), np.asarray(lA, dtype=dtype)
    K = len(la0)
    M = Pt if isinstance(Pt, int) else Pt.shape[0]
    ys = np.where(obs, y, 0)
    if isinstance(Pt, int):
        e = np.zeros((B, T, K), dtype=dtype)
    else:
        e = np.where(obs[..., None], np.asarray(Pt, dtype=dtype)[ys], np.zeros((), dtype=dtype))
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
    ob = obs.any(axis=1)
    gm = gamma * obs[..., None]
    S = np.zeros((M, K), dtype=dtype)
    np.add.at(S, ys[obs], gm[obs])
    return dict(z0sum=z0[ob].sum(0), xisum=zz[ob].sum((0, 1)), S=S, logZ=-g[ob].sum(),
                ge=np.sum(gm * e), gamma=gamma, z0=z0, zz=zz)


SUMS = ('z0sum', 'xisum', 'S', 'logZ', 'ge')
ALL = SUMS + PER_CHAIN


def compare(got, y, Pt, la0, lA, keys=SUMS, label='', out=print, mask=None):
    """The rule of DESIGN 4.14 / 4.15: per quantity the allowance is 8 times the largest deviation
    of the float64 evaluation of the reference formulas from the long-double one, with a floor of
    4 ulp of the quantity's magnitude.  With ``mask``, gamma, z0 and zz are compared on the chains
    with an observed step.  Prints the three figures; returns the failures."""
    ld, f64 = restate(y, Pt, la0, lA, mask=mask), restate(y, Pt, la0, lA, np.float64, mask=mask)
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


def pass_inputs(B, T, M, K, seed=None):
    """(y (B, T), Pt (M, K), la0, lA): Dirichlet <log> tables and sticky chains."""
    from scipy import special
    rs = np.random.RandomState(B + 3 * T + 5 * M + 7 * K if seed is None else seed)
    alP = rs.gamma(1.0, size=(K, M)) + 0.05
    Pt = (special.digamma(alP) - special.digamma(alP.sum(-1, keepdims=True))).T.copy()
    al0, alA = rs.gamma(1.0, size=K) + 0.05, rs.gamma(1.0, size=(K, K)) + 0.05
    la0 = special.digamma(al0) - special.digamma(al0.sum())
    lA = special.digamma(alA) - special.digamma(alA.sum(-1, keepdims=True))
    return rs.randint(M, size=(B, T)), Pt, la0, lA


class CPUCatHMMKernels(CPUDirichletKernels):
    """Double of CatHMMKernels on CPU tensors; ``calls`` lists the entry points in call order."""

    def __init__(self, rt):
        self.rt = rt
        self.calls = []

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def plan(self, B, T, M, K):
        lib = hmmc_host()
        if K > lib.hmmc_max_k() or M > lib.hmmc_max_m() or T < 2:
            raise NotImplementedError('above the limits')
        return lib.hmmc_chains_per_wg(B, M, K), lib.hmmc_workspace_doubles(B, T, M, K)

    def pass_(self, B, T, M, K, y, elogPt, elog_a0, elog_A, labels, mask, ws, z0sum, xisum, S, scal,
              gamma=None, z0=None, zz=None):
        name = 'pass' if gamma is None else 'pass_out' if zz is not None else 'pass_gamma'
        self.calls.append(name if mask is None else 'm' + name)
        torch = self.rt.torch
        assert y.dtype == torch.int32 and tuple(y.shape) == (B, T)
        assert mask is None or (mask.dtype == torch.uint8 and tuple(mask.shape) == (B, T))
        assert elogPt is None or tuple(elogPt.shape) == (M, K)
        r = host_pass(y.numpy(), M if elogPt is None else elogPt.numpy(), elog_a0.numpy(),
                      elog_A.numpy(), self._np(labels), want=gamma is not None,
                      mask=self._np(mask))
        z0sum.numpy()[...] = r['z0sum']
        xisum.numpy()[...] = r['xisum']
        S.numpy()[...] = r['S']
        scal.numpy()[:4] = [r['logZ'], r['ge'], float(np.sum(r['z0sum'] * elog_a0.numpy())),
                            float(np.sum(r['xisum'] * elog_A.numpy()))]
        if gamma is not None:
            gamma.numpy()[...] = r['gamma']
            z0.numpy()[...] = r['z0']
        if zz is not None:
            zz.numpy()[...] = r['zz']
