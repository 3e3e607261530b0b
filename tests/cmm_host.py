"""TEST INFRASTRUCTURE for the fused categorical-mixture block.

* ``cmm_host()``: ctypes library of tests/host/cmm_host.cpp, built with g++ from csrc/vmp_cmm_dev.h
  -- the arithmetic and the order of additions of csrc/vmp_cmm.hip.
* ``restate`` / ``restate_pack`` / ``restate_tables``: NumPy restatements of pack, tables, pass and
  combine in a dtype of the caller's choice (no chunks, no tiles, no bytes): long double is the
  yardstick, float64 is the reference's own arithmetic.
* ``CPUCMMKernels``: the double of the plan's kernel object (inference/plans/cmm.py CMMKernels) on
  CPU tensors through the host build; Dirichlet rows and dot products in NumPy / SciPy.
* ``build_sanitized_program``: tests/host/cmm_host_main.cpp as a program of its own.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from host_build import build_host_library, FLAGS, ROOT
from lda_host import CPUDirichletKernels

DTYPES = {'float64': 0, 'int64': 1, 'uint8': 2, 'int32': 3}
HIDDEN = 255
QUANTITIES = ('r', 'Nk', 'S', 'sum_lse', 'Nk_c', 'S_L')


@functools.lru_cache(None)
def cmm_host():
    lib = build_host_library('cmm', ['tests/host/cmm_host.cpp', 'bayespy_amd/csrc/vmp_cmm_dev.h'])
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.cmm_kpad.argtypes = [i32]
    lib.cmm_supported.argtypes = [i32, i32, i32]
    for name in ('cmm_cells', 'cmm_lds_bytes', 'cmm_partial_doubles'):
        getattr(lib, name).argtypes = [i32, i32, i32]
        getattr(lib, name).restype = i64
    for name in ('cmm_chunk_rows', 'cmm_chunks'):
        getattr(lib, name).argtypes = [i64, i32, i32, i32]
        getattr(lib, name).restype = i64
    lib.cmm_pack.argtypes = [i64, i32, i32, i32, vp, vp, vp]
    lib.cmm_tables.argtypes = [i32, i32, i32, vp, vp, vp, vp]
    lib.cmm_tables.restype = None
    lib.cmm_pass.argtypes = [i64, i32, i32, i32] + [vp] * 8
    lib.cmm_pass.restype = None
    return lib


def build_sanitized_program():
    """tests/host/cmm_host_main.cpp (which includes the host source) as a stand-alone program built
    with -fsanitize=address,undefined; returns its path."""
    d = tempfile.mkdtemp(prefix='bayespy_amd_cmm_san_')
    exe = os.path.join(d, 'cmm_host_main')
    flags = [f for f in FLAGS if f not in ('-shared', '-fPIC')]
    subprocess.check_call(['g++'] + flags + ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all',
                                             os.path.join(ROOT, 'tests/host/cmm_host_main.cpp'),
                                             '-o', exe])
    return exe


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_pack(x, M, mask=None):
    """(bytes (N, D) uint8, flag) of a 2-D array of dtype float64 / int64 / int32 / uint8."""
    x = np.ascontiguousarray(x)
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    N, D = x.shape
    xb = np.zeros((N, D), dtype=np.uint8)
    flag = cmm_host().cmm_pack(N, D, M, DTYPES[x.dtype.name], _p(x), _p(m), _p(xb))
    return xb, flag


def host_tables(D, K, M, elog_p, elog_pi):
    L, c = np.zeros((M, D * K)), np.zeros(K)
    cmm_host().cmm_tables(D, K, M, _p(None if elog_p is None else np.ascontiguousarray(elog_p)),
                          _p(np.ascontiguousarray(elog_pi)), _p(L), _p(c))
    return L, c


def host_pass(N, D, K, M, xb, labels, L, c, want_r=False):
    """dict of S (M, D, K), Nk (K), sum_lse, Nk_c, S_L, r or None of the host build."""
    S, Nk, scal = np.zeros((M, D, K)), np.zeros(K), np.zeros(1)
    r = np.full((N, K), np.nan) if want_r else None
    L, c = np.ascontiguousarray(L), np.ascontiguousarray(c)
    cmm_host().cmm_pass(N, D, K, M, _p(np.ascontiguousarray(xb)),
                        _p(None if labels is None else np.ascontiguousarray(labels, np.int32)),
                        _p(L), _p(c), _p(S), _p(Nk), _p(scal), _p(r))
    return dict(S=S, Nk=Nk, sum_lse=float(scal[0]), r=r, Nk_c=float(np.sum(Nk * c)),
                S_L=float(np.sum(S.reshape(-1) * L.reshape(-1))))


def restate_pack(x, M, mask=None):
    """(bytes, flag) the way the entry point is documented, in NumPy."""
    x = np.asarray(x)
    seen = np.ones(x.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(invalid='ignore'):
        xf = x.astype(np.float64)
        ok = (xf >= 0) & (xf < M) & (xf == np.floor(xf))
    xb = np.where(seen & ok, np.where(ok, xf, 0), HIDDEN).astype(np.uint8)
    return xb, int(np.any(seen & ~ok))


def restate_tables(elog_p, elog_pi, shape):
    L = np.zeros(shape) if elog_p is None else np.array(elog_p, dtype=np.float64).reshape(shape)
    return L, np.asarray(elog_pi) - np.max(elog_pi)


def restate(x, mask, L, c, dtype=np.longdouble):
    """The pass on dense x (N, D) and mask (N, D) or None, with L (M, D, K) and c (K), in
    ``dtype``, the way mixture.py / categorical.py evaluate it (hidden entries of x are not looked
    at): dict of r (N, K), lse (N), Nk, S (M, D, K), sum_lse and the dot products of the bound.
    Rows with nothing observed keep r = softmax(c) and enter no sum."""
    N, D = np.shape(x)
    M, _, K = np.shape(L)
    m = np.ones((N, D), dtype=bool) if mask is None else (np.asarray(mask) != 0)
    with np.errstate(invalid='ignore'):
        xi = np.where(m, np.nan_to_num(np.asarray(x, dtype=np.float64), posinf=0, neginf=0), 0)
    xi = xi.astype(np.int64).clip(0, M - 1)
    L, c = np.asarray(L, dtype=dtype), np.asarray(c, dtype=dtype)
    md = m.astype(dtype)
    # (N, D, K): <log P>[x_nd, d, :]
    picked = L[xi, np.arange(D)[None, :], :] * md[:, :, None]
    logit = c + picked.sum(axis=1)
    mx = logit.max(axis=1, keepdims=True) if N else np.zeros((0, 1), dtype=dtype)
    lse = mx[:, 0] + np.log(np.exp(logit - mx).sum(axis=1))
    r = np.exp(logit - lse[:, None])
    obs = m.any(axis=1)
    ro = r * obs[:, None].astype(dtype)
    onehot = (xi[:, :, None] == np.arange(M)) & m[:, :, None]          # (N, D, M)
    S = np.einsum('ndm,nk->mdk', onehot.astype(dtype), ro)
    Nk = ro.sum(axis=0)
    return dict(r=r, lse=lse, Nk=Nk, S=S, sum_lse=(lse * obs).sum(), Nk_c=np.sum(Nk * c),
                S_L=np.sum(S * L))


def tolerances(ld, f64):
    """Per quantity 8 times the largest deviation of the float64 NumPy evaluation (the reference's
    arithmetic) from long double, with a floor of 4 ulp of the quantity's magnitude:
    (allowance, float64 deviation) per quantity."""
    tol, dev = {}, {}
    for key in QUANTITIES:
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


def mixed_mask(N, D, rs):
    """Random 70 % with, where the shape has room: row 2 of nothing, the 64-row tile 64 .. 127 of
    nothing, row 5 fully observed and column 1 of nothing (the mask of fixture (f), at any size)."""
    m = rs.rand(N, D) < 0.7
    if N > 2:
        m[2] = False
    if N >= 128:
        m[64:128] = False
    if N > 5:
        m[5] = True
    if D > 2:
        m[:, 1] = False
    return m


def pass_inputs(N, D, K, M):
    """x (N, D) int64, L (M, D, K), c (K) with SOFT rows: the log-probabilities are drawn close to
    each other (scale 0.3 / sqrt(D)), so that r is nowhere near one-hot."""
    rs = np.random.RandomState(100000 * M + 1000 * K + 10 * D + N)
    x = rs.randint(M, size=(N, D)).astype(np.int64)
    p = np.exp(rs.normal(scale=0.3 / np.sqrt(D), size=(M, D, K)))
    L = np.log(p / p.sum(axis=0, keepdims=True))
    c = rs.normal(scale=0.3, size=K)
    return x, L, c - c.max(), rs


class CPUCMMKernels(CPUDirichletKernels):
    """Double of CMMKernels on CPU tensors; ``calls`` lists the entry points in call order."""

    def __init__(self, rt):
        self.rt = rt
        self.calls = []

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def plan(self, N, D, K, M):
        lib = cmm_host()
        if not lib.cmm_supported(D, K, M):
            raise NotImplementedError('above the limits')
        return (lib.cmm_chunk_rows(N, D, K, M),
                lib.cmm_chunks(N, D, K, M) * lib.cmm_partial_doubles(D, K, M) + 1024)

    def pack(self, N, D, M, dtype, x, mask, xb, flag):
        self.calls.append('pack')
        b, f = host_pack(x.numpy(), M, self._np(mask))
        xb.numpy()[:b.size] = b.reshape(-1)
        flag.numpy()[0] = f

    def tables(self, D, K, M, elog_p, elog_pi, L, c):
        self.calls.append('tables')
        ll, cc = host_tables(D, K, M, self._np(elog_p), self._np(elog_pi))
        L.numpy()[...] = ll
        c.numpy()[...] = cc

    def pass_(self, N, D, K, M, xb, labels, L, c, ws, S, Nk, scal, r_out=None):
        self.calls.append('pass' if r_out is None else 'pass_r')
        h = host_pass(N, D, K, M, xb.numpy()[:N * D].reshape(N, D), self._np(labels), L.numpy(),
                      c.numpy(), r_out is not None)
        S.numpy()[...] = h['S'].reshape(M, D * K)
        Nk.numpy()[...] = h['Nk']
        scal.numpy()[:3] = [h['sum_lse'], h['Nk_c'], h['S_L']]
        if r_out is not None:
            r_out.numpy()[...] = h['r']
