"""TEST INFRASTRUCTURE for the fused Bernoulli-mixture block.

* ``bmm_host()``: ctypes library of tests/host/bmm_host.cpp, built with g++ from csrc/vmp_bmm_dev.h
  -- the arithmetic and the order of additions of csrc/vmp_bmm.hip.
* ``restate``: a NumPy restatement of the pass in a dtype of the caller's choice (no chunks, no
  tiles): long double is the yardstick, float64 is the reference's own arithmetic.
* ``CPUBMMKernels``: the double of the plan's kernel object (inference/plans/bmm.py BMMKernels) on
  CPU tensors: pack, tables and pass through the host build, the Beta / Dirichlet rows and the dot
  products in NumPy / SciPy (tests/lda_host.py).
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np

from host_build import build_host_library
from lda_host import CPUDirichletKernels

DTYPES = {'float64': 0, 'int64': 1, 'bool': 2, 'uint8': 2}


@functools.lru_cache(None)
def bmm_host():
    lib = build_host_library('bmm', ['tests/host/bmm_host.cpp', 'bayespy_amd/csrc/vmp_bmm_dev.h'])
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.bmm_kpad.argtypes = [i32]
    lib.bmm_words.argtypes = [i32]
    for name in ('bmm_chunk_rows', 'bmm_chunks'):
        getattr(lib, name).argtypes = [i64, i32, i32]
        getattr(lib, name).restype = i64
    lib.bmm_partial_doubles.argtypes = [i32, i32]
    lib.bmm_partial_doubles.restype = i64
    lib.bmm_pack.argtypes = [i64, i32, i32, vp, vp]
    lib.bmm_unpack.argtypes = [i64, i32, vp, vp]
    lib.bmm_unpack.restype = None
    lib.bmm_tables.argtypes = [i32, i32, vp, vp, vp, vp]
    lib.bmm_tables.restype = None
    lib.bmm_pass.argtypes = [i64, i32, i32] + [vp] * 9
    lib.bmm_pass.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_pack(x):
    """(words (N, W) uint64, flag) of a 2-D array of dtype float64 / int64 / bool."""
    lib = bmm_host()
    x = np.ascontiguousarray(x)
    N, D = x.shape
    xw = np.zeros((N, lib.bmm_words(D)), dtype=np.uint64)
    flag = lib.bmm_pack(N, D, DTYPES[x.dtype.name], _p(x), _p(xw))
    return xw, flag


def host_unpack(xw, D):
    x = np.zeros((xw.shape[0], D))
    bmm_host().bmm_unpack(xw.shape[0], D, _p(np.ascontiguousarray(xw)), _p(x))
    return x


def host_tables(D, K, elog_p, elog_pi):
    w, c = np.zeros((D, K)), np.zeros(K)
    bmm_host().bmm_tables(D, K, _p(None if elog_p is None else np.ascontiguousarray(elog_p)),
                          _p(np.ascontiguousarray(elog_pi)), _p(w), _p(c))
    return w, c


def host_pass(N, D, K, xw, labels, w, c, want_r=False):
    """(S (D, K), Nk (K), counts (D K, 2), sum lse, r or None) of the host build."""
    S, Nk, counts, scal = np.zeros((D, K)), np.zeros(K), np.zeros((D * K, 2)), np.zeros(1)
    r = np.full((N, K), np.nan) if want_r else None
    bmm_host().bmm_pass(N, D, K, _p(np.ascontiguousarray(xw)), _p(labels),
                        _p(np.ascontiguousarray(w)), _p(np.ascontiguousarray(c)), _p(S), _p(Nk),
                        _p(counts), _p(scal), _p(r))
    return S, Nk, counts, float(scal[0]), r


def restate(x, w, c, dtype=np.longdouble):
    """The pass on dense x (N, D) of zeros and ones, in ``dtype``, the way mixture.py /
    bernoulli.py / categorical.py evaluate it: dict of r (N, K), lse (N), Nk, S (D, K), sum_lse and
    the two dot products of the bound, Nk . c and S . w."""
    x = np.asarray(x, dtype=dtype)
    w, c = np.asarray(w, dtype=dtype), np.asarray(c, dtype=dtype)
    logit = c + x @ w
    m = logit.max(axis=1, keepdims=True) if len(x) else np.zeros((0, 1), dtype=dtype)
    lse = m[:, 0] + np.log(np.exp(logit - m).sum(axis=1))
    r = np.exp(logit - lse[:, None])
    Nk, S = r.sum(axis=0), x.T @ r
    return dict(r=r, lse=lse, Nk=Nk, S=S, sum_lse=lse.sum(), Nk_c=np.sum(Nk * c),
                S_w=np.sum(S * w))


class CPUBMMKernels(CPUDirichletKernels):
    """Double of BMMKernels on CPU tensors; ``calls`` lists the entry points in call order."""

    def __init__(self, rt):
        self.rt = rt
        self.calls = []

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def plan(self, N, D, K):
        if K > 64 or D > 1024:
            raise NotImplementedError('above the limits')
        lib = bmm_host()
        return (lib.bmm_chunk_rows(N, D, K),
                lib.bmm_chunks(N, D, K) * lib.bmm_partial_doubles(D, K) + 1024)

    def pack(self, N, D, dtype, x, xw, flag):
        self.calls.append('pack')
        words, f = host_pack(x.numpy())
        xw.numpy()[:words.size] = words.reshape(-1).view(np.int64)
        flag.numpy()[0] = f

    def tables(self, D, K, elog_p, elog_pi, w, c):
        self.calls.append('tables')
        ww, cc = host_tables(D, K, self._np(elog_p), self._np(elog_pi))
        w.numpy()[...] = ww
        c.numpy()[...] = cc

    def pass_(self, N, D, K, xw, labels, w, c, ws, S, Nk, counts, scal, r_out=None):
        self.calls.append('pass' if r_out is None else 'pass_r')
        W = bmm_host().bmm_words(D)
        words = xw.numpy()[:N * W].view(np.uint64).reshape(N, W)
        s, n, cn, sl, r = host_pass(N, D, K, words, self._np(labels), w.numpy(), c.numpy(),
                                    r_out is not None)
        S.numpy()[...] = s
        Nk.numpy()[...] = n
        counts.numpy()[...] = cn
        scal.numpy()[:3] = [sl, float(np.sum(n * c.numpy())), float(np.sum(s * w.numpy()))]
        if r_out is not None:
            r_out.numpy()[...] = r
