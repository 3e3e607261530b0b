"""TEST INFRASTRUCTURE for the fused Bernoulli-mixture block with missing observations.

* ``bmmm_host()``: ctypes library of tests/host/bmm_masked_host.cpp, built with g++ from
  csrc/vmp_bmm_dev.h -- the arithmetic and the order of additions of the masked pass of
  csrc/vmp_bmm.hip.
* ``restate_masked``: a NumPy restatement of the masked pass in a dtype of the caller's choice (no
  chunks, no tiles, no bit planes): long double is the yardstick, float64 is the reference's own
  arithmetic.
* ``CPUBMMMaskedKernels``: the double of the plan's kernel object (inference/plans/bmm.py
  BMMKernels) on CPU tensors, the unmasked entries from tests/bmm_host.py and the masked ones
  through the host build.
* ``build_sanitized_program``: tests/host/bmm_masked_host_main.cpp as a program of its own.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from host_build import build_host_library, FLAGS, ROOT
from bmm_host import CPUBMMKernels, DTYPES

QUANTITIES = ('r', 'Nk', 'S', 'M', 'sum_lse', 'Nk_c', 'S_w')


@functools.lru_cache(None)
def bmmm_host():
    lib = build_host_library('bmm_masked', ['tests/host/bmm_masked_host.cpp',
                                            'bayespy_amd/csrc/vmp_bmm_dev.h'])
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.bmmm_words.argtypes = [i32]
    for name in ('bmmm_chunk_rows', 'bmmm_chunks'):
        getattr(lib, name).argtypes = [i64, i32, i32]
        getattr(lib, name).restype = i64
    lib.bmmm_partial_doubles.argtypes = [i32, i32]
    lib.bmmm_partial_doubles.restype = i64
    lib.bmmm_pack.argtypes = [i64, i32, i32, vp, vp, vp]
    lib.bmmm_tables.argtypes = [i32, i32, vp, vp, vp, vp, vp]
    lib.bmmm_tables.restype = None
    lib.bmmm_pass.argtypes = [i64, i32, i32] + [vp] * 11
    lib.bmmm_pass.restype = None
    return lib


def build_sanitized_program():
    """tests/host/bmm_masked_host_main.cpp (which includes the host source) as a stand-alone
    program built with -fsanitize=address,undefined; returns its path."""
    d = tempfile.mkdtemp(prefix='bayespy_amd_bmmm_san_')
    exe = os.path.join(d, 'bmm_masked_host_main')
    flags = [f for f in FLAGS if f not in ('-shared', '-fPIC')]
    subprocess.check_call(['g++'] + flags + ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all',
                                             os.path.join(ROOT, 'tests/host/bmm_masked_host_main.cpp'),
                                             '-o', exe])
    return exe


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def host_pack_masked(x, mask):
    """(words (N, 2 W) uint64, flag) of a 2-D array of dtype float64 / int64 / bool and its mask."""
    lib = bmmm_host()
    x = np.ascontiguousarray(x)
    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    N, D = x.shape
    xw = np.zeros((N, 2 * lib.bmmm_words(D)), dtype=np.uint64)
    flag = lib.bmmm_pack(N, D, DTYPES[x.dtype.name], _p(x), _p(m), _p(xw))
    return xw, flag


def host_tables_masked(D, K, elog_p, elog_pi):
    w, l0, c = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K)
    bmmm_host().bmmm_tables(D, K, _p(None if elog_p is None else np.ascontiguousarray(elog_p)),
                            _p(np.ascontiguousarray(elog_pi)), _p(w), _p(l0), _p(c))
    return w, l0, c


def host_pass_masked(N, D, K, xw, labels, w, l0, c, want_r=False):
    """dict of S, M (D, K), Nk (K), counts (D K, 2), sum_lse, r or None of the host build."""
    S, M, Nk = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K)
    counts, scal = np.zeros((D * K, 2)), np.zeros(1)
    r = np.full((N, K), np.nan) if want_r else None
    bmmm_host().bmmm_pass(N, D, K, _p(np.ascontiguousarray(xw)), _p(labels),
                          _p(np.ascontiguousarray(w)), _p(np.ascontiguousarray(l0)),
                          _p(np.ascontiguousarray(c)), _p(S), _p(M), _p(Nk), _p(counts), _p(scal),
                          _p(r))
    return dict(S=S, M=M, Nk=Nk, counts=counts, sum_lse=float(scal[0]), r=r,
                Nk_c=float(np.sum(Nk * c)), S_w=float(np.sum(S * w) + np.sum(M * l0)))


def restate_masked(x, mask, w, l0, c, dtype=np.longdouble):
    """The masked pass on dense x (N, D) and mask (N, D), in ``dtype``, the way mixture.py /
    bernoulli.py / categorical.py evaluate it (hidden entries of x are not looked at): dict of r
    (N, K), lse (N), Nk, S, M (D, K), sum_lse and the dot products of the bound, Nk . c and
    S . w + M . l0.  Rows with nothing observed keep r = softmax(c) and enter no sum."""
    m = (np.asarray(mask) != 0)
    xm = np.where(m, np.nan_to_num(np.asarray(x, dtype=np.float64)), 0.0).astype(dtype)
    md = m.astype(dtype)
    w, l0, c = (np.asarray(a, dtype=dtype) for a in (w, l0, c))
    logit = c + xm @ w + md @ l0
    mx = logit.max(axis=1, keepdims=True) if len(xm) else np.zeros((0, 1), dtype=dtype)
    lse = mx[:, 0] + np.log(np.exp(logit - mx).sum(axis=1))
    r = np.exp(logit - lse[:, None])
    obs = m.any(axis=1)
    ro = r * obs[:, None].astype(dtype)
    Nk, S, M = ro.sum(axis=0), xm.T @ ro, md.T @ ro
    return dict(r=r, lse=lse, Nk=Nk, S=S, M=M, sum_lse=(lse * obs).sum(), Nk_c=np.sum(Nk * c),
                S_w=np.sum(S * w) + np.sum(M * l0))


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
    nothing, row 5 fully observed, column 1 of nothing and hidden bits in the last partial word."""
    m = rs.rand(N, D) < 0.7
    if N > 2:
        m[2] = False
    if N >= 128:
        m[64:128] = False
    if N > 5:
        m[5] = True
    if D > 2:
        m[:, 1] = False
    if D % 64 and N > 7:
        m[7, D - 1] = False
        m[6, 64 * (D // 64):] = False
    return m


class CPUBMMMaskedKernels(CPUBMMKernels):
    """Double of BMMKernels on CPU tensors, masked entries included."""

    def plan_masked(self, N, D, K):
        lib = bmmm_host()
        if K > lib.bmmm_max_k() or D > lib.bmmm_max_d():
            raise NotImplementedError('above the limits')
        return (lib.bmmm_chunk_rows(N, D, K),
                lib.bmmm_chunks(N, D, K) * lib.bmmm_partial_doubles(D, K) + 1024 + 2)

    def pack_masked(self, N, D, dtype, x, mask, xw, flag):
        self.calls.append('pack_masked')
        words, f = host_pack_masked(x.numpy(), mask.numpy())
        xw.numpy()[:words.size] = words.reshape(-1).view(np.int64)
        flag.numpy()[0] = f

    def tables_masked(self, D, K, elog_p, elog_pi, w, l0, c):
        self.calls.append('tables_masked')
        ww, ll, cc = host_tables_masked(D, K, self._np(elog_p), self._np(elog_pi))
        w.numpy()[...] = ww
        l0.numpy()[...] = ll
        c.numpy()[...] = cc

    def pass_masked(self, N, D, K, xw, labels, w, l0, c, ws, S, M, Nk, counts, scal, r_out=None):
        self.calls.append('pass_masked' if r_out is None else 'pass_masked_r')
        W = bmmm_host().bmmm_words(D)
        words = xw.numpy()[:N * 2 * W].view(np.uint64).reshape(N, 2 * W)
        h = host_pass_masked(N, D, K, words, self._np(labels), w.numpy(), l0.numpy(), c.numpy(),
                             r_out is not None)
        S.numpy()[...] = h['S']
        M.numpy()[...] = h['M']
        Nk.numpy()[...] = h['Nk']
        counts.numpy()[...] = h['counts']
        scal.numpy()[:3] = [h['sum_lse'], h['Nk_c'], h['S_w']]
        if r_out is not None:
            r_out.numpy()[...] = h['r']
