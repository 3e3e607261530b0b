"""TEST INFRASTRUCTURE for the wide-topic form of the fused latent-Dirichlet-allocation block.

* ``lda_wide_host()``: ctypes library of tests/host/lda_wide_host.cpp, built with g++ from
  csrc/vmp_lda_wide_dev.h -- the layout and the order of additions of csrc/vmp_lda_wide.hip.
* ``host_token_pass``: both passes of that build with the outputs of ``vmp_lda_wide_token_pass``.
* ``CPUWideLDAKernels``: the double of the plan's kernel object (inference/plans/lda_wide.py
  WideLDAKernels) on CPU tensors; Dirichlet rows and dot products as in tests/lda_host.py.
The long-double restatement (``restate``) and the layouts (``make_layouts``) are those of
tests/lda_host.py: they do not depend on K.  It lives under tests/ and is never imported by the
product."""
import ctypes
import functools

import numpy as np

from host_build import build_host_library
from lda_host import CPUDirichletKernels, _p

MIN_K, MAX_K = 65, 1024


@functools.lru_cache(None)
def lda_wide_host():
    lib = build_host_library('lda_wide', ['tests/host/lda_wide_host.cpp',
                                          'bayespy_amd/csrc/vmp_lda_wide_dev.h',
                                          'bayespy_amd/csrc/vmp_lda_dev.h'])
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.lda_wide_regs.argtypes = [i32]
    lib.lda_wide_chunk_tokens.argtypes = [i64]
    lib.lda_wide_pass.argtypes = [i64, i64, i32] + [vp] * 14
    lib.lda_wide_pass.restype = None
    return lib


def host_token_pass(n, D, V, K, lay, labels, et, ebt, phases=7, orig=None, want_phi=False):
    """(Ndk, Nvk, scal[3], lse, phi or None) of the host build."""
    assert MIN_K <= K <= MAX_K
    lib = lda_wide_host()
    T = lib.lda_wide_chunk_tokens(n)
    nc = (n + T - 1) // T if n else 0
    lse = np.zeros(max(n, 1))
    Ndk, Nvk = np.full((D, K), np.nan), np.full((V, K), np.nan)
    head, tail, cl = np.zeros((max(nc, 1), K)), np.zeros((max(nc, 1), K)), np.zeros(max(nc, 1))
    phi = np.full((n, K), np.nan) if want_phi else None
    et = np.ascontiguousarray(et, dtype=np.float64)
    ebt = None if ebt is None else np.ascontiguousarray(ebt, dtype=np.float64)
    lib.lda_wide_pass(n, D, K, _p(lay['doc_d']), _p(lay['word_d']), _p(lay['doc_off']), None,
                      _p(labels), _p(et), _p(ebt), _p(lse), _p(Ndk), _p(head), _p(tail), _p(cl),
                      _p(orig) if want_phi else None, _p(phi))
    lib.lda_wide_pass(n, V, K, _p(lay['word_w']), _p(lay['doc_w']), _p(lay['word_off']),
                      _p(lay['pos_w']), _p(labels), _p(ebt), _p(et), _p(lse), _p(Nvk), _p(head),
                      _p(tail), _p(cl), None, None)
    with np.errstate(invalid='ignore'):          # 0 * -inf, as on the device
        scal = np.array([cl[:nc].sum(), float(np.sum(Ndk * et)),
                         0.0 if ebt is None else float(np.sum(Nvk * ebt))])
    return Ndk, Nvk, scal, lse[:n], phi


class CPUWideLDAKernels(CPUDirichletKernels):
    """Double of WideLDAKernels on CPU tensors; ``calls`` lists the entry points in call order."""

    def __init__(self, rt):
        self.rt = rt
        self.calls = []

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def plan(self, n, K):
        if not MIN_K <= K <= MAX_K:
            raise NotImplementedError('K outside the limits')
        lib = lda_wide_host()
        T = lib.lda_wide_chunk_tokens(n)
        nc = (n + T - 1) // T if n else 0
        return lib.lda_wide_regs(K), T, nc * (2 * K + 1) + 1024

    def token_pass(self, n, D, V, K, lay, labels, elog_theta, elog_beta_t, phases, lse, ws, Ndk,
                   Nvk, scal, orig=None, phi=None):
        self.calls.append('token_pass' if phi is None else 'token_pass_phi')
        nl = {k: self._np(v) for k, v in lay.items()}
        a, b, s, l, ph = host_token_pass(n, D, V, K, nl, self._np(labels), self._np(elog_theta),
                                         self._np(elog_beta_t), phases, self._np(orig),
                                         phi is not None)
        Ndk.numpy()[...] = a
        Nvk.numpy()[...] = b
        scal.numpy()[:3] = s
        lse.numpy()[:n] = l
        if phi is not None:
            phi.numpy()[...] = ph
