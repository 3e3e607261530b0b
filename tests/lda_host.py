"""TEST INFRASTRUCTURE for the fused latent-Dirichlet-allocation block.

* ``lda_host()``: ctypes library of tests/host/lda_host.cpp, built with g++ from csrc/vmp_lda_dev.h
  -- the arithmetic and the order of additions of csrc/vmp_lda.hip.
* ``restate``: a NumPy long-double restatement of the token pass (no chunks, no lane groups).
* ``CPULDAKernels``: the double of the plan's kernel object (inference/plans/lda.py LDAKernels) on
  CPU tensors: the token pass through the host build, the Dirichlet rows and dot products in NumPy /
  SciPy.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np
from scipy import special

from host_build import build_host_library


@functools.lru_cache(None)
def lda_host():
    lib = build_host_library('lda', ['tests/host/lda_host.cpp', 'bayespy_amd/csrc/vmp_lda_dev.h'])
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.lda_group.argtypes = [i32]
    lib.lda_chunk_tokens.argtypes = [i64, i32]
    lib.lda_pass.argtypes = [i64, i64, i32] + [vp] * 14
    lib.lda_pass.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def make_layouts(doc, word, D, V):
    """The two sorted layouts of inference/plans/lda.py as NumPy arrays (+ ``orig``)."""
    doc, word = np.asarray(doc, dtype=np.int64), np.asarray(word, dtype=np.int64)
    order = np.argsort(doc * V + word, kind='stable')
    doc_d, word_d = doc[order], word[order]
    order_w = np.argsort(word_d * D + doc_d, kind='stable')

    def off(ix, m):
        return np.concatenate([[0], np.cumsum(np.bincount(ix, minlength=m))]).astype(np.int64)
    i32 = np.int32
    return dict(doc_d=doc_d.astype(i32), word_d=word_d.astype(i32), doc_off=off(doc, D),
                word_w=word_d[order_w].astype(i32), doc_w=doc_d[order_w].astype(i32),
                pos_w=order_w.astype(i32), word_off=off(word, V)), order.astype(i32)


def host_token_pass(n, D, V, K, lay, labels, et, ebt, phases=7, orig=None, want_phi=False):
    """(Ndk, Nvk, scal[3], lse, phi or None) of the host build."""
    lib = lda_host()
    T = lib.lda_chunk_tokens(n, K)
    nc = (n + T - 1) // T if n else 0
    lse = np.zeros(max(n, 1))
    Ndk, Nvk = np.full((D, K), np.nan), np.full((V, K), np.nan)
    head, tail, cl = np.zeros((max(nc, 1), K)), np.zeros((max(nc, 1), K)), np.zeros(max(nc, 1))
    phi = np.full((n, K), np.nan) if want_phi else None
    et = np.ascontiguousarray(et, dtype=np.float64)
    ebt = None if ebt is None else np.ascontiguousarray(ebt, dtype=np.float64)
    lib.lda_pass(n, D, K, _p(lay['doc_d']), _p(lay['word_d']), _p(lay['doc_off']), None, _p(labels),
                 _p(et), _p(ebt), _p(lse), _p(Ndk), _p(head), _p(tail), _p(cl),
                 _p(orig) if want_phi else None, _p(phi))
    lib.lda_pass(n, V, K, _p(lay['word_w']), _p(lay['doc_w']), _p(lay['word_off']), _p(lay['pos_w']),
                 _p(labels), _p(ebt), _p(et), _p(lse), _p(Nvk), _p(head), _p(tail), _p(cl), None,
                 None)
    with np.errstate(invalid='ignore'):          # 0 * -inf, as on the device
        scal = np.array([cl[:nc].sum(), float(np.sum(Ndk * et)),
                         0.0 if ebt is None else float(np.sum(Nvk * ebt))])
    return Ndk, Nvk, scal, lse[:n], phi


def restate(doc, word, D, V, K, et, ebt):
    """Long-double restatement in the caller's token order: (phi (n, K), lse (n), Ndk, Nvk)."""
    ld = np.longdouble
    doc, word = np.asarray(doc, dtype=np.int64), np.asarray(word, dtype=np.int64)
    logit = np.asarray(et, dtype=ld)[doc] + (0 if ebt is None else np.asarray(ebt, dtype=ld)[word])
    m = logit.max(axis=1, keepdims=True) if len(doc) else np.zeros((0, 1), dtype=ld)
    lse = m[:, 0] + np.log(np.exp(logit - m).sum(axis=1))
    phi = np.exp(logit - lse[:, None])
    Ndk, Nvk = np.zeros((D, K), dtype=ld), np.zeros((V, K), dtype=ld)
    np.add.at(Ndk, doc, phi)
    np.add.at(Nvk, word, phi)
    return phi, lse, Ndk, Nvk


def dirichlet_rows(prior, counts):
    """(alpha, elog, bound) of vmp_lda_dirichlet for rows x cols arrays."""
    alpha = prior + (0.0 if counts is None else counts)
    elog = special.digamma(alpha) - special.digamma(alpha.sum(-1, keepdims=True))

    def g(a):
        return special.gammaln(a.sum(-1)) - special.gammaln(a).sum(-1)
    bound = float(np.sum((prior - alpha) * elog) + np.sum(g(prior) - g(alpha)))
    return alpha, elog, bound


class CPUDirichletKernels:
    """Mixin of the doubles with Dirichlet tables (LDA, Bernoulli mixture, HMM): ``dirichlet`` and
    ``dot`` of a kernels double that has ``calls``."""

    def dirichlet(self, rows, cols, rs, cs, prior, counts, alpha, elog, ws, bound):
        self.calls.append('dirichlet')

        def view(t):
            # element (r, c) at r * rs + c * cs
            return np.lib.stride_tricks.as_strided(t.numpy().reshape(-1), shape=(rows, cols),
                                                   strides=(8 * rs, 8 * cs))
        al, el, b = dirichlet_rows(view(prior), None if counts is None else view(counts))
        view(alpha)[...] = al
        view(elog)[...] = el
        bound.numpy()[...] = b

    def dot(self, m, a, b, ws, out):
        self.calls.append('dot')
        with np.errstate(invalid='ignore'):          # 0 * -inf, as on the device
            out.numpy()[...] = float(np.sum(a.numpy().reshape(-1)[:m] * b.numpy().reshape(-1)[:m]))


class CPULDAKernels(CPUDirichletKernels):
    """Double of LDAKernels on CPU tensors; ``calls`` lists the entry points in call order."""

    def __init__(self, rt):
        self.rt = rt
        self.calls = []

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def plan(self, n, K):
        if K > 64:
            raise NotImplementedError('K above the limit')
        lib = lda_host()
        T = lib.lda_chunk_tokens(n, K)
        nc = (n + T - 1) // T if n else 0
        return lib.lda_group(K), T, nc * (2 * K + 1) + 1024

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
