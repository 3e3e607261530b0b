"""TEST INFRASTRUCTURE for the fused diagonal-Gaussian-mixture block with missing observations.

* ``dgmmm_host()``: ctypes library of tests/host/dgmm_masked_host.cpp, built with g++ from
  csrc/vmp_dgmm_masked_dev.h -- the arithmetic and the order of additions of
  csrc/vmp_dgmm_masked.hip.
* ``restate_masked_pass`` / ``restate_masked_update``: NumPy restatements in a dtype of the
  caller's choice (no chunks, no tiles, no packed y; the updates and their bound terms in the
  reference's own form, through ``restate_update`` of tests/dgmm_host.py with the per-element count
  M): long double is the yardstick, float64 is the reference's own arithmetic.
* ``CPUDGMMMaskedKernels``: the double of the plan's kernel object
  (inference/plans/dgmm_masked.py MaskedDGMMKernels) on CPU tensors.
* ``build_sanitized_program``: tests/host/dgmm_masked_host_main.cpp as a program of its own.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from host_build import build_host_library, special_functions_text, FLAGS, ROOT
from dgmm_host import CPUDGMMKernels, restate_update, tolerances, error   # noqa: F401

PASS_QUANTITIES = ('r', 'Nk', 'M', 'S1', 'S2', 'sum_lse', 'Nk_c', 'S_hqg')
UPDATE_QUANTITIES = ('mu_mom', 'mu_bound', 'tau_mom', 'tau_bound', 'mu_par', 'tau_par')


@functools.lru_cache(None)
def dgmmm_host():
    lib = build_host_library('dgmm_masked', ['tests/host/dgmm_masked_host.cpp',
                                             'bayespy_amd/csrc/vmp_dgmm_masked_dev.h',
                                             'bayespy_amd/csrc/vmp_dgmm_dev.h'],
                             prelude=special_functions_text())
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    for name in ('dgmmm_chunk_rows', 'dgmmm_chunks'):
        getattr(lib, name).argtypes = [i64, i32, i32]
        getattr(lib, name).restype = i64
    lib.dgmmm_partial_doubles.argtypes = [i32, i32]
    lib.dgmmm_partial_doubles.restype = i64
    lib.dgmmm_pack.argtypes = [i64, i32, vp, vp, vp]
    lib.dgmmm_pack.restype = i64
    lib.dgmmm_tables.argtypes = [i32, i32] + [vp] * 7
    lib.dgmmm_tables.restype = None
    lib.dgmmm_pass.argtypes = [i64, i32, i32] + [vp] * 12
    lib.dgmmm_pass.restype = None
    lib.dgmmm_dots.argtypes = [ctypes.c_double] * 3
    lib.dgmmm_dots.restype = ctypes.c_double
    lib.dgmmm_update.argtypes = [i32, i32, i32] + [vp] * 9
    lib.dgmmm_update.restype = None
    return lib


def build_sanitized_program():
    """tests/host/dgmm_masked_host_main.cpp (which includes the host source) as a stand-alone
    program built with -fsanitize=address,undefined; returns its path."""
    d = tempfile.mkdtemp(prefix='bayespy_amd_dgmmm_san_')
    exe = os.path.join(d, 'dgmm_masked_host_main')
    pre = os.path.join(d, 'prelude.h')
    with open(pre, 'w') as f:
        f.write(special_functions_text())
    flags = [f for f in FLAGS if f not in ('-shared', '-fPIC')]
    subprocess.check_call(['g++'] + flags + ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all', '-include', pre,
                                             os.path.join(ROOT, 'tests/host/dgmm_masked_host_main.cpp'),
                                             '-o', exe])
    return exe


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def host_pack_masked(y, mask):
    """(packed y (N, D), number of observed entries) of the host build."""
    y = _c(y)
    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    N, D = y.shape
    out = np.zeros((N, D))
    count = dgmmm_host().dgmmm_pack(N, D, _p(y), _p(m), _p(out))
    return out, int(count)


def host_tables_masked(D, K, mu_mom, tau_mom, elog_pi):
    """(h, q, g (D, K), c (K)) of the host build; moment tables (D K, 2) or None."""
    h, q, g, c = np.zeros((D, K)), np.zeros((D, K)), np.zeros((D, K)), np.zeros(K)
    bufs = (_c(mu_mom), _c(tau_mom), _c(elog_pi))
    dgmmm_host().dgmmm_tables(D, K, _p(bufs[0]), _p(bufs[1]), _p(bufs[2]), _p(h), _p(q), _p(g),
                              _p(c))
    return h, q, g, c


def host_pass_masked(N, D, K, yp, labels, h, q, g, c, want_r=False):
    """dict of S1, S2, M (D, K), Nk (K), sum_lse, Nk_c, S_hqg, r or None of the host build on the
    packed ``yp``."""
    S1, S2, M = np.zeros((D, K)), np.zeros((D, K)), np.zeros((D, K))
    Nk, scal = np.zeros(K), np.zeros(1)
    r = np.full((N, K), np.nan) if want_r else None
    bufs = (_c(yp), None if labels is None else np.ascontiguousarray(labels, dtype=np.int32),
            _c(h), _c(q), _c(g), _c(c))
    lib = dgmmm_host()
    lib.dgmmm_pass(N, D, K, *[_p(b) for b in bufs], _p(S1), _p(S2), _p(M), _p(Nk), _p(scal), _p(r))
    dots = lib.dgmmm_dots(float(np.sum(S1 * bufs[2])), float(np.sum(S2 * bufs[3])),
                          float(np.sum(M * bufs[4])))
    return dict(S1=S1, S2=S2, M=M, Nk=Nk, sum_lse=float(scal[0]), r=r,
                Nk_c=float(np.sum(Nk * bufs[5])), S_hqg=dots)


def host_update_masked(D, K, which, prior_a, prior_b, S1, S2, M, other):
    """(par (D K, 2), mom (D K, 2), bound) of the host build; statistics None: the prior."""
    par, mom, bound = np.zeros((D * K, 2)), np.zeros((D * K, 2)), np.zeros(1)
    bufs = [_c(np.broadcast_to(prior_a, (D, K))), _c(np.broadcast_to(prior_b, (D, K))), _c(S1),
            _c(S2), _c(M), _c(other)]
    dgmmm_host().dgmmm_update(D, K, which, *[_p(b) for b in bufs], _p(par), _p(mom), _p(bound))
    return par, mom, float(bound[0])


def restate_masked_tables(mu_mom, tau_mom, elog_pi, D, K, dtype=np.longdouble):
    """h, q, g and c = <log pi> less its maximum from the moment tables, in ``dtype``."""
    mu, tau = (np.asarray(a, dtype=dtype).reshape(D, K, 2) for a in (mu_mom, tau_mom))
    h, q = tau[..., 0] * mu[..., 0], -tau[..., 0] / 2
    g = tau[..., 1] / 2 - tau[..., 0] * mu[..., 1] / 2
    c = np.asarray(elog_pi, dtype=dtype)
    return h, q, g, c - c.max()


def restate_masked_pass(y, mask, h, q, g, c, dtype=np.longdouble, labels=None):
    """The masked pass on y (N, D) and mask (N, D) in ``dtype``, the way mixture.py / gaussian.py /
    categorical.py evaluate it (hidden entries of y are not looked at): dict of r (N, K), lse (N),
    Nk, M, S1, S2 (D, K), sum_lse and the dot products of the bound, Nk . c and
    S1 . h + S2 . q + M . g.  Rows with nothing observed keep r = softmax(c) and enter no sum."""
    m = np.asarray(mask) != 0
    yt = np.where(m, np.nan_to_num(np.asarray(y, dtype=np.float64), nan=0.0, posinf=0.0,
                                   neginf=0.0), 0.0).astype(dtype)
    md = m.astype(dtype)
    h, q, g, c = (np.asarray(a, dtype=dtype) for a in (h, q, g, c))
    K = c.shape[0]
    if labels is None:
        logit = c + md @ g + yt @ h + (yt * yt) @ q
        mx = logit.max(axis=1, keepdims=True) if len(yt) else np.zeros((0, 1), dtype=dtype)
        lse = mx[:, 0] + np.log(np.exp(logit - mx).sum(axis=1))
        r = np.exp(logit - lse[:, None])
    else:
        r = np.eye(K, dtype=dtype)[np.asarray(labels)]
        lse = np.zeros(len(yt), dtype=dtype)
    obs = m.any(axis=1)
    ro = r * obs[:, None].astype(dtype)
    Nk, M, S1, S2 = ro.sum(axis=0), md.T @ ro, yt.T @ ro, (yt * yt).T @ ro
    return dict(r=r, lse=lse, Nk=Nk, M=M, S1=S1, S2=S2, sum_lse=(lse * obs).sum(),
                Nk_c=np.sum(Nk * c), S_hqg=np.sum(S1 * h) + np.sum(S2 * q) + np.sum(M * g))


def restate_masked_update(m0, beta0, a0, b0, S1, S2, M, mu_mom, tau_mom, dtype=np.longdouble):
    """``restate_update`` of tests/dgmm_host.py (the reference's own form) with the count of the
    element M (D, K) in the place of N_k: it broadcasts against the (D, K) tables there."""
    return restate_update(m0, beta0, a0, b0, S1, S2, np.asarray(M), mu_mom, tau_mom, dtype=dtype)


def mixed_mask(N, D, seed=0):
    """About 70 % ones with, where the shape has room: row 2 and column 1 of nothing, row 5 fully
    observed (but for column 1) and a hidden entry at column 64 (row 7)."""
    rs = np.random.RandomState(77 + seed + 1000 * D + N)
    m = rs.rand(N, D) < 0.7
    if N > 5:
        m[5] = True
    if N > 2:
        m[2] = False
    if D > 2:
        m[:, 1] = False
    if D > 64 and N > 7:
        m[7, 64] = False
    return m


def junk_at_hidden(y, mask, value):
    """``y`` with ``value`` at the hidden positions."""
    return np.where(np.asarray(mask) != 0, y, value)


class CPUDGMMMaskedKernels(CPUDGMMKernels):
    """Double of MaskedDGMMKernels on CPU tensors."""

    def plan_masked(self, N, D, K):
        lib = dgmmm_host()
        if K > lib.dgmmm_max_k() or D > lib.dgmmm_max_d():
            raise NotImplementedError('above the limits')
        return (lib.dgmmm_chunk_rows(N, D, K),
                lib.dgmmm_chunks(N, D, K) * lib.dgmmm_partial_doubles(D, K) + 1024 + 3)

    def pack_masked(self, N, D, y, mask, out, count):
        self.calls.append('pack_masked')
        yp, n = host_pack_masked(y.numpy().reshape(N, D), mask.numpy().reshape(N, D))
        out.numpy()[...] = yp
        count.numpy()[0] = n

    def tables_masked(self, D, K, mu_mom, tau_mom, elog_pi, h, q, g, c):
        self.calls.append('tables_masked')
        hh, qq, gg, cc = host_tables_masked(D, K, self._np(mu_mom), self._np(tau_mom),
                                            self._np(elog_pi))
        h.numpy()[...] = hh
        q.numpy()[...] = qq
        g.numpy()[...] = gg
        c.numpy()[...] = cc

    def pass_masked(self, N, D, K, y, labels, h, q, g, c, ws, S1, S2, M, Nk, scal, r_out=None):
        self.calls.append('pass_masked' if r_out is None else 'pass_masked_r')
        o = host_pass_masked(N, D, K, y.numpy().reshape(N, D), self._np(labels), h.numpy(),
                             q.numpy(), g.numpy(), c.numpy(), r_out is not None)
        S1.numpy()[...] = o['S1']
        S2.numpy()[...] = o['S2']
        M.numpy()[...] = o['M']
        Nk.numpy()[...] = o['Nk']
        scal.numpy()[:3] = [o['sum_lse'], o['Nk_c'], o['S_hqg']]
        if r_out is not None:
            r_out.numpy()[...] = o['r']

    def update_masked(self, D, K, which, prior_a, prior_b, S1, S2, M, other, par, mom, bound):
        self.calls.append('update_masked_mu' if which == 0 else 'update_masked_tau')
        p, m, b = host_update_masked(D, K, which, prior_a.numpy(), prior_b.numpy(), self._np(S1),
                                     self._np(S2), self._np(M), self._np(other))
        par.numpy()[...] = p
        mom.numpy()[...] = m
        bound.numpy()[...] = b
