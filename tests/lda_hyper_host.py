"""TEST INFRASTRUCTURE for the fused latent-Dirichlet-allocation block with learnt concentrations.

* ``lda_hyper_host()``: ctypes library of tests/host/lda_hyper_host.cpp, built with g++ from
  csrc/vmp_lda_hyper_dev.h -- the layout and the order of additions of csrc/vmp_lda_hyper.hip -- and
  its long-double restatement of S and qterm.
* ``host_stats`` / ``restate`` / ``float64_stats``: the host build, the long-double restatement and
  the plain float64 NumPy + SciPy evaluation of the same formulas; ``compare`` applies the rule of
  DESIGN.md 4.14 (8 x the float64 deviation from long double, floor 4 ulp) and prints the figures.
* ``CPUHyperLDAKernels`` / ``CPUWideHyperLDAKernels``: doubles of the plans' kernel objects
  (inference/plans/lda_hyper.py) on CPU tensors.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np
from scipy import special

from host_build import build_host_library, special_functions_text
from lda_host import CPULDAKernels
from lda_wide_host import CPUWideLDAKernels

MAX_W = 1024


@functools.lru_cache(None)
def lda_hyper_host():
    lib = build_host_library('lda_hyper', ['tests/host/lda_hyper_host.cpp',
                                           'bayespy_amd/csrc/vmp_lda_hyper_dev.h',
                                           'bayespy_amd/csrc/vmp_lda_dev.h'],
                             prelude=special_functions_text())
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.lda_hyper_regs.argtypes = [i32]
    lib.lda_hyper_chunk_rows.argtypes = [i64]
    lib.lda_hyper_ws_doubles.argtypes = [i64, i32]
    lib.lda_hyper_ws_doubles.restype = i64
    lib.lda_hyper_stats.argtypes = [i64, i64, i32, vp, vp, vp, vp]
    lib.lda_hyper_restate.argtypes = [i64, i64, i32, vp, vp, vp, vp]
    lib.lda_hyper_restate.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _memory(x, transposed):
    """A rows x cols array as the flat memory of its form."""
    x = np.asarray(x, dtype=np.float64)
    return np.ascontiguousarray(x.T if transposed else x).reshape(-1)


def host_stats(alpha, elog, transposed):
    """(S, qterm) of the host build for rows x cols arrays."""
    rows, cols = alpha.shape
    S, q = np.full(cols, np.nan), np.full(1, np.nan)
    a, e = _memory(alpha, transposed), _memory(elog, transposed)
    rc = lda_hyper_host().lda_hyper_stats(rows, cols, int(transposed), _p(a), _p(e), _p(S), _p(q))
    assert rc == 0
    return S, q[0]


def restate(alpha, elog):
    """(S, qterm) in long double: plain loops and lgammal."""
    rows, cols = alpha.shape
    S, q = np.zeros(cols, dtype=np.longdouble), np.zeros(1, dtype=np.longdouble)
    a, e = _memory(alpha, False), _memory(elog, False)
    lda_hyper_host().lda_hyper_restate(rows, cols, 0, _p(a), _p(e), _p(S), _p(q))
    return S, q[0]


def float64_stats(alpha, elog):
    """(S, qterm): the plain float64 evaluation of the same formulas (NumPy sums, SciPy gammaln)."""
    with np.errstate(invalid='ignore'):
        S = elog.sum(axis=0) if alpha.shape[0] else np.zeros(alpha.shape[1])
        q = float(np.sum(special.gammaln(alpha.sum(axis=1)) - special.gammaln(alpha).sum(axis=1)
                         + ((alpha - 1.0) * elog).sum(axis=1)))
    return S, q


def compare(got_S, got_q, alpha, elog, label='', out=print):
    """The rule of DESIGN 4.14: per quantity the allowance is 8 times the deviation of the float64
    evaluation from the long-double one, with a floor of 4 ulp of the quantity's magnitude.  Prints
    the three figures per quantity; returns the failures as (key, error, allowance)."""
    rS, rq = restate(alpha, elog)
    fS, fq = float64_stats(alpha, elog)
    bad = []
    for key, got, ref, f64 in (('S', got_S, rS, fS), ('qterm', got_q, rq, fq)):
        ref = np.atleast_1d(np.asarray(ref, dtype=np.longdouble))
        dev = float(np.max(np.abs(np.atleast_1d(f64) - ref)))
        mag = float(np.max(np.abs(ref)))
        tol = max(8 * dev, 4 * float(np.spacing(mag)))
        err = float(np.max(np.abs(np.atleast_1d(np.asarray(got, dtype=np.longdouble)) - ref)))
        out('%s %-5s float64 deviation %.3e  error %.3e  allowance %.3e' % (label, key, dev, err, tol))
        if not err <= tol:
            bad.append((key, err, tol))
    return bad


def make_tables(rs, rows, cols, kind='plain'):
    """(alpha, elog) of rows x cols Dirichlet rows.  'spread': every row's alpha spans 1e-3 .. 1e6."""
    if kind == 'spread':
        alpha = 10.0 ** rs.uniform(-3.0, 6.0, size=(rows, cols))
        if cols >= 2:
            alpha[:, 0], alpha[:, -1] = 1e-3, 1e6
    else:
        alpha = rs.gamma(2.0, 1.5, size=(rows, cols)) + 0.05
    elog = special.digamma(alpha) - special.digamma(alpha.sum(axis=1, keepdims=True))
    return alpha, elog


class _CPUHyperKernels:
    """Mixin of the doubles: the entry points the plans of lda_hyper.py add."""

    @staticmethod
    def _form(rows, cols, rs, cs):
        if cs == 1 and rs == cols and cols <= MAX_W:
            return False
        if rs == 1 and cs == rows and rows <= MAX_W:
            return True
        raise NotImplementedError('strides outside the two forms')

    def stats_ws(self, rows, cols, rs, cs):
        if rows == 0:
            return 1
        tr = self._form(rows, cols, rs, cs)
        return lda_hyper_host().lda_hyper_ws_doubles(cols if tr else rows, rows if tr else cols)

    def stats(self, rows, cols, rs, cs, alpha, elog, ws, S, qterm):
        self.calls.append('stats')
        tr = self._form(rows, cols, rs, cs)
        shape = (cols, rows) if tr else (rows, cols)
        a, e = alpha.numpy().reshape(shape), elog.numpy().reshape(shape)
        s, q = host_stats(a.T if tr else a, e.T if tr else e, tr)
        S.numpy()[...] = s
        qterm.numpy()[...] = q

    def prior_fill(self, rows, cols, rs, cs, a, prior):
        self.calls.append('prior_fill')
        view = np.lib.stride_tricks.as_strided(prior.numpy().reshape(-1), shape=(rows, cols),
                                               strides=(8 * rs, 8 * cs))
        view[...] = a.numpy()[None, :]

    def ml_concentration(self, K, m0, m1, r0, r1, max_iter, alpha, work, z, status):
        from ml_host import host_concentration
        self.calls.append('ml_concentration')
        a, zz, st = host_concentration(m0.numpy().reshape(1, K), m1.numpy().reshape(1),
                                       r0.numpy().reshape(1, K), r1.numpy().reshape(1), max_iter)
        alpha.numpy()[...] = a[0]
        z.numpy()[...] = zz
        status.numpy()[...] = st


class CPUHyperLDAKernels(_CPUHyperKernels, CPULDAKernels):
    pass


class CPUWideHyperLDAKernels(_CPUHyperKernels, CPUWideLDAKernels):
    pass
