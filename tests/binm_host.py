"""TEST INFRASTRUCTURE for the fused binomial-mixture block.

* ``binm_host()``: ctypes library of tests/host/binm_host.cpp, built with g++ from
  csrc/vmp_binm_dev.h -- the arithmetic and the order of additions of csrc/vmp_binm.hip.  The
  one-plane form is the Poisson pass and runs on tests/pmm_host.py's library.
* ``restate_pack`` / ``restate_tables`` / ``restate_pass``: NumPy restatements in a dtype of the
  caller's choice (no chunks, no tiles, no 16-bit planes): long double is the yardstick, float64 is
  the reference's own arithmetic.
* ``CPUBINMKernels``: the double of the plan's kernel object (inference/plans/binm.py BINMKernels)
  on CPU tensors through the host build; Dirichlet rows and dot products in NumPy / SciPy.
* ``build_sanitized_program``: tests/host/binm_host_main.cpp as a program of its own.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from host_build import build_host_library, special_functions_text, FLAGS, ROOT
from lda_host import CPUDirichletKernels
from dgmm_host import _special, tolerances, error            # noqa: F401
import pmm_host as _pmm

DTYPES = {'float64': 0, 'int64': 1, 'uint8': 2, 'int32': 3}
HIDDEN = 0xFFFF
MAX_TRIALS = 65534
PASS_QUANTITIES = ('r', 'Nk', 'S', 'T', 'counts', 'sum_lse', 'Nk_c', 'dots')
HEADERS = ['bayespy_amd/csrc/vmp_binm_dev.h'] + _pmm.HEADERS


@functools.lru_cache(None)
def binm_host():
    lib = build_host_library('binm', ['tests/host/binm_host.cpp'] + HEADERS,
                             prelude=special_functions_text())
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    for name in ('binm_chunk_rows', 'binm_workspace_doubles'):
        getattr(lib, name).argtypes = [i64, i32, i32]
        getattr(lib, name).restype = i64
    lib.binm_pack.argtypes = [i64, i32, i32, vp, vp, i64, i64] + [vp] * 6
    lib.binm_pack.restype = None
    lib.binm_tables.argtypes = [i32, i32, i32] + [vp] * 7
    lib.binm_tables.restype = None
    lib.binm_pass.argtypes = [i64, i32, i32] + [vp] * 12
    lib.binm_pass.restype = None
    lib.binm_const.argtypes = [i32, i32] + [vp] * 5
    lib.binm_const.restype = None
    lib.binm_dots.argtypes = [i32] + [vp] * 4
    lib.binm_dots.restype = ctypes.c_double
    return lib


def build_sanitized_program():
    """tests/host/binm_host_main.cpp (which includes the host sources) as a stand-alone program
    built with -fsanitize=address,undefined; returns its path."""
    d = tempfile.mkdtemp(prefix='bayespy_amd_binm_san_')
    exe = os.path.join(d, 'binm_host_main')
    pre = os.path.join(d, 'prelude.h')
    with open(pre, 'w') as f:
        f.write(special_functions_text())
    flags = [f for f in FLAGS if f not in ('-shared', '-fPIC')]
    subprocess.check_call(['g++'] + flags + ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all', '-include', pre,
                                             os.path.join(ROOT, 'tests/host/binm_host_main.cpp'),
                                             '-o', exe])
    return exe


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def trials_strides(n, N, D):
    """``n`` (a scalar, (D, 1), (N, 1, 1) or (N, D, 1)) without its cluster axis as a contiguous
    int64 array and its element strides (along N, along D)."""
    t = np.asarray(n, dtype=np.int64)
    t = np.ascontiguousarray(t.reshape((1,) * (3 - t.ndim) + t.shape)[..., 0])
    assert t.shape[0] in (1, N) and t.shape[1] in (1, D)
    return t, (t.shape[1] if t.shape[0] > 1 else 0), (1 if t.shape[1] > 1 else 0)


def dense_trials(n, N, D):
    t = trials_strides(n, N, D)[0]
    return np.broadcast_to(t, (N, D))


def host_pack(x, n, mask=None, strides=None):
    """dict of xp, np (N, D) uint16, flags (4), n_observed, n_hidden, constant, lcoef of a 2-D
    array of dtype float64 / int64 / int32 / uint8 and trials that broadcast to (N, D, 1) (or, with
    ``strides``, an int64 buffer read with these element strides)."""
    x = np.ascontiguousarray(x)
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    N, D = x.shape
    if strides is None:
        t, ts_n, ts_d = trials_strides(n, N, D)
    else:
        t, (ts_n, ts_d) = np.ascontiguousarray(n, dtype=np.int64), strides
    xp, np_ = np.zeros((N, D), dtype=np.uint16), np.zeros((N, D), dtype=np.uint16)
    flags, counts, lcoef = np.zeros(4, dtype=np.int32), np.zeros(3, dtype=np.int64), np.zeros(1)
    binm_host().binm_pack(N, D, DTYPES[x.dtype.name], _p(x), _p(t), ts_n, ts_d, _p(m), _p(xp),
                          _p(np_), _p(flags), _p(counts), _p(lcoef))
    return dict(xp=xp, np=np_, flags=flags, n_observed=int(counts[0]), n_hidden=int(counts[1]),
                constant=int(counts[2]), lcoef=float(lcoef[0]))


def host_tables(D, K, form, elog_p, elog_pi, ncol=None):
    """(l1, l0 (D, K), c (K), cfold (K) or None) of the host build; elog_p (D K, 2) or None."""
    l1, l0, c = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K)
    cf = None if ncol is None else np.zeros(K)
    bufs = (_c(elog_p), _c(elog_pi), _c(ncol))
    binm_host().binm_tables(D, K, form, *[_p(b) for b in bufs], _p(l1), _p(l0), _p(c), _p(cf))
    return l1, l0, c, cf


def host_pass(N, D, K, one_plane, xp, np_, ncol, labels, l1, l0, c, want_r=False):
    """dict of S, T (D, K), Nk (K), counts (D K, 2), sum_lse, Nk_c, dots (scal[2]), r or None of
    the host build on the packed planes; ``c`` is cfold in the one-plane form."""
    S, T, Nk = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K)
    counts, scal = np.zeros((D * K, 2)), np.zeros(2)
    r = np.full((N, K), np.nan) if want_r else None
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
    xp = np.ascontiguousarray(xp, dtype=np.uint16)
    l1, l0, c = _c(l1), _c(l0), _c(c)
    lib = binm_host()
    if one_plane:
        ncol = _c(ncol)
        _pmm.pmm_host().pmm_pass(N, D, K, 0, _p(xp), _p(lab), _p(l1), _p(l0), _p(c), _p(S), None,
                                 _p(Nk), _p(scal), _p(r))
        lib.binm_const(D, K, _p(ncol), _p(S), _p(Nk), _p(T), _p(counts))
        dots = float(np.sum(S * l1))
    else:
        np_ = np.ascontiguousarray(np_, dtype=np.uint16)
        lib.binm_pass(N, D, K, _p(xp), _p(np_), _p(lab), _p(l1), _p(l0), _p(c), _p(S), _p(T),
                      _p(Nk), _p(counts), _p(scal), _p(r))
        # formed row by row inside the pass; under fixed labels from S and T
        dots = float(scal[1]) if lab is None else lib.binm_dots(D * K, _p(S), _p(l1), _p(T), _p(l0))
    return dict(S=S, T=T, Nk=Nk, counts=counts, sum_lse=float(scal[0]), r=r,
                Nk_c=float(np.sum(Nk * c)), dots=dots)


# -- restatements ------------------------------------------------------------------------------------
def restate_pack(x, n, mask=None, dtype=np.longdouble):
    """The pack the way the entry point is documented, in NumPy: dict of xp, np, flags, n_observed,
    n_hidden, constant and lcoef = sum over the observed entries of the log binomial coefficient in
    ``dtype``."""
    x = np.asarray(x)
    N, D = x.shape
    nd = dense_trials(n, N, D)
    seen = np.ones(x.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(invalid='ignore'):
        xf = x.astype(np.float64)
        whole = xf == np.floor(xf)
        nonneg = xf >= 0
        tfit = nd <= MAX_TRIALS
        within = (nd >= 0) & (xf <= nd)
    ok = whole & nonneg & tfit & within
    obs = seen & ok
    xp = np.where(obs, np.where(ok, xf, 0), 0).astype(np.uint16)
    np_ = np.where(obs, np.where(ok, nd, 0), HIDDEN).astype(np.uint16)
    flags = np.array([np.any(seen & whole & ~nonneg), np.any(seen & ~whole),
                      np.any(seen & whole & nonneg & tfit & ~within),
                      np.any(seen & whole & nonneg & ~tfit)], dtype=np.int32)
    lgamma = _special(dtype)[1]
    xo, no = xp[obs].astype(np.float64), np_[obs].astype(np.float64)
    if dtype == np.float64:                 # the reference: gammaln of every entry, then the sum
        lcoef = float(np.sum(lgamma(no + 1.0) - lgamma(xo + 1.0) - lgamma(no - xo + 1.0)))
    else:                                   # one evaluation per distinct argument
        vals = np.unique(np.concatenate([no, xo, no - xo]))
        table = dict(zip(vals.tolist(), np.asarray(lgamma(vals + 1.0), dtype=dtype))) \
            if vals.size else {}
        look = lambda a: np.array([table[v] for v in a.tolist()], dtype=dtype)    # noqa: E731
        lcoef = np.sum(look(no) - look(xo) - look(no - xo)) if xo.size else dtype(0)
    return dict(xp=xp, np=np_, flags=flags, n_observed=int(obs.sum()),
                n_hidden=int(obs.size - obs.sum()), constant=int(np.all(nd == nd[:1])) if N else 1,
                lcoef=lcoef)


def restate_tables(elog_p, elog_pi, D, K, form, ncol=None, dtype=np.longdouble):
    """l1, l0, c and cfold (None without ncol) from elog_p (None: zeros), in ``dtype``."""
    e = np.zeros((D, K, 2), dtype=dtype) if elog_p is None \
        else np.asarray(elog_p, dtype=dtype).reshape(D, K, 2)
    l1, l0 = e[..., 0] - e[..., 1], e[..., 1]
    if form & 1:                                        # centred: column 0 of every row taken out
        l1, l0 = l1 - l1[:, :1], l0 - l0[:, :1]
    c = np.asarray(elog_pi, dtype=dtype)
    cf = None
    if ncol is not None:
        cf = c + np.asarray(ncol, dtype=dtype) @ l0
        cf = cf - cf.max()
    return l1, l0, c - c.max(), cf


def restate_pass(x, n, mask, l1, l0, c, one_plane=0, dtype=np.longdouble, labels=None):
    """The pass on dense x, trials that broadcast to (N, D, 1) and mask (N, D) or None in ``dtype``,
    the way mixture.py / binomial.py / categorical.py evaluate it (hidden entries are not looked
    at): dict of r (N, K), Nk, S, T, counts, sum_lse and the dot products of the bound.  ``c`` is
    cfold in the one-plane form, whose logits leave n l0 out.  Rows with nothing observed keep
    r = softmax(c) and enter no sum."""
    x = np.asarray(x)
    N, D = x.shape
    m = np.ones(x.shape, dtype=bool) if mask is None else (np.asarray(mask) != 0)
    xt = np.where(m, np.nan_to_num(np.asarray(x, dtype=np.float64), nan=0.0, posinf=0.0,
                                   neginf=0.0), 0.0).astype(dtype)
    nt = np.where(m, dense_trials(n, N, D), 0).astype(dtype)
    l1, l0, c = (np.asarray(a, dtype=dtype) for a in (l1, l0, c))
    K = c.shape[0]
    if labels is None:
        logit = c + xt @ l1 + (0 if one_plane else nt @ l0)
        mx = logit.max(axis=1, keepdims=True) if N else np.zeros((0, 1), dtype=dtype)
        lse = mx[:, 0] + np.log(np.exp(logit - mx).sum(axis=1))
        r = np.exp(logit - lse[:, None])
    else:
        r = np.eye(K, dtype=dtype)[np.asarray(labels)]
        lse = np.zeros(N, dtype=dtype)
    obs = m.any(axis=1)
    ro = r * obs[:, None].astype(dtype)
    Nk, T, S = ro.sum(axis=0), nt.T @ ro, xt.T @ ro
    return dict(r=r, lse=lse, Nk=Nk, T=T, S=S, counts=np.stack([S, T - S], -1).reshape(D * K, 2),
                sum_lse=(lse * obs).sum(), Nk_c=np.sum(Nk * c),
                dots=np.sum(S * l1) + (0 if one_plane else np.sum(T * l0)))


# -- inputs ------------------------------------------------------------------------------------------
EPS = 0.3


def pass_inputs(N, D, K, kind='entry', top=40):
    """Counts x (N, D) int64 out of trials with SOFT rows: the log-odds of (d, k) are those of the
    column plus eps of scale EPS / sqrt(D top), so the clusters' log-odds of a row are of order one
    at every D.  ``kind``: 'entry' trials (N, D, 1) with zeros and, where there is room, the cap;
    'column' trials (D, 1); 'scalar'.  Also the <log> table (D K, 2) of a plausible Beta posterior
    around those probabilities, <log pi>, labels and the random state."""
    from scipy.special import digamma
    rs = np.random.RandomState(1000 * K + 10 * D + N)
    base = rs.normal(scale=1.0, size=(D, 1))
    eta = base + rs.normal(scale=EPS / np.sqrt(D * top / 4.0), size=(D, K))
    p = 1.0 / (1.0 + np.exp(-eta))
    if kind == 'entry':
        n = rs.randint(0, top + 1, size=(N, D, 1))
        if N > 9 and D > 2:
            n[9, 2, 0] = MAX_TRIALS
            n[8, :, 0] = 0
    elif kind == 'column':
        n = rs.randint(1, top + 1, size=(D, 1))
    else:
        n = np.array(top // 2)
    z = rs.randint(K, size=N)
    x = rs.binomial(dense_trials(n, N, D), p.T[z].reshape(N, D)).astype(np.int64)
    w = rs.gamma(60.0, 1.0, size=(D, K))
    a, b = p * w + 0.5, (1 - p) * w + 0.5
    elog_p = np.stack([digamma(a) - digamma(a + b), digamma(b) - digamma(a + b)],
                      -1).reshape(D * K, 2)
    alpha = rs.gamma(5.0, 10.0, size=K)
    elog_pi = digamma(alpha) - digamma(alpha.sum())
    return dict(x=x, n=n, elog_p=elog_p, elog_pi=elog_pi,
                labels=rs.randint(K, size=N).astype(np.int32), rs=rs)


mixed_mask = _pmm.mixed_mask
junk_at_hidden = _pmm.junk_at_hidden


class CPUBINMKernels(CPUDirichletKernels):
    """Double of BINMKernels on CPU tensors; ``calls`` lists the entry points in call order."""

    def __init__(self, rt):
        self.rt = rt
        self.calls = []

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def plan(self, N, D, K):
        lib = binm_host()
        if K > lib.binm_max_k() or D > lib.binm_max_d():
            raise NotImplementedError('above the limits')
        return lib.binm_chunk_rows(N, D, K), lib.binm_workspace_doubles(N, D, K)

    def pack(self, N, D, dtype, x, trials, ts_n, ts_d, mask, xp, np_, flags, counts, lcoef, ws):
        self.calls.append('pack')
        o = host_pack(x.numpy().reshape(N, D), trials.numpy(), self._np(mask),
                      strides=(ts_n, ts_d))
        xp.numpy()[:N * D] = o['xp'].reshape(-1).view(np.int16)
        np_.numpy()[:N * D] = o['np'].reshape(-1).view(np.int16)
        flags.numpy()[...] |= o['flags']
        counts.numpy()[...] = [o['n_observed'], o['n_hidden'], o['constant']]
        lcoef.numpy()[0] = o['lcoef']

    def tables(self, D, K, form, elog_p, elog_pi, ncol, l1, l0, c, cfold=None):
        self.calls.append('tables')
        a, b, cc, cf = host_tables(D, K, form, self._np(elog_p), self._np(elog_pi),
                                   self._np(ncol) if cfold is not None else None)
        l1.numpy()[...] = a
        l0.numpy()[...] = b
        c.numpy()[...] = cc
        if cfold is not None:
            cfold.numpy()[...] = cf

    def pass_(self, N, D, K, one_plane, xp, np_, ncol, labels, l1, l0, c, ws, S, T, Nk, counts,
              scal, r_out=None):
        self.calls.append(('pass' if r_out is None else 'pass_r') + ('_one' if one_plane else ''))
        plane = lambda t: t.numpy()[:N * D].view(np.uint16).reshape(N, D)      # noqa: E731
        o = host_pass(N, D, K, one_plane, plane(xp), plane(np_), self._np(ncol), self._np(labels),
                      l1.numpy(), l0.numpy(), c.numpy(), r_out is not None)
        S.numpy()[...] = o['S']
        T.numpy()[...] = o['T']
        Nk.numpy()[...] = o['Nk']
        counts.numpy()[...] = o['counts']
        scal.numpy()[:3] = [o['sum_lse'], o['Nk_c'], o['dots']]
        if r_out is not None:
            r_out.numpy()[...] = o['r']
