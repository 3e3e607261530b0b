"""TEST INFRASTRUCTURE for the fused Poisson-mixture block.

* ``pmm_host()``: ctypes library of tests/host/pmm_host.cpp, built with g++ from csrc/vmp_pmm_dev.h
  -- the arithmetic and the order of additions of csrc/vmp_pmm.hip.
* ``restate_pack`` / ``restate_tables`` / ``restate_pass`` / ``restate_update``: NumPy restatements
  in a dtype of the caller's choice (no chunks, no tiles, no 16-bit x; the update and its bound term
  in the reference's own form): long double is the yardstick, float64 is the reference's own
  arithmetic.
* ``CPUPMMKernels``: the double of the plan's kernel object (inference/plans/pmm.py PMMKernels) on
  CPU tensors through the host build; Dirichlet rows and dot products in NumPy / SciPy.
* ``build_sanitized_program``: tests/host/pmm_host_main.cpp as a program of its own.
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

DTYPES = {'float64': 0, 'int64': 1, 'uint8': 2, 'int32': 3}
HIDDEN = 0xFFFF
MAX_COUNT = 65534
PASS_QUANTITIES = ('r', 'Nk', 'S', 'M', 'sum_lse', 'Nk_c', 'S_lM')
UPDATE_QUANTITIES = ('par', 'mom', 'bound')
HEADERS = ['bayespy_amd/csrc/vmp_pmm_dev.h', 'bayespy_amd/csrc/vmp_dgmm_masked_dev.h',
           'bayespy_amd/csrc/vmp_dgmm_dev.h']


@functools.lru_cache(None)
def pmm_host():
    lib = build_host_library('pmm', ['tests/host/pmm_host.cpp'] + HEADERS,
                             prelude=special_functions_text())
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    lib.pmm_dblock.argtypes = [i32]
    for name in ('pmm_chunk_rows', 'pmm_chunks', 'pmm_workspace_doubles'):
        getattr(lib, name).argtypes = [i64, i32, i32]
        getattr(lib, name).restype = i64
    for name in ('pmm_pack_span', 'pmm_pack_blocks'):
        getattr(lib, name).argtypes = [i64]
        getattr(lib, name).restype = i64
    lib.pmm_pack.argtypes = [i64, i32, i32] + [vp] * 6
    lib.pmm_pack.restype = None
    lib.pmm_tables.argtypes = [i32, i32, i32] + [vp] * 6
    lib.pmm_tables.restype = None
    lib.pmm_pass.argtypes = [i64, i32, i32, i32] + [vp] * 10
    lib.pmm_pass.restype = None
    lib.pmm_dots.argtypes = [ctypes.c_double] * 2
    lib.pmm_dots.restype = ctypes.c_double
    lib.pmm_update.argtypes = [i32, i32, i32] + [vp] * 7
    lib.pmm_update.restype = None
    return lib


def build_sanitized_program():
    """tests/host/pmm_host_main.cpp (which includes the host source) as a stand-alone program built
    with -fsanitize=address,undefined; returns its path."""
    d = tempfile.mkdtemp(prefix='bayespy_amd_pmm_san_')
    exe = os.path.join(d, 'pmm_host_main')
    pre = os.path.join(d, 'prelude.h')
    with open(pre, 'w') as f:
        f.write(special_functions_text())
    flags = [f for f in FLAGS if f not in ('-shared', '-fPIC')]
    subprocess.check_call(['g++'] + flags + ['-g', '-fsanitize=address,undefined',
                                             '-fno-sanitize-recover=all', '-include', pre,
                                             os.path.join(ROOT, 'tests/host/pmm_host_main.cpp'),
                                             '-o', exe])
    return exe


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def host_pack(x, mask=None):
    """dict of xp (N, D) uint16, flags (3), n_observed, n_hidden, lgam of a 2-D array of dtype
    float64 / int64 / int32 / uint8."""
    x = np.ascontiguousarray(x)
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    N, D = x.shape
    xp = np.zeros((N, D), dtype=np.uint16)
    flags, counts, lgam = np.zeros(3, dtype=np.int32), np.zeros(2, dtype=np.int64), np.zeros(1)
    pmm_host().pmm_pack(N, D, DTYPES[x.dtype.name], _p(x), _p(m), _p(xp), _p(flags), _p(counts),
                        _p(lgam))
    return dict(xp=xp, flags=flags, n_observed=int(counts[0]), n_hidden=int(counts[1]),
                lgam=float(lgam[0]))


def host_tables(D, K, form, lam_mom, elog_pi):
    """(l, lb (D, K), c (K), lsum (K)) of the host build; the moment table (D K, 2) or None."""
    l, lb, c, lsum = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K), np.zeros(K)
    bufs = (_c(lam_mom), _c(elog_pi))
    pmm_host().pmm_tables(D, K, form, _p(bufs[0]), _p(bufs[1]), _p(l), _p(lb), _p(c), _p(lsum))
    return l, lb, c, lsum


def host_pass(N, D, K, hidden, xp, labels, l, lb, c, want_r=False):
    """dict of S, M (D, K), Nk (K), sum_lse, Nk_c, S_lM, r or None of the host build on the packed
    ``xp``.  Without hidden entries M is N_k on every row, as the update uses it."""
    S, M, Nk, scal = np.zeros((D, K)), np.zeros((D, K)), np.zeros(K), np.zeros(1)
    r = np.full((N, K), np.nan) if want_r else None
    bufs = (np.ascontiguousarray(xp, dtype=np.uint16),
            None if labels is None else np.ascontiguousarray(labels, dtype=np.int32),
            _c(l), _c(lb), _c(c))
    lib = pmm_host()
    lib.pmm_pass(N, D, K, hidden, *[_p(b) for b in bufs], _p(S), _p(M), _p(Nk), _p(scal), _p(r))
    s_l = float(np.sum(S * bufs[2]))
    S_lM = lib.pmm_dots(s_l, float(np.sum(M * bufs[3]))) if hidden else s_l
    if not hidden:
        M = np.broadcast_to(Nk, (D, K)).copy()
    return dict(S=S, M=M, Nk=Nk, sum_lse=float(scal[0]), r=r, Nk_c=float(np.sum(Nk * bufs[4])),
                S_lM=S_lM)


def host_update(D, K, per_element, prior_a, prior_b, S, cnt):
    """(par (D K, 2), mom (D K, 2), bound) of the host build; statistics None: the prior."""
    par, mom, bound = np.zeros((D * K, 2)), np.zeros((D * K, 2)), np.zeros(1)
    bufs = [_c(np.broadcast_to(prior_a, (D, K))), _c(np.broadcast_to(prior_b, (D, K))), _c(S),
            _c(cnt)]
    pmm_host().pmm_update(D, K, per_element, *[_p(b) for b in bufs], _p(par), _p(mom), _p(bound))
    return par, mom, float(bound[0])


# -- restatements ------------------------------------------------------------------------------------
def restate_pack(x, mask=None, dtype=np.longdouble):
    """The pack the way the entry point is documented, in NumPy: dict of xp, flags, n_observed,
    n_hidden and lgam = sum over the observed entries of lgamma(x + 1) in ``dtype``."""
    x = np.asarray(x)
    seen = np.ones(x.shape, dtype=bool) if mask is None else np.asarray(mask) != 0
    with np.errstate(invalid='ignore'):
        xf = x.astype(np.float64)
        whole = xf == np.floor(xf)
        nonneg = xf >= 0
        ok = whole & nonneg & (xf <= MAX_COUNT)
    xp = np.where(seen & ok, np.where(ok, xf, 0), HIDDEN).astype(np.uint16)
    flags = np.array([np.any(seen & ~(whole & nonneg)), np.any(seen & whole & nonneg & ~ok),
                      np.any(seen & ~whole)], dtype=np.int32)
    obs = xp[xp != HIDDEN]
    lgamma = _special(dtype)[1]
    if dtype == np.float64:                 # the reference: gammaln of every entry, then the sum
        lgam = float(np.sum(lgamma(obs.astype(np.float64) + 1.0)))
    else:                                   # one evaluation per distinct count
        vals, cnt = np.unique(obs, return_counts=True)
        lg = lgamma(vals.astype(np.float64) + 1.0) if vals.size else np.zeros(0, dtype)
        lgam = np.sum(np.asarray(lg, dtype=dtype) * cnt.astype(dtype))
    return dict(xp=xp, flags=flags, n_observed=int(obs.size), n_hidden=int(xp.size - obs.size),
                lgam=lgam)


def restate_tables(lam_mom, elog_pi, D, K, form, dtype=np.longdouble):
    """l, lb, c and lsum from the moment table (None: zeros), in ``dtype``."""
    mom = np.zeros((D, K, 2), dtype=dtype) if lam_mom is None \
        else np.asarray(lam_mom, dtype=dtype).reshape(D, K, 2)
    l, lb = mom[..., 1], mom[..., 0]
    if form & 2:                                        # centred: column 0 of every row taken out
        l, lb = l - l[:, :1], lb - lb[:, :1]
    lsum = lb.sum(axis=0)
    c = np.asarray(elog_pi, dtype=dtype) - (0 if form & 1 else lsum)
    return l, lb, c - c.max(), lsum


def restate_pass(x, mask, l, lb, c, hidden, dtype=np.longdouble, labels=None):
    """The pass on dense x (N, D) and mask (N, D) or None in ``dtype``, the way mixture.py /
    poisson.py / categorical.py evaluate it (hidden entries of x are not looked at): dict of
    r (N, K), lse (N), Nk, S, M (D, K), sum_lse and the dot products of the bound.  ``hidden``: the
    form of c and of scal[2] (vmp_pmm_dev.h).  Rows with nothing observed keep r = softmax(c) and
    enter no sum."""
    x = np.asarray(x)
    m = np.ones(x.shape, dtype=bool) if mask is None else (np.asarray(mask) != 0)
    xt = np.where(m, np.nan_to_num(np.asarray(x, dtype=np.float64), nan=0.0, posinf=0.0,
                                   neginf=0.0), 0.0).astype(dtype)
    md = m.astype(dtype)
    l, lb, c = (np.asarray(a, dtype=dtype) for a in (l, lb, c))
    K = c.shape[0]
    if labels is None:
        logit = c + xt @ l - (md @ lb if hidden else 0)
        mx = logit.max(axis=1, keepdims=True) if len(xt) else np.zeros((0, 1), dtype=dtype)
        lse = mx[:, 0] + np.log(np.exp(logit - mx).sum(axis=1))
        r = np.exp(logit - lse[:, None])
    else:
        r = np.eye(K, dtype=dtype)[np.asarray(labels)]
        lse = np.zeros(len(xt), dtype=dtype)
    obs = m.any(axis=1)
    ro = r * obs[:, None].astype(dtype)
    Nk, M, S = ro.sum(axis=0), md.T @ ro, xt.T @ ro
    return dict(r=r, lse=lse, Nk=Nk, M=M, S=S, sum_lse=(lse * obs).sum(), Nk_c=np.sum(Nk * c),
                S_lM=np.sum(S * l) - (np.sum(M * lb) if hidden else 0))


def restate_update(a0, b0, S, cnt, dtype=np.longdouble):
    """q(lam) from the statistics with the bound term in the reference's form: cgf of the prior -
    cgf of q + sum (phi_p - phi_q) u.  ``cnt``: (K) or (D, K); statistics None: the prior."""
    psi, lgam = _special(dtype)
    D, K = np.shape(a0)
    t = lambda a: np.array(np.broadcast_to(a, (D, K)), dtype=dtype)     # noqa: E731
    a0, b0 = t(a0), t(b0)
    S = t(0.0) if S is None else t(S)
    cnt = t(0.0) if cnt is None else t(cnt)
    a, b = a0 + S, b0 + cnt
    v = np.stack([a / b, psi(a) - np.log(b)], -1)
    L = (a0 * np.log(b0) - lgam(a0)) - (a * np.log(b) - lgam(a)) + (-b0 + b) * v[..., 0] \
        + (a0 - a) * v[..., 1]
    return dict(par=np.stack([a, b], -1).reshape(D * K, 2), mom=v.reshape(D * K, 2),
                bound=L.sum())


# -- inputs ------------------------------------------------------------------------------------------
EPS = 0.3


def pass_inputs(N, D, K):
    """Counts x (N, D) int64 with SOFT rows: the rate of (d, k) is lam_d exp(eps_dk) with eps of
    scale EPS / sqrt(D), so the clusters' log-odds of a row are of order one at every D.  Also the
    moment table (D K, 2) of a plausible Gamma posterior around those rates, <log pi>, labels, the
    priors and the random state."""
    from scipy.special import digamma
    rs = np.random.RandomState(1000 * K + 10 * D + N)
    base = rs.gamma(2.0, 2.5, size=(D, 1)) + 0.5
    rate = base * np.exp(rs.normal(scale=EPS / np.sqrt(D), size=(D, K)))
    z = rs.randint(K, size=N)
    x = rs.poisson(rate.T[z]).astype(np.int64).reshape(N, D)
    b = rs.gamma(50.0, 1.0, size=(D, K))
    a = rate * b
    lam_mom = np.stack([a / b, digamma(a) - np.log(b)], -1).reshape(D * K, 2)
    alpha = rs.gamma(5.0, 10.0, size=K)
    elog_pi = digamma(alpha) - digamma(alpha.sum())
    return dict(x=x, lam_mom=lam_mom, elog_pi=elog_pi, labels=rs.randint(K, size=N).astype(np.int32),
                a0=rs.gamma(2.0, 0.5, size=(D, K)) + 0.01, b0=rs.gamma(2.0, 0.5, size=(D, K)) + 0.01,
                rs=rs)


def mixed_mask(N, D, rs, block):
    """The mask of fixture (f) at any size: about 70 % ones with, where the shape has room, row 2
    and column 1 of nothing, row 5 fully observed (but for column 1) and a hidden entry in the last
    column of the first column block and in the first column of the second (row 7)."""
    m = rs.rand(N, D) < 0.7
    if N > 5:
        m[5] = True
    if N > 2:
        m[2] = False
    if D > 2:
        m[:, 1] = False
    if N > 7:
        if D >= block:
            m[7, block - 1] = False
        if D > block:
            m[7, block] = False
    return m


def junk_at_hidden(x, mask, value):
    """``x`` as float64 with ``value`` at the hidden positions."""
    return np.where(np.asarray(mask) != 0, np.asarray(x, dtype=np.float64), value)


class CPUPMMKernels(CPUDirichletKernels):
    """Double of PMMKernels on CPU tensors; ``calls`` lists the entry points in call order."""

    def __init__(self, rt):
        self.rt = rt
        self.calls = []

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def plan(self, N, D, K):
        lib = pmm_host()
        if K > lib.pmm_max_k() or D > lib.pmm_max_d():
            raise NotImplementedError('above the limits')
        return lib.pmm_chunk_rows(N, D, K), lib.pmm_workspace_doubles(N, D, K)

    def pack(self, N, D, dtype, x, mask, xp, flags, counts, lgam, ws):
        self.calls.append('pack')
        o = host_pack(x.numpy().reshape(N, D), self._np(mask))
        xp.numpy()[:N * D] = o['xp'].reshape(-1).view(np.int16)
        flags.numpy()[...] |= o['flags']
        counts.numpy()[...] = [o['n_observed'], o['n_hidden']]
        lgam.numpy()[0] = o['lgam']

    def tables(self, D, K, form, lam_mom, elog_pi, l, lb, c, lsum=None):
        self.calls.append('tables')
        ll, bb, cc, ss = host_tables(D, K, form, self._np(lam_mom), self._np(elog_pi))
        l.numpy()[...] = ll
        lb.numpy()[...] = bb
        c.numpy()[...] = cc
        if lsum is not None:
            lsum.numpy()[...] = ss

    def pass_(self, N, D, K, hidden, xp, labels, l, lb, c, ws, S, M, Nk, scal, r_out=None):
        self.calls.append(('pass' if r_out is None else 'pass_r') + ('_hidden' if hidden else ''))
        o = host_pass(N, D, K, hidden, xp.numpy()[:N * D].view(np.uint16).reshape(N, D),
                      self._np(labels), l.numpy(), lb.numpy(), c.numpy(), r_out is not None)
        S.numpy()[...] = o['S']
        if hidden:
            M.numpy()[...] = o['M']
        Nk.numpy()[...] = o['Nk']
        scal.numpy()[:3] = [o['sum_lse'], o['Nk_c'], o['S_lM']]
        if r_out is not None:
            r_out.numpy()[...] = o['r']

    def update(self, D, K, per_element, prior_a, prior_b, S, cnt, par, mom, bound):
        self.calls.append('update_M' if per_element else 'update')
        p, m, b = host_update(D, K, per_element, prior_a.numpy(), prior_b.numpy(), self._np(S),
                              self._np(cnt))
        par.numpy()[...] = p
        mom.numpy()[...] = m
        bound.numpy()[...] = b
