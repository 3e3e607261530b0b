"""TEST INFRASTRUCTURE for the fused multinomial-mixture block.

* ``mmm_host()``: ctypes library of tests/host/mmm_host.cpp, built with g++ from csrc/vmp_mmm_dev.h
  -- the arithmetic and the order of additions of csrc/vmp_mmm.hip.
* ``restate_pack`` / ``restate_tables`` / ``restate_pass``: NumPy restatements in a dtype of the
  caller's choice (no chunks, no tiles, no 16-bit x): long double is the yardstick, float64 is the
  reference's own arithmetic.
* ``CPUMMMKernels``: the double of the plan's kernel object (inference/plans/mmm.py MMMKernels) on
  CPU tensors through the host build; Dirichlet rows and dot products in NumPy / SciPy.
It lives under tests/ and is never imported by the product."""
import ctypes
import functools

import numpy as np

from host_build import build_host_library, special_functions_text
from lda_host import CPUDirichletKernels
from dgmm_host import _special, tolerances, error            # noqa: F401

DTYPES = {'float64': 0, 'int64': 1, 'uint8': 2, 'int32': 3}
MAX_COUNT = 65534
PASS_QUANTITIES = ('r', 'Nk', 'S', 'sum_lse', 'Nk_c', 'S_L')
HEADERS = ['tests/host/pmm_host.cpp', 'bayespy_amd/csrc/vmp_mmm_dev.h',
           'bayespy_amd/csrc/vmp_pmm_dev.h', 'bayespy_amd/csrc/vmp_dgmm_masked_dev.h',
           'bayespy_amd/csrc/vmp_dgmm_dev.h']


@functools.lru_cache(None)
def mmm_host():
    lib = build_host_library('mmm', ['tests/host/mmm_host.cpp'] + HEADERS,
                             prelude=special_functions_text())
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    for name in ('mmm_chunk_rows', 'mmm_chunks', 'mmm_workspace_doubles'):
        getattr(lib, name).argtypes = [i64, i32, i32]
        getattr(lib, name).restype = i64
    lib.mmm_pack.argtypes = [i64, i32, i32] + [vp] * 5
    lib.mmm_pack.restype = None
    lib.mmm_tables.argtypes = [i32, i32] + [vp] * 4
    lib.mmm_tables.restype = None
    lib.mmm_pass.argtypes = [i64, i32, i32] + [vp] * 8
    lib.mmm_pass.restype = None
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def host_pack(x, trials):
    """dict of xp (N, M) uint16, flags (4) and lcoef of a 2-D array of dtype float64 / int64 /
    int32 / uint8 and the trials (N)."""
    x = np.ascontiguousarray(x)
    N, M = x.shape
    n = np.ascontiguousarray(np.broadcast_to(trials, (N,)), dtype=np.int64)
    xp = np.zeros((N, M), dtype=np.uint16)
    flags, lcoef = np.zeros(4, dtype=np.int32), np.zeros(1)
    mmm_host().mmm_pack(N, M, DTYPES[x.dtype.name], _p(x), _p(n), _p(xp), _p(flags), _p(lcoef))
    return dict(xp=xp, flags=flags, lcoef=float(lcoef[0]))


def host_tables(M, K, elog_p, elog_pi):
    """(L (M, K), c (K)) of the host build; elog_p (K, M) or None."""
    L, c = np.zeros((M, K)), np.zeros(K)
    bufs = (_c(elog_p), _c(elog_pi))
    mmm_host().mmm_tables(M, K, _p(bufs[0]), _p(bufs[1]), _p(L), _p(c))
    return L, c


def host_pass(N, M, K, xp, labels, L, c, want_r=False):
    """dict of S (K, M), Nk (K), sum_lse, Nk_c, S_L, r or None of the host build on the packed
    ``xp``."""
    S, Nk, scal = np.zeros((K, M)), np.zeros(K), np.zeros(3)
    r = np.full((N, K), np.nan) if want_r else None
    bufs = (np.ascontiguousarray(xp, dtype=np.uint16),
            None if labels is None else np.ascontiguousarray(labels, dtype=np.int32), _c(L), _c(c))
    mmm_host().mmm_pass(N, M, K, *[_p(b) for b in bufs], _p(S), _p(Nk), _p(scal), _p(r))
    return dict(S=S, Nk=Nk, sum_lse=float(scal[0]), Nk_c=float(scal[1]), S_L=float(scal[2]), r=r)


# -- restatements ------------------------------------------------------------------------------------
def restate_pack(x, trials, dtype=np.longdouble):
    """The pack the way the entry point is documented, in NumPy: dict of xp, flags and
    lcoef = sum_n [lgamma(n_n + 1) - sum_m lgamma(x_nm + 1)] in ``dtype``."""
    x = np.asarray(x)
    n = np.broadcast_to(np.asarray(trials, dtype=np.int64), x.shape[:1])
    with np.errstate(invalid='ignore'):
        xf = x.astype(np.float64)
        whole = xf == np.floor(xf)
        nonneg = xf >= 0
        ok = whole & nonneg & (xf <= MAX_COUNT)
    xp = np.where(ok, xf, 0).astype(np.uint16)
    clean = ok.all(axis=1)
    flags = np.array([np.any(~(whole & nonneg)), np.any(whole & nonneg & ~ok), np.any(~whole),
                      np.any(clean & (xp.astype(np.int64).sum(axis=1) != n))], dtype=np.int32)
    lgamma = _special(dtype)[1]
    if dtype == np.float64:                 # the reference: gammaln of every entry, then the sums
        lcoef = float(np.sum(lgamma(n + 1.0) - np.sum(lgamma(xp.astype(np.float64) + 1.0), axis=-1)))
    else:                                   # one evaluation per distinct count
        total = dtype(0)
        for a, sign in ((n, 1), (xp, -1)):
            vals, cnt = np.unique(a, return_counts=True)
            lg = lgamma(vals.astype(np.float64) + 1.0) if vals.size else np.zeros(0, dtype)
            total = total + sign * np.sum(np.asarray(lg, dtype=dtype) * cnt.astype(dtype))
        lcoef = total
    return dict(xp=xp, flags=flags, lcoef=lcoef)


def restate_tables(elog_p, elog_pi, M, K, dtype=np.longdouble):
    """L (M, K) and c from <log p> (K, M) (None: zeros), in ``dtype``."""
    e = np.zeros((K, M), dtype=dtype) if elog_p is None else np.asarray(elog_p, dtype=dtype)
    c = np.asarray(elog_pi, dtype=dtype)
    return (e - e[:1]).T, c - c.max()


def restate_pass(x, L, c, dtype=np.longdouble, labels=None):
    """The pass on dense x (N, M) in ``dtype``, the way mixture.py / multinomial.py /
    categorical.py evaluate it: dict of r (N, K), lse (N), Nk, S (K, M), sum_lse and the dot
    products of the bound."""
    xt = np.asarray(x, dtype=np.float64).astype(dtype)
    L, c = np.asarray(L, dtype=dtype), np.asarray(c, dtype=dtype)
    K = c.shape[0]
    if labels is None:
        logit = c + xt @ L
        mx = logit.max(axis=1, keepdims=True) if len(xt) else np.zeros((0, 1), dtype=dtype)
        lse = mx[:, 0] + np.log(np.exp(logit - mx).sum(axis=1))
        r = np.exp(logit - lse[:, None])
    else:
        r = np.eye(K, dtype=dtype)[np.asarray(labels)]
        lse = np.zeros(len(xt), dtype=dtype)
    Nk, S = r.sum(axis=0), r.T @ xt
    return dict(r=r, lse=lse, Nk=Nk, S=S, sum_lse=lse.sum(), Nk_c=np.sum(Nk * c),
                S_L=np.sum(S * L.T))


# -- inputs ------------------------------------------------------------------------------------------
def pass_inputs(N, M, K):
    """Count vectors x (N, M) int64 with SOFT rows: 20 to 59 trials a row, the word probabilities of
    cluster k are base_m exp(eps_km) renormalised with eps of scale 0.16, so the clusters' log-odds
    of a row are of order one at every M.  Also the trials (N), <log p> (K, M) of a plausible
    Dirichlet posterior around those probabilities, <log pi>, labels and the random state."""
    from scipy.special import digamma
    rs = np.random.RandomState(1000 * K + 10 * M + N)
    base = rs.dirichlet(2.0 * np.ones(M))
    p = base * np.exp(rs.normal(scale=0.16, size=(K, M)))
    p /= p.sum(axis=1, keepdims=True)
    z = rs.randint(K, size=N)
    trials = rs.randint(20, 60, size=N).astype(np.int64)
    x = np.array([rs.multinomial(n, p[k]) for n, k in zip(trials, z)], dtype=np.int64).reshape(N, M)
    alpha_p = p * 200.0 * M + 0.5
    elog_p = digamma(alpha_p) - digamma(alpha_p.sum(axis=1, keepdims=True))
    alpha = rs.gamma(5.0, 10.0, size=K)
    elog_pi = digamma(alpha) - digamma(alpha.sum())
    return dict(x=x, trials=trials, elog_p=elog_p, elog_pi=elog_pi,
                labels=rs.randint(K, size=N).astype(np.int32), rs=rs)


class CPUMMMKernels(CPUDirichletKernels):
    """Double of MMMKernels on CPU tensors; ``calls`` lists the entry points in call order."""

    def __init__(self, rt):
        self.rt = rt
        self.calls = []

    @staticmethod
    def _np(t):
        return None if t is None else t.numpy()

    def plan(self, N, M, K):
        lib = mmm_host()
        if K > lib.mmm_max_k() or M > lib.mmm_max_m():
            raise NotImplementedError('above the limits')
        return lib.mmm_chunk_rows(N, M, K), lib.mmm_workspace_doubles(N, M, K)

    def pack(self, N, M, dtype, x, trials, xp, flags, lcoef, ws):
        self.calls.append('pack')
        o = host_pack(x.numpy().reshape(N, M), trials.numpy()[:N])
        xp.numpy()[:N * M] = o['xp'].reshape(-1).view(np.int16)
        flags.numpy()[...] |= o['flags']
        lcoef.numpy()[0] = o['lcoef']

    def tables(self, M, K, elog_p, elog_pi, L, c):
        self.calls.append('tables')
        ll, cc = host_tables(M, K, self._np(elog_p), self._np(elog_pi))
        L.numpy()[...] = ll
        c.numpy()[...] = cc

    def pass_(self, N, M, K, xp, labels, L, c, ws, S, Nk, scal, r_out=None):
        self.calls.append('pass' if r_out is None else 'pass_r')
        o = host_pass(N, M, K, xp.numpy()[:N * M].view(np.uint16).reshape(N, M), self._np(labels),
                      L.numpy(), c.numpy(), r_out is not None)
        S.numpy()[...] = o['S']
        Nk.numpy()[...] = o['Nk']
        scal.numpy()[:3] = [o['sum_lse'], o['Nk_c'], o['S_L']]
        if r_out is not None:
            r_out.numpy()[...] = o['r']
