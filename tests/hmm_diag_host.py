"""TEST INFRASTRUCTURE of tests/test_hmm_diag_gpu.py: the long-double restatement and the inputs;
the recursion, the sums and the allowance rule are those of tests/hmm_cat_host.py, as they are."""
import numpy as np

import hmm_cat_host as cat
from hmm_cat_host import PER_CHAIN

_cat_restate = cat.restate
SUMS = ('z0sum', 'xisum', 'S1', 'S2', 'Nk', 'logZ', 'ge')
ALL = SUMS + PER_CHAIN


def restate(y, tables, la0, lA, dtype=np.longdouble, mask=None):
    """``hmm_cat_host.restate`` with e = g + y . h + y^2 . q (0 at a masked step; ``tables`` None:
    0) and S1, S2, Nk as plain sums in ``dtype``: every step is a word of its own with e as its
    row, so that the count table of the categorical restatement is gamma at the observed steps."""
    y = np.asarray(y)
    B, T, D = y.shape
    obs = np.ones((B, T), dtype=bool) if mask is None else (np.asarray(mask) != 0)
    ys = np.where(obs[..., None], y, 0).astype(dtype).reshape(B * T, D)
    if tables is None:
        table = B * T
    else:
        h, q, g = (np.asarray(a, dtype=dtype) for a in tables)
        table = g + ys @ h + (ys * ys) @ q
    r = _cat_restate(np.arange(B * T).reshape(B, T), table, la0, lA, dtype, mask)
    gm = r.pop('S')
    r.update(S1=ys.T @ gm, S2=(ys * ys).T @ gm, Nk=gm.sum(0))
    return r


def compare(got, y, tables, la0, lA, keys=SUMS, label='', mask=None):
    cat.restate = restate
    try:
        return cat.compare(got, y, tables, la0, lA, keys, label, mask=mask)
    finally:
        cat.restate = _cat_restate


def pass_inputs(B, T, D, K, mean=0.0):
    """(y, (h, q, g), la0, lA): moments of a Gaussian-Gamma posterior per (d, k), digamma tables for
    the chain; ``mean``: y ~ N(mean, 1) per dimension around state means near ``mean``."""
    _, _, la0, lA = cat.pass_inputs(B, T, 2, K)
    rs = np.random.RandomState(B + 3 * T + 5 * D + 7 * K + 2)
    m, v = mean + rs.randn(D, K), 0.01 + 0.05 * rs.rand(D, K)
    a, b = 2.0 + 3.0 * rs.rand(D, K), 1.0 + 2.0 * rs.rand(D, K)
    from scipy import special
    tau, logtau = a / b, special.digamma(a) - np.log(b)
    tables = (tau * m, -0.5 * tau, (0.5 * logtau - 0.5 * tau * (m * m + v)).sum(0))
    return mean + rs.randn(B, T, D), tables, la0, lA
