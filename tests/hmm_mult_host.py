"""TEST INFRASTRUCTURE of tests/test_hmm_mult_gpu.py: the long-double restatement and the inputs;
the recursion, the sums and the allowance rule are those of tests/hmm_cat_host.py, as they are."""
import numpy as np

import hmm_cat_host as cat
from hmm_cat_host import ALL, SUMS  # noqa: F401

_cat_restate = cat.restate


def restate(x, Pt, la0, lA, dtype=np.longdouble, mask=None):
    """``hmm_cat_host.restate`` with e = x @ Pt (0 at a masked step; an integer ``Pt`` = M: 0) and
    S = sum_obs x (outer) gamma in ``dtype``: every step is a word of its own with e as its row."""
    x = np.asarray(x)
    B, T, M = x.shape
    obs = np.ones((B, T), dtype=bool) if mask is None else (np.asarray(mask) != 0)
    xs = np.where(obs[..., None], x, 0).astype(dtype).reshape(B * T, M)
    table = B * T if isinstance(Pt, int) else xs @ np.asarray(Pt, dtype=dtype)
    r = _cat_restate(np.arange(B * T).reshape(B, T), table, la0, lA, dtype, mask)
    r['S'] = xs.T @ r['S']
    return r


def compare(got, x, Pt, la0, lA, keys=SUMS, label='', mask=None):
    cat.restate = restate
    try:
        return cat.compare(got, x, Pt, la0, lA, keys, label, mask=mask)
    finally:
        cat.restate = _cat_restate


def pass_inputs(B, T, M, K, big=False):
    """(x, Pt, la0, lA): digamma tables, row totals 1 to 299; ``big``: a single count of 65534."""
    _, Pt, la0, lA = cat.pass_inputs(B, T, M, K)
    rs = np.random.RandomState(B + 3 * T + 5 * M + 7 * K + 1)
    p = rs.dirichlet(np.full(M, 0.3))
    x = np.array([rs.multinomial(n, p) for n in rs.randint(1, 300, size=B * T)]).reshape(B, T, M)
    if big:
        x[0, 1] = 0
        x[0, 1, M - 1] = 65534
    return x, Pt, la0, lA
