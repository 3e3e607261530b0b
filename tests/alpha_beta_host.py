"""TEST INFRASTRUCTURE for the generic forward-backward kernel (csrc/vmp_hmm.hip,
``vmp_alpha_beta_recursion``).

* ``restate``: ``random.alpha_beta_recursion`` of the reference (utils/random.py:357-422) in a
  dtype of the caller's choice, statement by statement: per-axis log-sum-exp for logalpha and
  logbeta, ``exp(v - lse(v))`` and a second normalisation for ``zz``, ``z0`` from the rows of
  ``zz_0``.  Long double is the yardstick, float64 is the reference's own arithmetic.
* ``allowances`` / ``compare``: the rule of DESIGN 4.14 / 4.15 (tests/hmm_fused_host.py
  ``compare``) for ``z0``, ``zz`` and ``g``.
* ``inputs``: seeded generators of the regimes the CPU and the GPU tests share, ``SPARSE`` the
  sparse-table case in which a shift by the joint maximum of a slice loses the only route.
It lives under tests/ and is never imported by the product."""
import numpy as np
from scipy import special

EXP_UNDERFLOW = 745.0           # exp(-745.2) is the last float64 above zero


def _lse(x, axis):
    m = np.max(x, axis=axis, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        m0 = np.where(np.isfinite(m), m, 0)
        return np.squeeze(m0, axis) + np.log(np.sum(np.exp(x - m0), axis=axis))


def restate(logp0, logP, dtype=np.longdouble, full=False):
    """logp0 (..., K), logP (..., N, K, K), chain and time axes of either may be broadcast ->
    z0 (..., K), zz (..., N, K, K), g (...,) in ``dtype``; with ``full`` also logalpha and logbeta
    (..., N, K)."""
    logp0 = np.asarray(logp0, dtype=dtype)
    logP = np.asarray(logP, dtype=dtype)
    K = logp0.shape[-1]
    N = logP.shape[-3]
    assert logP.shape[-2:] == (K, K)
    plates = np.broadcast_shapes(logp0.shape[:-1], logP.shape[:-3])
    logP = np.broadcast_to(logP, plates + (N, K, K))
    la = np.zeros(plates + (N, K), dtype=dtype)
    lb = np.zeros(plates + (N, K), dtype=dtype)
    g = np.zeros(plates, dtype=dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        la[..., 0, :] = logp0
        for n in range(1, N):
            v = la[..., n - 1, :, None] + logP[..., n - 1, :, :]
            c = _lse(v.reshape(plates + (K * K,)), -1)
            la[..., n, :] = _lse(v - c[..., None, None], -2)
            g -= c
        v = la[..., N - 1, :, None] + logP[..., N - 1, :, :]
        g -= _lse(v.reshape(plates + (K * K,)), -1)
        for n in reversed(range(N - 1)):
            v = lb[..., n + 1, None, :] + logP[..., n + 1, :, :]
            c = _lse(v.reshape(plates + (K * K,)), -1)
            lb[..., n, :] = _lse(v - c[..., None, None], -1)
        v = la[..., :, :, None] + lb[..., :, None, :] + logP
        c = _lse(v.reshape(plates + (N, K * K)), -1)
        zz = np.exp(v - c[..., None, None])
        zz = zz / np.sum(zz, axis=(-1, -2), keepdims=True)
        z0 = np.sum(zz[..., 0, :, :], axis=-1)
        z0 = z0 / np.sum(z0, axis=-1, keepdims=True)
    return (z0, zz, g, la, lb) if full else (z0, zz, g)


KEYS = ('z0', 'zz', 'g')


def allowances(logp0, logP, keys=KEYS):
    """key -> (long-double value, float64 deviation, allowance): 8 times the largest deviation of
    the float64 evaluation of ``restate`` from the long-double one, at least 4 ulp of the
    quantity's magnitude."""
    ld = dict(zip(KEYS, restate(logp0, logP)))
    f64 = dict(zip(KEYS, restate(logp0, logP, np.float64)))
    out = {}
    for key in keys:
        ref = ld[key]
        dev = float(np.max(np.abs(np.asarray(f64[key], dtype=np.longdouble) - ref)))
        mag = float(np.max(np.abs(ref)))
        out[key] = (ref, dev, max(8 * dev, 4 * float(np.spacing(mag))))
    return out


def compare(got, logp0, logP, keys=KEYS, label='', out=print):
    """``got``: dict of z0, zz, g of the code under test.  Prints float64 deviation, error and
    allowance per quantity; returns the failures as (key, error, allowance)."""
    bad = []
    for key, (ref, dev, tol) in allowances(logp0, logP, keys).items():
        err = float(np.max(np.abs(np.asarray(got[key], dtype=np.longdouble).reshape(ref.shape)
                                  - ref)))
        out('%s %-3s float64 deviation %.3e  error %.3e  allowance %.3e' % (label, key, dev, err, tol))
        if not err <= tol:
            bad.append((key, err, tol))
    return bad


# the sparse-table case: a Dirichlet(1e-3) table (every unlearned entry at psi(1e-3) - psi(3e-3),
# rounded to -985 with the emission constants) with five learned entries, and one 40-sigma
# outlier (-800) at instance 1.  The only cheap route is 1 -> 2 at instance 1, and state 1 sits
# more than 745 below state 0 in logalpha_1 AND below the joint maximum of the slice.
def _sparse_case():
    lA = np.full((3, 3), -985.0)
    lA[0, 0], lA[0, 1], lA[1, 1], lA[1, 2], lA[2, 2] = -0.1, -2.5, -3.0, -0.05, -0.01
    ev = np.array([[0.0, 0.0, -50.0], [0.0, -800.0, -900.0], [-900.0, -900.0, 0.0],
                   [-900.0, -900.0, 0.0]])
    return np.log(1.0 / 3.0) + ev[0], lA[None] + ev[1:, None, :]


SPARSE = _sparse_case()
SPARSE_G = 803.18               # -log-normaliser of the sparse case (oracle/hmm.py: 803.1837...)

KINDS = ('random', 'inf_p0', 'inf_col', 'inf_row', 'left_to_right', 'sparse', 'dirichlet_tiny',
         'one_row', 'long')
INF_KINDS = ('inf_p0', 'inf_col', 'inf_row', 'left_to_right')


def inputs(kind, B, N, K, seed=0):
    """logp0 (B, K), logP (B, N, K, K) of one regime.

    random          2 randn tables
    inf_p0          random, one -inf entry of logp0 per chain
    inf_col         random, a whole column -inf at one instance per chain (needs K >= 2)
    inf_row         random, a whole row -inf at one instance per chain (needs K >= 2)
    left_to_right   random, upper-triangular tables: -inf below the diagonal
    sparse          chain 0 is ``SPARSE`` (K = 3, N = 3), the others relabel its states
    dirichlet_tiny  every entry psi(1e-3) - psi(K 1e-3) < -900: the unlearned Dirichlet(1e-3) table
    one_row         row 0 learned (log of a probability row), the other rows in (-745, -600);
                    odd chains start in a state other than 0, so their first transition leaves
                    from a row 600 below the used one
    long            emissions N(mean_k, I_4) with means 50 apart, sticky transitions
    """
    rs = np.random.RandomState(seed)
    if kind in ('random',) + INF_KINDS:
        logp0 = 2.0 * rs.randn(B, K)
        logP = 2.0 * rs.randn(B, N, K, K)
        for b in range(B):
            n = rs.randint(N)
            if kind == 'inf_p0' and K > 1:
                logp0[b, rs.randint(K)] = -np.inf
            elif kind == 'inf_col':
                logP[b, n, :, rs.randint(K)] = -np.inf
            elif kind == 'inf_row':
                logP[b, n, rs.randint(K), :] = -np.inf
        if kind == 'left_to_right':
            logP[..., np.tril_indices(K, -1)[0], np.tril_indices(K, -1)[1]] = -np.inf
        return logp0, logP
    if kind == 'sparse':
        assert (N, K) == (3, 3)
        p0, P = SPARSE
        logp0, logP = np.empty((B, K)), np.empty((B, N, K, K))
        for b in range(B):
            perm = np.arange(K) if b == 0 else rs.permutation(K)
            logp0[b] = p0[perm]
            logP[b] = P[:, perm][:, :, perm]
        return logp0, logP
    if kind == 'dirichlet_tiny':
        e = float(special.psi(1e-3) - special.psi(K * 1e-3))
        return np.full((B, K), e), np.full((B, N, K, K), e)
    if kind == 'one_row':
        row = np.log(rs.dirichlet(np.ones(K), size=(B, N)))
        logP = -600.0 - 140.0 * rs.rand(B, N, K, K)
        logP[:, :, 0, :] = row
        logp0 = np.full((B, K), -800.0)
        logp0[np.arange(B), np.where(np.arange(B) % 2 == 1, 1 % K, 0)] = 0.0
        return logp0, logP
    if kind == 'long':
        D = 4
        mean = 50.0 * np.arange(K)[:, None] * np.ones(D)
        logA = np.log(0.02 / max(K - 1, 1) * np.ones((K, K)) + (0.98 - 0.02 / max(K - 1, 1)) * np.eye(K))
        z = np.zeros((B, N + 1), dtype=int)
        for n in range(1, N + 1):
            stay = rs.rand(B) < 0.98
            z[:, n] = np.where(stay, z[:, n - 1], rs.randint(K, size=B))
        y = mean[z] + rs.randn(B, N + 1, D)
        ev = -0.5 * np.sum((y[:, :, None, :] - mean) ** 2, -1) - 0.5 * D * np.log(2 * np.pi)
        return np.log(1.0 / K) + ev[:, 0], logA + ev[:, 1:, None, :]
    raise ValueError(kind)


def emulate_joint_shift(logp0, logP):
    """float64 arithmetic of a forward-backward pass that shifts every K x K slice by its JOINT
    maximum before it forms logalpha and logbeta (what the kernel did before it shifted per
    column and per row): the counter-example of the CPU tests."""
    logp0, logP = np.asarray(logp0, dtype=np.float64), np.asarray(logP, dtype=np.float64)
    N, K = logP.shape[-3], logp0.shape[-1]
    la = np.empty((N, K))
    la[0] = logp0
    g = 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        for n in range(N):
            v = la[n][:, None] + logP[n]
            s = np.exp(v - v.max()).sum(0)
            g -= v.max() + np.log(s.sum())
            if n + 1 < N:
                la[n + 1] = np.log(s) - np.log(s.sum())
        zz = np.empty((N, K, K))
        lb = np.zeros(K)
        for n in range(N - 1, -1, -1):
            w = la[n][:, None] + lb[None, :] + logP[n]
            e = np.exp(w - w.max())
            zz[n] = e / e.sum()
            v = lb[None, :] + logP[n]
            r = np.exp(v - v.max()).sum(1)
            lb = np.log(r) - np.log(r.sum())
    z0 = zz[0].sum(-1)
    return z0 / z0.sum(), zz, g
