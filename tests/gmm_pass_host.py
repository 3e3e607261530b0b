"""TEST INFRASTRUCTURE for the fused full-covariance Gaussian-mixture block (csrc/vmp_gmm.hip,
vmp_gmm_wide.hip): plain NumPy restatements of every kernel of the block in a dtype of the
caller's choice -- long double is the yardstick, float64 is the reference's own arithmetic and
recipe (mixture.py:53-293, utils/misc.py:1388-1401 with its second renormalisation,
gaussian.py:649-706, wishart.py:153-188, dirichlet.py:150-152, expfamily.py:400-480) -- and the
seeded inputs of tests/test_gmm_pass_host.py and tests/test_gmm_pass_gpu.py.  No tiles, no
grids, no tables: what a kernel computes, not how.  The allowance of a comparison is
``dgmm_host.tolerances``.  It lives under tests/ and is never imported by the
product."""
import numpy as np

from dgmm_host import _special, tolerances, error     # noqa: F401  (one copy, shared)

PASS_QUANTITIES = ('r', 'R', 'S1', 'S2', 'sum_lse', 'rphi')


# -- the compact feature list ------------------------------------------------------------------------
def n_pairs(D):
    return D * (D + 1) // 2


def n_features(D):
    """pairs y_a y_b (a <= b, row-major over a), then y_d, then 1."""
    return n_pairs(D) + D + 1


def pair_index(D):
    """(a, b) of the pair features in their order."""
    a, b = np.triu_indices(D)
    return a, b


def features(y, F2P, dtype=np.longdouble):
    """(N, F2P): the compact features of the rows of y, the padded ones 0."""
    y = np.asarray(y, dtype=dtype)
    N, D = y.shape
    a, b = pair_index(D)
    out = np.zeros((N, F2P), dtype=dtype)
    out[:, :n_pairs(D)] = y[:, a] * y[:, b]
    out[:, n_pairs(D):n_pairs(D) + D] = y
    out[:, n_pairs(D) + D] = 1
    return out


def natural(T, D):
    """Compact statistics (K, F2P) as R (K), S1 (K, D) and the full symmetric S2 (K, D, D)."""
    K = T.shape[0]
    a, b = pair_index(D)
    npair = n_pairs(D)
    S2 = np.zeros((K, D, D), dtype=T.dtype)
    S2[:, a, b] = T[:, :npair]
    S2[:, b, a] = T[:, :npair]
    return T[:, npair + D].copy(), T[:, npair:npair + D].copy(), S2


# -- inputs ---------------------------------------------------------------------------------------
def spd(rs, D, cond):
    """SPD with the given condition number from a seeded rotation, largest eigenvalue 1."""
    q, _ = np.linalg.qr(rs.normal(size=(D, D)))
    e = np.exp(-rs.uniform(0.0, np.log(cond), size=D))
    e[0] = 1.0
    if D > 1:
        e[-1] = 1.0 / cond
    a = (q * e) @ q.T
    return 0.5 * (a + a.T)


def make_inputs(N, D, K, seed=None):
    """y (N, D), Lam, Cmu (K, D, D), mu (K, D), logdetLam, logpi (K), labels (N) and priors.

    The centre of a cluster is a vector of D normals scaled by 3 / sqrt(D), so two centres lie
    about four units apart at every D and neighbouring clusters overlap: the rows of r are soft
    (the reasoning of dgmm_host.make_inputs; with well separated clusters the rows are one-hot
    and neither the exponential nor sum lse nor <C, T> is exercised).  <Lambda_k> is SPD with a
    condition number of 300 and eigenvalues of at most one (the precision of a broad posterior,
    which keeps the quadratic forms of neighbours within a few units), the other moments are
    those of plausible posteriors: means near the centres, covariances of the means of a few
    hundredths, <log|Lambda|> a little below log|<Lambda>|, <log pi> from Dirichlet counts."""
    from scipy.special import digamma
    rs = np.random.RandomState(7919 + 1000 * K + 10 * D + N if seed is None else seed)
    centre = 3.0 * rs.normal(size=(K, D)) / np.sqrt(D)
    z = rs.randint(K, size=N)
    y = rs.normal(size=(N, D)) + centre[z]
    Lam = np.stack([spd(rs, D, 300.0) for _ in range(K)])
    mu = centre + 0.1 * rs.normal(size=(K, D))
    Cmu = np.stack([spd(rs, D, 10.0) for _ in range(K)]) / rs.uniform(20.0, 200.0, size=(K, 1, 1))
    logdetLam = np.linalg.slogdet(Lam)[1] - rs.uniform(0.05, 0.5, size=K)
    alpha = rs.gamma(5.0, 10.0, size=K)
    logpi = digamma(alpha) - digamma(alpha.sum())
    return dict(y=y, Lam=Lam, mu=mu, Cmu=Cmu, logdetLam=logdetLam, logpi=logpi,
                labels=z.astype(np.int64), alpha0=rs.uniform(0.5, 2.0, size=K), beta0=0.7,
                n0=D + 2.0, V0=spd(rs, D, 1e3))


# -- z: the coefficient matrix and the pass ---------------------------------------------------------
def restate_C(Lam, mu, Cmu, logdetLam, logpi, KP, F2P, prior_only=False, dtype=np.longdouble):
    """(KP, F2P) coefficients of ell_nk = c_k + (Lam_k mu_k) . y - 1/2 y^T Lam_k y over the compact
    features: -1/2 Lam_aa, -1/2 (Lam_ab + Lam_ba), Lam mu, <log pi_k> + c_k with
    c_k = 1/2 <log|Lam_k|> - D/2 log 2 pi - 1/2 tr(Lam_k <mu mu^T>); prior_only: <log pi> alone.
    Padded clusters: 0 and -inf in the constant column; padded features: 0."""
    Lam, mu, Cmu, logdetLam, logpi = (np.asarray(a, dtype=dtype)
                                      for a in (Lam, mu, Cmu, logdetLam, logpi))
    K, D = mu.shape
    a, b = pair_index(D)
    npair = n_pairs(D)
    half = dtype(1) / 2
    C = np.zeros((KP, F2P), dtype=dtype)
    C[K:, npair + D] = -np.inf
    if prior_only:
        C[:K, npair + D] = logpi
        return C
    C[:K, :npair] = np.where(a == b, -half * Lam[:, a, a], -half * (Lam[:, a, b] + Lam[:, b, a]))
    C[:K, npair:npair + D] = np.einsum('kij,kj->ki', Lam, mu)
    mm = Cmu + mu[:, :, None] * mu[:, None, :]
    two_pi = 8 * np.arctan(dtype(1))
    C[:K, npair + D] = logpi + (half * logdetLam - half * D * np.log(two_pi)
                                - half * np.einsum('kij,kij->k', Lam, mm))
    return C


def restate_pass(y, C, labels=None, dtype=np.longdouble):
    """The pass over y (N, D) with the coefficient rows C (K, >= F2) of the K real clusters, the
    way mixture.py / categorical.py evaluate it: phi = C feat, r = normalized_exp(phi) (log-sum-exp
    about the row maximum, exp, and the second renormalisation), T = r^T feat.  dict of r (N, K),
    lse (N), T (K, F2P compact), R, S1, S2 (natural), sum_lse, rphi = sum r phi over r != 0
    (expfamily.py:455-460) and rphi_mag = sum |C T| over T != 0, the condition of <C, T>.
    labels: r is their one-hot (categorical.py:30-46); sum_lse and rphi are None."""
    y = np.asarray(y, dtype=dtype)
    C = np.asarray(C, dtype=dtype)
    N, D = y.shape
    K, F2P = C.shape
    F2 = n_features(D)
    feat = features(y, F2P, dtype)
    out = {}
    if labels is None:
        with np.errstate(invalid='ignore'):
            phi = feat[:, :F2] @ C[:, :F2].T
        m = phi.max(axis=1, keepdims=True)
        lse = np.log(np.exp(phi - m).sum(axis=1, keepdims=True)) + m
        r = np.exp(phi - lse)
        r = r / r.sum(axis=1, keepdims=True)
        nz = r != 0
        out.update(lse=lse[:, 0], sum_lse=lse.sum(),
                   rphi=np.sum(r[nz] * phi[nz]) if nz.any() else dtype(0))
    else:
        r = np.zeros((N, K), dtype=dtype)
        r[np.arange(N), np.asarray(labels)] = 1
        out.update(lse=None, sum_lse=None, rphi=None)
    T = r.T @ feat
    R, S1, S2 = natural(T, D)
    tz = T != 0
    mag = np.sum(np.abs(C[tz] * T[tz])) if tz.any() else dtype(0)
    out.update(r=r, T=T, R=R, S1=S1, S2=S2, rphi_mag=mag)
    return out


def pass_tolerances(ld, f64, keys=PASS_QUANTITIES):
    """``tolerances`` of the pass; the floor of rphi is 4 ulp of sum |C T| (the size of the terms
    of the contraction the design forms it by), not of |rphi|."""
    tol, dev = tolerances(ld, f64, keys)
    if 'rphi' in keys:
        tol['rphi'] = max(tol['rphi'], 4 * float(np.spacing(float(ld['rphi_mag']))))
    return tol, dev


# -- the per-cluster kernels -----------------------------------------------------------------------
def spd_inverse(A, dtype=np.longdouble):
    """Inverse and log-determinant of the SPD matrices A (K, D, D) by Gauss-Jordan sweeps over
    the pivots in order (NumPy's inv is float64 only); a pivot <= 0 gives NaN, no exception."""
    M = np.array(A, dtype=dtype)
    K, D, _ = M.shape
    logdet = np.zeros(K, dtype=dtype)
    with np.errstate(invalid='ignore', divide='ignore'):
        for p in range(D):
            piv = M[:, p, p].copy()
            logdet += np.log(piv)
            d = 1 / piv
            col, row = M[:, :, p].copy(), M[:, p, :].copy()
            M -= col[:, :, None] * row[:, None, :] * d[:, None, None]
            M[:, p, :] = row * d[:, None]
            M[:, :, p] = -col * d[:, None]
            M[:, p, p] = d
    return M, logdet


def _multidigamma(a, D, dtype):
    psi, _ = _special(dtype)
    half = dtype(1) / 2
    return psi(np.asarray(a, dtype=dtype)[:, None] - half * np.arange(D).astype(dtype)).sum(axis=1)


def _multigammaln(a, D, dtype):
    _, lgam = _special(dtype)
    half = dtype(1) / 2
    pi = 4 * np.arctan(dtype(1))
    return (dtype(D * (D - 1)) / 4 * np.log(pi)
            + lgam(np.asarray(a, dtype=dtype)[:, None] - half * np.arange(D).astype(dtype)).sum(axis=1))


def _lambda_moments(nk, V, D, dtype):
    Vs = (V + np.swapaxes(V, 1, 2)) / 2
    inv, logdetV = spd_inverse(Vs, dtype)
    Lam = nk[:, None, None] * inv                                           # wishart.py:184
    logdetLam = _multidigamma(nk / 2, D, dtype) + D * np.log(dtype(2)) - logdetV
    return Lam, logdetV, logdetLam


def restate_init(alpha0, beta0, n0, V0, dtype=np.longdouble):
    """Every node at its prior (expfamily.py:168-184)."""
    psi, _ = _special(dtype)
    alpha0, V0 = np.asarray(alpha0, dtype=dtype), np.asarray(V0, dtype=dtype)
    beta0, n0 = dtype(beta0), dtype(n0)
    K, D = len(alpha0), len(V0)
    nk = np.full(K, n0, dtype=dtype)
    Vk = np.tile(V0, (K, 1, 1))
    Lam, logdetV, logdetLam = _lambda_moments(nk, Vk, D, dtype)
    return dict(alpha=alpha0.copy(), logpi=psi(alpha0) - psi(alpha0.sum()[None])[0], nk=nk, Vk=Vk,
                mu=np.zeros((K, D), dtype=dtype),
                Cmu=np.tile(np.identity(D, dtype=dtype) / beta0, (K, 1, 1)),
                logdetLmu=np.full(K, D * np.log(beta0), dtype=dtype), Lam=Lam, logdetV=logdetV,
                logdetLam=logdetLam, logdetV0=logdetV[:1].copy())


def restate_update_mu(R, S1, Lam, beta0, dtype=np.longdouble):
    """Lambda_mu = beta0 I + R <Lambda>, Cov = its inverse, mean = Cov <Lambda> S1."""
    R, S1, Lam = (np.asarray(a, dtype=dtype) for a in (R, S1, Lam))
    D = S1.shape[1]
    Lmu = dtype(beta0) * np.identity(D, dtype=dtype) + R[:, None, None] * Lam
    Cmu, logdetLmu = spd_inverse(Lmu, dtype)
    mu = np.einsum('kij,kj->ki', Cmu, np.einsum('kij,kj->ki', Lam, S1))
    return dict(mu=mu, Cmu=Cmu, logdetLmu=logdetLmu)


def restate_update_lambda(R, S1, S2, mu, Cmu, n0, V0, dtype=np.longdouble):
    """n_k = n0 + R, V_k = V0 + S2 - S1 mu^T - mu S1^T + R <mu mu^T> (stored as formed; the
    moments are those of its symmetric part)."""
    R, S1, S2, mu, Cmu, V0 = (np.asarray(a, dtype=dtype) for a in (R, S1, S2, mu, Cmu, V0))
    D = S1.shape[1]
    mm = Cmu + mu[:, :, None] * mu[:, None, :]
    sm = S1[:, :, None] * mu[:, None, :]
    nk = dtype(n0) + R
    Vk = V0 + S2 - sm - np.swapaxes(sm, 1, 2) + R[:, None, None] * mm
    Lam, logdetV, logdetLam = _lambda_moments(nk, Vk, D, dtype)
    return dict(nk=nk, Vk=Vk, Lam=Lam, logdetV=logdetV, logdetLam=logdetLam)


def restate_update_alpha(alpha0, R, dtype=np.longdouble):
    psi, _ = _special(dtype)
    alpha = np.asarray(alpha0, dtype=dtype) + np.asarray(R, dtype=dtype)
    return dict(alpha=alpha, logpi=psi(alpha) - psi(alpha.sum()[None])[0])


BOUND_QUANTITIES = ('L_Y', 'L_z', 'L_alpha', 'L_mu', 'L_Lambda', 'L')


def restate_lower_bound(s, dtype=np.longdouble):
    """The five terms of expfamily.py:400-480 (Y, z, alpha, mu, Lambda) and their sum from a given
    state ``s``: R, S1, S2, sum_lse, rphi, alpha, logpi, mu, Cmu, logdetLmu, nk, Vk, Lam, logdetV,
    logdetLam and the priors alpha0, beta0, n0, V0."""
    _, lgam = _special(dtype)
    g = {k: np.asarray(v, dtype=dtype) for k, v in s.items() if k != 'y' and v is not None}
    R, S1, S2, Lam, mu, Cmu = g['R'], g['S1'], g['S2'], g['Lam'], g['mu'], g['Cmu']
    D = S1.shape[1]
    half = dtype(1) / 2
    two_pi = 8 * np.arctan(dtype(1))
    mm = Cmu + mu[:, :, None] * mu[:, None, :]
    c = half * g['logdetLam'] - half * D * np.log(two_pi) - half * np.einsum('kij,kij->k', Lam, mm)
    b = np.einsum('kij,kj->ki', Lam, mu)
    L_Y = np.sum(R * c) + np.sum(b * S1) - half * np.einsum('kij,kij->', Lam, S2)
    L_z = g['sum_lse'] - g['rphi'] + np.sum(R * g['logpi'])
    a0, a = g['alpha0'], g['alpha']
    L_a = (lgam(a0.sum()[None])[0] - lgam(a0).sum() - lgam(a.sum()[None])[0] + lgam(a).sum()
           + np.sum((a0 - a) * g['logpi']))
    beta0, n0, nk, V0 = g['beta0'], g['n0'], g['nk'], g['V0']
    L_mu = np.sum(-half * beta0 * np.einsum('kii->k', mm) + half * D * np.log(beta0)
                  - half * g['logdetLmu'] + half * D)
    _, logdetV0 = spd_inverse(V0[None], dtype)
    g_p = (half * n0 * logdetV0[0] - half * D * n0 * np.log(dtype(2))
           - _multigammaln(n0[None] / 2, D, dtype)[0])
    g_q = half * nk * g['logdetV'] - half * D * nk * np.log(dtype(2)) - _multigammaln(nk / 2, D, dtype)
    t = (-half * np.einsum('ij,kij->k', V0, Lam) + half * n0 * g['logdetLam']
         + half * np.einsum('kij,kij->k', g['Vk'], Lam) - half * nk * g['logdetLam'])
    L_L = np.sum(g_p - g_q + t)
    return dict(L_Y=L_Y, L_z=L_z, L_alpha=L_a, L_mu=L_mu, L_Lambda=L_L,
                L=L_Y + L_z + L_a + L_mu + L_L)


def cluster_tolerances(ld, f64, key):
    """``tolerances`` cluster by cluster (inverses and products of inverses: the magnitude of the
    floor is the largest element of that cluster's own matrix): (allowance (K,), deviation (K,))."""
    K = len(ld[key])
    out = [tolerances({key: ld[key][k]}, {key: f64[key][k]}, (key,)) for k in range(K)]
    return (np.array([t[key] for t, _ in out]), np.array([d[key] for _, d in out]))


def cluster_errors(val, ref):
    return np.array([error(val[k], ref[k]) for k in range(len(ref))])


# -- edge columns ----------------------------------------------------------------------------------
EDGE_SHAPES = ((8, 64), (16, 64), (32, 64))
EDGE_N, EDGE_DEAD, EDGE_TWINS, EDGE_FAR_ROW, EDGE_ZERO_ROW = 64, 7, (3, 40), 5, 9


def edge_inputs(D, K, KP, F2P):
    """(y, C (KP, F2P) float64) with: cluster EDGE_DEAD impossible (constant coefficient -inf),
    clusters EDGE_TWINS with identical rows of C (k = 3 and k = 40: one in each half of the
    pair-split form), row EDGE_FAR_ROW of y scaled by 40 (the spread of phi over k exceeds 800:
    the losers underflow to exact zeros) and row EDGE_ZERO_ROW all zero."""
    g = make_inputs(EDGE_N, D, K)
    C = restate_C(g['Lam'], g['mu'], g['Cmu'], g['logdetLam'], g['logpi'], KP, F2P,
                  dtype=np.float64)
    C[EDGE_DEAD, n_features(D) - 1] = -np.inf
    C[EDGE_TWINS[1]] = C[EDGE_TWINS[0]]
    y = g['y'].copy()
    y[EDGE_FAR_ROW] *= 40.0
    y[EDGE_ZERO_ROW] = 0.0
    return y, C
