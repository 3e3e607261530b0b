"""State-space models whose GaussianMarkovChain has time-varying dynamics A_t and / or innovation
precisions nu_t, shared (statement for statement) by the fixture generator
tools/make_golden_chain_tv.py, which runs them on the reference, and the tests, which run them on
this package.  The layout is demos/lssm.py: Y = GaussianARD(SumMultiply(C, X), tau).

Cases (tag: A, nu, sequences B, states D, time instances N, observed dimensions M):
  a     constant arrays A (N-1, D, D), nu (N-1, D); one chain
  b2 / b4 / b12   nodes A, nu with plates (N-1, D); B = 6; D = 2, 4, 12
  cA    node A (N-1, D), node nu (D,): only the dynamics vary        cnu   the reverse
  d     node A with plates (6, N-1, D): the dynamics carry the sequence plate too
  e     N = 2 (the time plate is 1)
"""
import numpy as np

SWEEPS = 5

#        tag     B     D   N   M
CASES = (('a', None, 3, 12, 4),
         ('b2', 6, 2, 10, 5),
         ('b4', 6, 4, 10, 5),
         ('b12', 6, 12, 8, 14),
         ('cA', 6, 2, 9, 4),
         ('cnu', 6, 2, 9, 4),
         ('d', 6, 2, 7, 4),
         ('e', 6, 3, 2, 4))
TAGS = tuple(c[0] for c in CASES)
# the cases whose moments are stored in full (the large ones keep the means only)
FULL_MOMENTS = ('a', 'b2', 'd', 'e')


def make_chain_tv_inputs(rs):
    g = {}
    for tag, B, D, N, M in CASES:
        pl = () if B is None else (B,)
        g[tag + '_y'] = rs.normal(size=(M,) + pl + (N,)) + np.sin(0.7 * np.arange(N))
        g[tag + '_x0'] = rs.normal(size=pl + (N, D))
        g[tag + '_c0'] = rs.normal(size=(M,) + (1,) * (len(pl) + 1) + (D,))
    D, N = 3, 12
    # constant, time-varying dynamics of case a: slowly turning contractions and drifting precisions
    ang = 0.3 + 0.05 * np.arange(N - 1)
    A = np.zeros((N - 1, D, D))
    A[:, 0, 0], A[:, 0, 1], A[:, 1, 0], A[:, 1, 1] = np.cos(ang), -np.sin(ang), np.sin(ang), np.cos(ang)
    A[:, 2, 2] = 0.5 + 0.04 * np.arange(N - 1)
    g['a_A'] = 0.9 * A + 0.05 * rs.normal(size=(N - 1, D, D))
    g['a_nu'] = np.exp(0.3 * rs.normal(size=(N - 1, D))) * np.linspace(0.5, 2.0, N - 1)[:, None]
    return g


def build_chain_tv(nodes_mod, vb_cls, g, tag, **vb_kwargs):
    """(Q, tracked nodes by name) of case ``tag``."""
    N_ = nodes_mod
    _, B, D, N, M = [c for c in CASES if c[0] == tag][0]
    y, x0, c0 = g[tag + '_y'], g[tag + '_x0'], g[tag + '_c0']
    pl = () if B is None else (B,)
    track = {}
    extra = []
    if tag == 'a':
        A, nu = g['a_A'], g['a_nu']
        n = None                          # inferred from the N-1 plate of the arrays
    else:
        if tag == 'cnu':
            Apl = (D,)
        elif tag == 'd':
            Apl = (B, N - 1, D)
        else:
            Apl = (N - 1, D)
        nupl = (D,) if tag == 'cA' else (N - 1, D)
        alpha = N_.Gamma(1e-5, 1e-5, plates=(D,), name='alpha')
        A = N_.GaussianARD(0, alpha, shape=(D,), plates=Apl, name='A')
        A.initialize_from_value(np.broadcast_to(0.9 * np.identity(D), Apl + (D,)).copy())
        nu = N_.Gamma(1e-3, 1e-3, plates=nupl, name='nu')
        n = N
        track.update(A=A, alpha=alpha, nu=nu)
        extra = [A, alpha, nu]
    X = N_.GaussianMarkovChain(np.zeros(D), 1e-3 * np.identity(D), A, nu, n=n, plates=pl, name='X')
    X.initialize_from_value(x0)
    gamma = N_.Gamma(1e-5, 1e-5, plates=(D,), name='gamma')
    gamma.initialize_from_value(1e-2 * np.ones(D))
    C = N_.GaussianARD(0, gamma, shape=(D,), plates=(M,) + (1,) * (len(pl) + 1), name='C')
    C.initialize_from_value(c0)
    tau = N_.Gamma(1e-5, 1e-5, name='tau')
    tau.initialize_from_value(1e2)
    F = N_.SumMultiply('i,i', C, X, name='F')
    Y = N_.GaussianARD(F, tau, name='Y')
    Y.observe(y)
    Q = vb_cls(Y, F, C, gamma, X, *(extra + [tau]), **vb_kwargs)
    Q.ignore_bound_checks = True
    track.update(X=X, C=C, gamma=gamma, tau=tau)
    return Q, track


def run_chain_tv_case(nodes_mod, vb_cls, g, tag, **vb_kwargs):
    """The bound after each sweep, the per-node bound terms and the final moments of case ``tag``."""
    Q, track = build_chain_tv(nodes_mod, vb_cls, g, tag, **vb_kwargs)
    Q.update(repeat=SWEEPS, verbose=False)
    out = {tag + '_L': np.array(Q.L[:SWEEPS])}
    for nm, nd in track.items():
        out['%s_%s_L' % (tag, nm)] = np.array(Q.l[nd][:SWEEPS])
        u = [np.array(v) for v in (nd.u if hasattr(nd, 'u') else nd.get_moments())]
        if tag not in FULL_MOMENTS:
            u = u[:1]
        for i, ui in enumerate(u):
            out['%s_%s_u%d' % (tag, nm, i)] = ui
    return out
