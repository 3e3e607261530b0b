"""State-space models whose GaussianMarkovChain is driven by input signals,
x_t = A x_{t-1} + B u_t + noise, shared (statement for statement) by the fixture generator
tools/make_golden_chain_in.py, which runs them on the reference, and the tests, which run them on
this package.  The layout is demos/lssm.py: Y = GaussianARD(SumMultiply(C, X), tau).

Cases (tag: inputs, [A | B], nu, sequences B, states D, inputs K, time instances N, observed M):
  a   constant inputs (N-1, K), constant [A | B] and nu; one chain, D = K = 1, N = 3
  b   constant inputs (B, N-1, K); node [A | B] with plates (D,), node nu (D,); B = 6
  c   as b with plates (N-1, D) on [A | B] and nu: time-varying dynamics with inputs
  d   as b with constant inputs (N-1, K) that every sequence shares
  e   as b with a node as the inputs, GaussianARD(0, 1, shape=(K,), plates=(B, N-1))
  f   N = 2 (the time plates are 1); [A | B] carries the sequence plate, plates (B, 1, D)
  g   as b with D = 12, K = 16 (the kernel's largest input dimension); means only stored
"""
import numpy as np

SWEEPS = 5

#        tag   B     D   K   N   M
CASES = (('a', None, 1, 1, 3, 2),
         ('b', 6, 2, 3, 10, 5),
         ('c', 6, 2, 3, 10, 5),
         ('d', 6, 2, 3, 10, 5),
         ('e', 6, 2, 3, 10, 5),
         ('f', 4, 2, 2, 2, 4),
         ('g', 5, 12, 16, 6, 14))
TAGS = tuple(c[0] for c in CASES)
# the cases whose moments are stored in full (the large one keeps the means only)
FULL_MOMENTS = ('a', 'b', 'c', 'd', 'e', 'f')
# the reference's own closed-form case (its test_gaussian_markov_chain.py:664-680)
CLOSED_FORM = dict(mu=2.0, Lambda=3.0, A=4.0, B=5.0, v=6.0, inputs=[[-2.0], [3.0]])


def case(tag):
    return [c for c in CASES if c[0] == tag][0]


def make_chain_in_inputs(rs):
    g = {}
    for tag, B, D, K, N, M in CASES:
        pl = () if B is None else (B,)
        g[tag + '_y'] = rs.normal(size=(M,) + pl + (N,)) + np.sin(0.7 * np.arange(N))
        g[tag + '_x0'] = rs.normal(size=pl + (N, D))
        g[tag + '_c0'] = rs.normal(size=(M,) + (1,) * (len(pl) + 1) + (D,))
        upl = (N - 1,) if tag in ('a', 'd') else pl + (N - 1,)
        g[tag + '_u'] = rs.normal(size=upl + (K,)) + np.cos(0.4 * np.arange(N - 1))[:, None]
    g['a_AB'] = np.array([[0.8, 0.5]])
    g['a_nu'] = np.array([1.5])
    return g


def build_chain_in(nodes_mod, vb_cls, g, tag, expand_shared_inputs=False, **vb_kwargs):
    """(Q, tracked nodes by name) of case ``tag``.  ``expand_shared_inputs``: the inputs that the
    sequences of case d share are handed over as B equal copies, (B, N-1, K) -- the same model; the
    reference cannot take the shared form (it concatenates the blocks of its message to [A | B]
    without broadcasting them, gaussian_markov_chain.py:495-498), so the generator sets this."""
    N_ = nodes_mod
    _, B, D, K, N, M = case(tag)
    y, x0, c0, u = g[tag + '_y'], g[tag + '_x0'], g[tag + '_c0'], g[tag + '_u']
    pl = () if B is None else (B,)
    track = {}
    extra = []
    if tag == 'a':
        A, nu = g['a_AB'], g['a_nu']
        n = None                          # inferred from the N-1 plate of the inputs
    else:
        if tag == 'c':
            Apl = nupl = (N - 1, D)
        elif tag == 'f':
            Apl, nupl = (B, 1, D), (D,)
        else:
            Apl = nupl = (D,)
        alpha = N_.Gamma(1e-5, 1e-5, plates=(D + K,), name='alpha')
        A = N_.GaussianARD(0, alpha, shape=(D + K,), plates=Apl, name='A')
        a0 = np.concatenate([0.9 * np.identity(D), 0.1 * np.ones((D, K))], axis=-1)
        A.initialize_from_value(np.broadcast_to(a0, Apl + (D + K,)).copy())
        nu = N_.Gamma(1e-3, 1e-3, plates=nupl, name='nu')
        n = N
        track.update(A=A, alpha=alpha, nu=nu)
        extra = [A, alpha, nu]
    if tag == 'e':
        U = N_.GaussianARD(0, 1, shape=(K,), plates=pl + (N - 1,), name='U')
        U.initialize_from_value(u)
        track.update(U=U)
        extra = extra + [U]
    elif tag == 'd' and expand_shared_inputs:
        U = np.broadcast_to(u, pl + u.shape).copy()
    else:
        U = u
    # (the initial mean carries the sequence plate: the reference sizes phi0 by the plates of mu and
    # of [A | B] alone, gaussian_markov_chain.py:589-600, so inputs with a sequence plate need one)
    X = N_.GaussianMarkovChain(np.zeros(pl + (D,)), 1e-3 * np.identity(D), A, nu, n=n, inputs=U,
                               plates=pl, name='X')
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


def run_chain_in_case(nodes_mod, vb_cls, g, tag, expand_shared_inputs=False, **vb_kwargs):
    """The bound after each sweep, the per-node bound terms and the final moments of case ``tag``."""
    Q, track = build_chain_in(nodes_mod, vb_cls, g, tag, expand_shared_inputs, **vb_kwargs)
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
