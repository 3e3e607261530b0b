"""TEST INFRASTRUCTURE: the binomial-mixture (successes out of trials) model scripts that run,
statement for statement, on the reference (tools/make_golden_binm.py -> tests/golden/binm.npz) and on
this framework (tests/test_binm_host.py, tests/test_binm_gpu.py).

``mods``: dict(nodes=<module with Dirichlet, Categorical, Beta, Binomial, Mixture>, VB=<class>,
vb_kwargs=<dict, optional>, after_vb=<callable(Q), optional>).  Every case starts from a state that
breaks the symmetry between the clusters: ``P`` from a value or from parameters, or ``Z`` from
labels with ``P`` updated first."""
import numpy as np

N_ITER = 4
#   a  scalar n                       b  (a) with Z from labels, P updated first
#   c  n per column (D, 1), K = 1     d  n per entry (N, D, 1) with zeros
#   e  n per row (N, 1, 1) up to 3000, P from parameters
#   f  (d) with a full mask: a hidden row, a hidden column
#   g  (a) with a mask of ones        h  (a) with the scalar mask True
#   i  (a) with a mask (N, 1) that broadcasts over the columns
CASES = ('a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', 'i')
# case -> the case whose data it runs on
SOURCE = dict(a='a', b='a', c='c', d='d', e='e', f='d', g='a', h='a', i='a')
# the cases the fused block takes (it declines the masks of (h) and (i))
FUSED_CASES = ('a', 'b', 'c', 'd', 'e', 'f', 'g')


def make_binm_inputs(rs):
    g = {}

    def data(tag, N, D, K, n):
        p = rs.beta(1.5, 1.5, size=(K, D))
        z = rs.randint(K, size=N)
        n = np.asarray(n, dtype=np.int64)
        nb = np.broadcast_to(n.reshape((1,) * (3 - n.ndim) + n.shape)[..., 0], (N, D))
        g[tag + '_x'] = rs.binomial(nb, p[z]).astype(np.int64)
        g[tag + '_n'] = n
        g[tag + '_p0'] = rs.beta(2.0, 2.0, size=(D, K))
        g[tag + '_z0'] = rs.randint(K, size=(N, 1))
    data('a', 300, 7, 3, 12)                                        # scalar
    data('c', 50, 5, 1, rs.randint(1, 30, size=(5, 1)))             # per column, K = 1
    nd = rs.randint(0, 25, size=(60, 4, 1))                         # per entry, with zeros
    nd[3, 1, 0] = nd[7, :, 0] = 0
    data('d', 60, 4, 3, nd)
    data('e', 40, 6, 2, rs.randint(100, 3000, size=(40, 1, 1)))     # per row, lgamma matters
    g['a_alpha'] = np.array([0.5, 1.0, 2.0])
    g['a_ab0'] = rs.gamma(2.0, 0.5, size=(7, 3, 2)) + 0.1
    g['e_ab'] = rs.gamma(3.0, 2.0, size=(6, 2, 2)) + 0.5            # (e): P from parameters
    m = rs.rand(60, 4) < 0.7        # (f): about 70 % ones, a row and a column of nothing
    m[4], m[:, 2], m[11] = False, False, True
    m[11, 2] = False
    g['f_mask'] = m
    g['g_mask'] = np.ones((300, 7), dtype=bool)
    g['h_mask'] = np.array(True)
    g['i_mask'] = rs.rand(300, 1) < 0.8
    return g


def build_binm(mods, x, n, K, ab0=None, alpha=None, mask=None, observe=True):
    """The hidden entries of ``x`` are set to zero before ``observe``, which checks every value,
    hidden ones included, in the reference as here."""
    N_ = mods['nodes']
    N, D = np.shape(x)
    R = N_.Dirichlet(K * [1e-2] if alpha is None else alpha, name='R')
    Z = N_.Categorical(R, plates=(N, 1), name='Z')
    P = N_.Beta([0.5, 0.5] if ab0 is None else ab0, plates=(D, K), name='P')
    X = N_.Mixture(Z, N_.Binomial, n, P, name='X')
    if observe:
        if mask is None:
            X.observe(x)
        else:
            X.observe(np.where(mask, x, 0).astype(np.int64), mask=mask)
    return dict(R=R, Z=Z, P=P, X=X)


def run_binm_cases(mods, g, only=None, n_iter=N_ITER):
    """Per case: <tag>_L, <tag>_<node>_Lterm for R, Z, P, X, <tag>_R_u0, <tag>_P_u0, <tag>_Z_u0,
    <tag>_Z_mask and <tag>_P_mask; the engine itself as <tag>_plan."""
    out = {}
    for tag in CASES:
        if only is not None and tag not in only:
            continue
        src = SOURCE[tag]
        x, n, p0 = g[src + '_x'], g[src + '_n'], g[src + '_p0']
        K = p0.shape[1]
        mask = g[tag + '_mask'] if tag + '_mask' in g else None
        if mask is not None and mask.ndim == 0:
            mask = bool(mask)
        if src == 'a':
            m = build_binm(mods, x, n, K, ab0=g['a_ab0'], alpha=g['a_alpha'], mask=mask)
        else:
            m = build_binm(mods, x, n, K, mask=mask)
        R, Z, P, X = m['R'], m['Z'], m['P'], m['X']
        if tag == 'e':
            P.initialize_from_parameters(g['e_ab'])
        elif tag != 'b':
            P.initialize_from_value(p0)
        if tag == 'b':
            Z.initialize_from_value(g['a_z0'])
        Q = mods['VB'](Z, R, X, P, **mods.get('vb_kwargs', {}))
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        Q.ignore_bound_checks = True
        if tag == 'b':
            Q.update(P, Z, R, repeat=n_iter, verbose=False)
        else:
            Q.update(repeat=n_iter, verbose=False)
        out[tag + '_L'] = np.array(Q.L[:n_iter])
        for nm in ('R', 'Z', 'P', 'X'):
            out['%s_%s_Lterm' % (tag, nm)] = np.array(Q.l[m[nm]][:n_iter])
        out[tag + '_R_u0'] = np.array(R.get_moments()[0])
        out[tag + '_P_u0'] = np.array(P.get_moments()[0])
        out[tag + '_Z_u0'] = np.array(Z.get_moments()[0])
        out[tag + '_Z_mask'] = np.array(Z.mask)
        out[tag + '_P_mask'] = np.array(P.mask)
        out[tag + '_plan'] = Q
    return out
