"""TEST INFRASTRUCTURE: the multinomial-mixture (count-vector clustering) model scripts that run,
statement for statement, on the reference (tools/make_golden_mmm.py -> tests/golden/mmm.npz) and on
this framework (tests/test_mmm_host.py, tests/test_mmm_gpu.py).

``mods``: dict(nodes=<module with Dirichlet, Categorical, Multinomial, Mixture>, VB=<class>,
vb_kwargs=<dict, optional>, after_vb=<callable(Q), optional>).  The number of trials is one scalar
per case: the reference compares the row sums of x with ``n`` as it stands beside the cluster axis,
which only a scalar passes."""
import numpy as np

N_ITER = 12
CASES = ('a', 'b', 'c', 'd', 'e', 'f')
# case -> the case whose data it runs on
SOURCE = dict(a='a', b='a', c='a', d='a', e='e', f='f')


def make_mmm_inputs(rs):
    g = {}

    def data(tag, N, M, K, n, conc, near=0.0):
        p = rs.dirichlet(conc * np.ones(M), size=K)
        z = rs.randint(K, size=N)
        g[tag + '_x'] = np.array([rs.multinomial(n, p[k]) for k in z], dtype=np.int64)
        g[tag + '_n'] = np.array(n)
        g[tag + '_p0'] = near * p + (1.0 - near) * rs.dirichlet(2.0 * np.ones(M), size=K)
        g[tag + '_z0'] = rs.randint(K, size=N)
    data('a', 300, 7, 3, 40, 1.0)       # (a) - (d) share it
    # large totals: the coefficient and the 16-bit range matter; p0 near the truth keeps both clusters
    data('e', 40, 6, 2, 9000, 0.5, near=0.6)
    data('f', 50, 5, 1, 25, 1.0)        # K = 1
    g['c_alpha_p'] = rs.gamma(2.0, 2.0, size=(3, 7)) + 0.1
    g['c_alpha_r'] = rs.gamma(2.0, 2.0, size=3) + 0.1
    g['d_conc_p'] = rs.gamma(2.0, 0.5, size=(3, 7)) + 0.1
    g['d_conc_r'] = np.array([0.5, 1.0, 2.0])
    return g


def build_mmm(mods, x, n, K, conc_p=None, conc_r=None, observe=True):
    N_ = mods['nodes']
    N, M = np.shape(x)
    R = N_.Dirichlet(np.ones(K) if conc_r is None else conc_r, name='R')
    Z = N_.Categorical(R, plates=(N,), name='Z')
    P = N_.Dirichlet(0.5 * np.ones(M) if conc_p is None else conc_p, plates=(K,), name='P')
    X = N_.Mixture(Z, N_.Multinomial, n, P, name='X')
    if observe:
        X.observe(x)
    return dict(R=R, Z=Z, P=P, X=X)


def run_mmm_cases(mods, g, only=None, n_iter=N_ITER):
    """Per case: <tag>_L, <tag>_<node>_Lterm for R, Z, P, X, <tag>_R_u0, <tag>_P_u0 and
    <tag>_Z_u0; the engine itself as <tag>_plan.
      (a) default initialisations, Z from a value (P is updated first);
      (b) P from a value;  (c) P and R from parameters;
      (d) non-uniform concentrations of P and R, P from a value;
      (e) totals of 9000 with a count above 3000;  (f) K = 1, nothing initialised."""
    out = {}
    for tag in CASES:
        if only is not None and tag not in only:
            continue
        src = SOURCE[tag]
        x, n, p0 = g[src + '_x'], int(g[src + '_n']), g[src + '_p0']
        K = p0.shape[0]
        if tag == 'd':
            m = build_mmm(mods, x, n, K, conc_p=g['d_conc_p'], conc_r=g['d_conc_r'])
        else:
            m = build_mmm(mods, x, n, K)
        R, Z, P, X = m['R'], m['Z'], m['P'], m['X']
        if tag == 'a':
            Z.initialize_from_value(g['a_z0'])
        elif tag == 'c':
            P.initialize_from_parameters(g['c_alpha_p'])
            R.initialize_from_parameters(g['c_alpha_r'])
        elif tag != 'f':
            P.initialize_from_value(p0)
        Q = mods['VB'](Z, R, X, P, **mods.get('vb_kwargs', {}))
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        Q.ignore_bound_checks = True
        if tag == 'a':
            Q.update(P, Z, R, repeat=n_iter, verbose=False)
        else:
            Q.update(repeat=n_iter, verbose=False)
        out[tag + '_L'] = np.array(Q.L[:n_iter])
        for nm in ('R', 'Z', 'P', 'X'):
            out['%s_%s_Lterm' % (tag, nm)] = np.array(Q.l[m[nm]][:n_iter])
        out[tag + '_R_u0'] = np.array(R.get_moments()[0])
        out[tag + '_P_u0'] = np.array(P.get_moments()[0])
        out[tag + '_Z_u0'] = np.array(Z.get_moments()[0])
        out[tag + '_plan'] = Q
    return out
