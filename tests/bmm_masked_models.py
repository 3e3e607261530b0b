"""TEST INFRASTRUCTURE: the Bernoulli-mixture model scripts with missing observations
(doc/source/examples/bmm.rst with ``X.observe(x, mask=m)``) that run, statement for statement, on
the reference (tools/make_golden_bmm_masked.py -> tests/golden/bmm_masked.npz) and on this
framework (tests/test_bmm_masked_host.py, tests/test_bmm_masked_gpu.py).

``mods``: dict(nodes=<module with Dirichlet, Categorical, Beta, Mixture, Bernoulli>, VB=<class>,
vb_kwargs=<dict, optional>, after_vb=<callable(Q), optional>).  ``P`` is initialised from a value
in every case: from a symmetric prior with a Dirichlet concentration of 1e-5 the reference itself
reaches NaN after two sweeps."""
import numpy as np

N_ITER = 5
CASES = ('a', 'b', 'c', 'd', 'e')


def make_masked_inputs(rs, fused_inputs):
    """``fused_inputs``: the in_* arrays of tests/golden/bmm_fused.npz; its case a is the data of
    (a), (b) and (d).  Hidden entries of every x are NaN."""
    g = {}

    def hide(tag, x, m):
        g[tag + '_mask'] = m
        g[tag + '_x'] = np.where(m, x.astype(np.float64), np.nan)

    xa = fused_inputs['a_x']
    for k in ('a_p0', 'a_z0', 'a_alpha'):
        g[k] = fused_inputs[k]
    hide('a', xa, rs.rand(*xa.shape) < 0.7)                 # (a) and (b) share it
    hide('d', xa, np.ones(xa.shape, dtype=bool))            # a mask of ones
    # (c) D = 65: a row and a column of nothing, a fully observed row, a hidden bit in word 1
    N, D, K = 90, 65, 3
    p = rs.beta(0.4, 0.4, size=(K, D))
    x = (rs.rand(N, D) < p[rs.randint(K, size=N)]).astype(np.int64)
    m = rs.rand(N, D) < 0.7
    m[4], m[:, 9], m[11] = False, False, True
    m[11, 9], m[12, 64] = False, False
    hide('c', x, m)
    g['c_p0'] = rs.beta(0.5, 0.5, size=(D, K)).clip(1e-3, 1 - 1e-3)
    # (e) K = 1
    N, D = 50, 5
    x = (rs.rand(N, D) < rs.beta(0.4, 0.4, size=D)).astype(np.int64)
    hide('e', x, rs.rand(N, D) < 0.7)
    g['e_p0'] = rs.beta(0.5, 0.5, size=(D, 1)).clip(1e-3, 1 - 1e-3)
    return g


def build_bmm_masked(mods, x, mask, K, beta=(0.5, 0.5), alpha=None):
    """The hidden entries of ``x`` (NaN in the fixtures) are set to zero before ``observe``, which
    checks every value, hidden ones included, in the reference as here."""
    N_ = mods['nodes']
    N, D = np.shape(x)
    R = N_.Dirichlet(K * [1e-5] if alpha is None else alpha, name='R')
    Z = N_.Categorical(R, plates=(N, 1), name='Z')
    P = N_.Beta(list(beta), plates=(D, K), name='P')
    X = N_.Mixture(Z, N_.Bernoulli, P, name='X')
    X.observe(np.where(mask, x, 0).astype(np.int64), mask=mask)
    return dict(R=R, Z=Z, P=P, X=X)


def run_masked_cases(mods, g, only=None, n_iter=N_ITER):
    """Per case: <tag>_L, <tag>_<node>_Lterm for R, Z, P, X, <tag>_<node>_u0 for R, P, Z,
    <tag>_Z_mask and <tag>_P_mask; the engine itself as <tag>_plan."""
    out = {}
    for tag in CASES:
        if only is not None and tag not in only:
            continue
        src = 'a' if tag == 'b' else tag
        x, mask = g[src + '_x'], g[src + '_mask']
        p0 = g['a_p0'] if tag in ('a', 'b', 'd') else g[tag + '_p0']
        K = p0.shape[1]
        if tag in ('a', 'b', 'd'):
            m = build_bmm_masked(mods, x, mask, K, beta=(2.0, 0.5), alpha=g['a_alpha'])
        else:
            m = build_bmm_masked(mods, x, mask, K)
        R, Z, P, X = m['R'], m['Z'], m['P'], m['X']
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
        for nm in ('R', 'P', 'Z'):
            out['%s_%s_u0' % (tag, nm)] = np.array(m[nm].get_moments()[0])
        out[tag + '_Z_mask'] = np.array(Z.mask)
        out[tag + '_P_mask'] = np.array(P.mask)
        out[tag + '_plan'] = Q
    return out
