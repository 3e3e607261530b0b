"""TEST INFRASTRUCTURE: hidden-Markov-model scripts with diagonal-Gaussian emissions that run,
statement for statement, on the reference (tools/make_golden_hmm_diag.py ->
tests/golden/hmm_diag.npz) and through engine='fused+diagonal' (tests/test_hmm_diag_gpu.py).

``mods``: dict(nodes=<module>, VB=<class>, vb_kwargs=<dict, optional>, after_vb=<callable(Q),
optional>), as in tests/hmm_cat_models.py."""
import numpy as np

from hmm_cat_models import trailing

N_ITER = 4
LEARNED = ('mu', 'tau', 'A', 'a0')

#       plates  T   K  D  Z from labels
CASES = dict(
    p=((3,), 9, 2, 5, False),           # a batch, everything from the prior
    q=((), 30, 3, 4, True),             # one chain with a mask (a hole, a ragged tail), Z from labels
)


def make_inputs(rs):
    g = {}
    for tag, (plates, T, K, D, labels) in CASES.items():
        A = rs.dirichlet(np.ones(K), size=K) * 0.3 + 0.7 * np.identity(K)
        means = 3.0 * rs.randn(K, D)
        z = np.empty(plates + (T,), dtype=np.int64)
        for idx in np.ndindex(*plates):
            s = rs.randint(K)
            for t in range(T):
                z[idx + (t,)] = s
                s = rs.choice(K, p=A[s])
        g[tag + '_y'] = means[z] + 0.7 * rs.randn(*plates + (T, D))
        g[tag + '_a0_prior'] = 0.5 + rs.gamma(1.0, size=K)
        g[tag + '_A_prior'] = 0.5 + rs.gamma(1.0, size=(K, K))
        # prior means per state, so that the states are told apart from the first sweep on
        g[tag + '_m0'], g[tag + '_beta0'] = means + rs.randn(K, D), np.array(0.1)
        g[tag + '_ta'], g[tag + '_tb'] = 1.0 + rs.rand(D), 1.0 + rs.rand(K, D)
        g[tag + '_z0'] = rs.randint(K, size=plates + (T,))
    m = trailing((24,), 30)[0]
    m[7:10] = False
    g['q_mask'] = m
    return g


def build(mods, g, tag, fill=None):
    N_ = mods['nodes']
    plates, T, K, D, _ = CASES[tag]
    a0 = N_.Dirichlet(g[tag + '_a0_prior'], name='a0')
    A = N_.Dirichlet(g[tag + '_A_prior'], name='A')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=plates, name='Z')
    mu = N_.GaussianARD(g[tag + '_m0'], g[tag + '_beta0'], shape=(D,), plates=(K,), name='mu')
    tau = N_.Gamma(g[tag + '_ta'], g[tag + '_tb'], plates=(K, D), name='tau')
    Y = N_.Mixture(Z, N_.GaussianARD, mu, tau, 1, name='Y')
    y = g[tag + '_y']
    if tag + '_mask' in g:
        mask = g[tag + '_mask']
        Y.observe(y if fill is None else np.where(mask[..., None], y, fill), mask=mask)
    else:
        Y.observe(y)
    return dict(a0=a0, A=A, mu=mu, tau=tau, Z=Z, Y=Y)


def run_cases(mods, g, only=None, n_iter=N_ITER, fill=None):
    """Per case: <tag>_L, <tag>_<node>_Lterm for Y, Z and the learned roles, <tag>_Z_u0 / _Z_u1,
    <tag>_<role>_u0 / _u1 of mu and tau, <tag>_<role>_u0 of A and a0, with a mask <tag>_Z_mask and
    <tag>_Y_mask; the engine itself as <tag>_plan and the nodes as <tag>_model."""
    out = {}
    for tag, (plates, T, K, D, labels) in CASES.items():
        if only is not None and tag not in only:
            continue
        m = build(mods, g, tag, fill=fill)
        if labels:
            m['Z'].initialize_from_value(g[tag + '_z0'])
        params = [m[nm] for nm in LEARNED]
        Q = mods['VB'](m['Y'], m['Z'], *params, **mods.get('vb_kwargs', {}))
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        Q.ignore_bound_checks = True
        if labels:
            Q.update(*params, m['Z'], repeat=n_iter, verbose=False)
        else:
            Q.update(repeat=n_iter, verbose=False)
        out[tag + '_L'] = np.array(Q.L[:n_iter])
        for nm in ('Y', 'Z') + LEARNED:
            out['%s_%s_Lterm' % (tag, nm)] = np.array(Q.l[m[nm]][:n_iter])
        for nm in ('Z', 'mu', 'tau'):
            u = m[nm].get_moments()
            out['%s_%s_u0' % (tag, nm)], out['%s_%s_u1' % (tag, nm)] = np.array(u[0]), np.array(u[1])
        for nm in ('A', 'a0'):
            out['%s_%s_u0' % (tag, nm)] = np.array(m[nm].get_moments()[0])
        if tag + '_mask' in g:
            for nm in ('Z', 'Y'):
                out['%s_%s_mask' % (tag, nm)] = np.array(
                    np.broadcast_to(m[nm].mask, m[nm].plates), dtype=bool)
        out[tag + '_plan'] = Q
        out[tag + '_model'] = m
    return out
