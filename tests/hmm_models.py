"""TEST INFRASTRUCTURE: the Gaussian hidden-Markov-model scripts (doc/source/examples/hmm.rst,
second half) that run, statement for statement, on the reference (tools/make_golden_hmm.py ->
tests/golden/hmm_fused.npz) and on this framework (tests/test_hmm_fused_host.py,
tests/test_hmm_fused_gpu.py), and the same scripts with missing observations and ragged sequence
lengths (``Y.observe(y, mask=m)``; tools/make_golden_hmm.py masked -> tests/golden/hmm_masked.npz,
tests/test_hmm_masked_host.py, tests/test_hmm_masked_gpu.py).  NaN stands at every masked position
of their ``y``.

``mods``: dict(nodes=<module with Dirichlet, CategoricalMarkovChain, Mixture, Gaussian, GaussianARD,
Wishart>,
VB=<class>, vb_kwargs=<dict, optional>, after_vb=<callable(Q), optional>)."""
import functools

import numpy as np

N_ITER = 4


def _data(g, rs, tag, plates, T, D, K, per_state):
    mu = 4.0 * rs.normal(size=(K, D))
    if per_state:
        W = rs.normal(size=(K, D, D + 2))
        Lam = np.einsum('kab,kcb->kac', W, W) / (D + 2)
    else:
        Lam = 0.5 * np.identity(D)
    z = rs.randint(K, size=plates + (T,))
    for t in range(1, T):                       # sticky chains
        stay = rs.rand(*plates) < 0.8
        z[..., t] = np.where(stay, z[..., t - 1], z[..., t])
    g[tag + '_y'] = mu[z] + rs.normal(size=plates + (T, D))
    g[tag + '_mu'], g[tag + '_Lambda'] = mu, Lam
    g[tag + '_z0'] = rs.randint(K, size=plates + (T,))


def make_hmm_inputs(rs):
    g = {}
    data = functools.partial(_data, g, rs)
    data('a', (), 60, 2, 3, False)         # one chain, the form of hmm.rst
    data('b', (7,), 12, 3, 4, True)        # a batch of chains, a precision per state; labels
    data('c', (3,), 2, 1, 1, False)        # T = 2, D = 1, K = 1
    data('d', (5,), 9, 2, 5, True)         # observed after VB(...)
    data('e', (6,), 15, 2, 3, False)       # learned emissions, fixed initial labels
    data('f', (), 30, 3, 2, False)         # learned emissions, one chain, Z from its prior
    g['b_a0'] = np.array([0.5, 1.0, 2.0, 1.5])
    g['b_A'] = rs.gamma(2.0, size=(4, 4))
    return g


CASES = ('a', 'b', 'c', 'd')
LEARNED = ('e', 'f')


def trailing(lengths, T):
    """(B, T) mask of sequences of the given lengths, padded at the end."""
    return np.arange(T)[None, :] < np.asarray(lengths)[:, None]


def make_masked_inputs(rs):
    g = {}
    data = functools.partial(_data, g, rs)
    # 1: one chain, constants, about 70 % observed, the first step masked
    data('a', (), 60, 2, 3, False)
    m = rs.rand(60) < 0.7
    m[0], m[1], m[-1] = False, True, True
    g['a_mask'] = m
    # 2: a batch, a precision per state, fixed initial labels; lengths as trailing masks, one
    # chain with nothing observed
    data('b', (7,), 12, 3, 4, True)
    g['b_mask'] = trailing((12, 9, 5, 1, 0, 12, 7), 12)
    g['b_a0'] = np.array([0.5, 1.0, 2.0, 1.5])
    g['b_A'] = rs.gamma(2.0, size=(4, 4))
    # 3: T = 2, D = 1, K = 1
    data('c', (3,), 2, 1, 1, False)
    g['c_mask'] = np.array([[1, 0], [0, 1], [0, 0]], dtype=bool)
    # 4: observed with a mask after VB(...), then with another mask of the same shape
    data('d', (5,), 9, 2, 5, True)
    g['d_mask0'] = rs.rand(5, 9) < 0.5
    m = rs.rand(5, 9) < 0.75
    m[2] = False                                    # nothing observed
    m[0, 0], m[1, -1] = False, False
    g['d_mask'] = m
    # 5: learned emissions, a batch with ragged tails and holes, fixed initial labels
    data('e', (6,), 15, 2, 3, False)
    m = trailing((15, 11, 8, 15, 4, 13), 15) & (rs.rand(6, 15) < 0.8)
    m[0, 0], m[3] = False, True
    g['e_mask'] = m
    # 6: learned emissions, one chain, Z from its prior
    data('f', (), 30, 3, 2, False)
    m = rs.rand(30) < 0.7
    m[-3:] = False
    g['f_mask'] = m
    g['d_y0'] = np.where(g['d_mask0'][..., None], g['d_y'], np.nan)
    for tag in CASES + LEARNED:
        g[tag + '_y'] = np.where(g[tag + '_mask'][..., None], g[tag + '_y'], np.nan)
    return g


def build_hmm(mods, y, mu, Lam, a0_prior=None, A_prior=None, observe=True, learned=False):
    """``learned``: mu and Lambda are nodes with the priors of the Gaussian-mixture block (the
    given arrays only fix K and D)."""
    N_ = mods['nodes']
    K = len(mu)
    if learned:
        D = np.shape(y)[-1]
        mu = N_.GaussianARD(0, 1e-2, shape=(D,), plates=(K,), name='mu')
        Lam = N_.Wishart(D + 1.0, np.identity(D), plates=(K,), name='Lambda')
    plates, T = np.shape(y)[:-2], np.shape(y)[-2]
    a0 = N_.Dirichlet(1e-3 * np.ones(K) if a0_prior is None else a0_prior, name='a0')
    A = N_.Dirichlet(1e-3 * np.ones((K, K)) if A_prior is None else A_prior, name='A')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=plates, name='Z')
    Y = N_.Mixture(Z, N_.Gaussian, mu, Lam, name='Y')
    if observe:
        Y.observe(y)
    return dict(a0=a0, A=A, Z=Z, Y=Y, mu=mu, Lambda=Lam)


def run_hmm_cases(mods, g, only=None, n_iter=N_ITER, device_mask=None):
    """Per case: <tag>_L, <tag>_<node>_Lterm for Y, Z, A, a0 (and mu, Lambda), <tag>_Z_u0 /
    _Z_u1, <tag>_A_u0 / <tag>_a0_u0 (and <tag>_mu_u0 / _mu_u1 / _Lambda_u0 / _Lambda_u1); the engine
    itself as <tag>_plan.  With the inputs of ``make_masked_inputs`` also <tag>_Z_mask and
    <tag>_Y_mask; ``device_mask``: callable that turns a host mask into what ``observe`` is given."""
    out = {}
    wrap = device_mask if device_mask is not None else (lambda m: m)
    for tag in CASES + LEARNED:
        if only is not None and tag not in only:
            continue
        kw = dict(a0_prior=g['b_a0'], A_prior=g['b_A']) if tag == 'b' else {}
        masked = tag + '_mask' in g
        m = build_hmm(mods, g[tag + '_y'], g[tag + '_mu'], g[tag + '_Lambda'], observe=False,
                      learned=tag in LEARNED, **kw)

        def observe(y, mask):
            m['Y'].observe(g[y], **(dict(mask=wrap(g[mask])) if masked else {}))
        if tag != 'd':
            observe(tag + '_y', tag + '_mask')
        if tag in ('b', 'e'):
            m['Z'].initialize_from_value(g[tag + '_z0'])
        more = (m['mu'], m['Lambda']) if tag in LEARNED else ()
        Q = mods['VB'](m['Y'], m['Z'], m['A'], m['a0'], *more, **mods.get('vb_kwargs', {}))
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        if tag == 'd':
            if masked:
                observe('d_y0', 'd_mask0')
            observe('d_y', 'd_mask')
        Q.ignore_bound_checks = True
        if tag == 'b':
            Q.update(m['A'], m['a0'], m['Z'], repeat=n_iter, verbose=False)
        elif tag in LEARNED:
            Q.update(m['mu'], m['Lambda'], m['A'], m['a0'], m['Z'], repeat=n_iter, verbose=False)
        else:
            Q.update(repeat=n_iter, verbose=False)
        out[tag + '_L'] = np.array(Q.L[:n_iter])
        for nm in ('Y', 'Z', 'A', 'a0') + (('mu', 'Lambda') if tag in LEARNED else ()):
            out['%s_%s_Lterm' % (tag, nm)] = np.array(Q.l[m[nm]][:n_iter])
        u = m['Z'].get_moments()
        out[tag + '_Z_u0'], out[tag + '_Z_u1'] = np.array(u[0]), np.array(u[1])
        out[tag + '_A_u0'] = np.array(m['A'].get_moments()[0])
        out[tag + '_a0_u0'] = np.array(m['a0'].get_moments()[0])
        if tag in LEARNED:
            for nm in ('mu', 'Lambda'):
                u = m[nm].get_moments()
                out['%s_%s_u0' % (tag, nm)], out['%s_%s_u1' % (tag, nm)] = np.array(u[0]), np.array(u[1])
        if masked:
            out[tag + '_Z_mask'] = np.array(np.broadcast_to(m['Z'].mask, m['Z'].plates), dtype=bool)
            out[tag + '_Y_mask'] = np.array(np.broadcast_to(m['Y'].mask, m['Y'].plates), dtype=bool)
        out[tag + '_plan'] = Q
    return out
