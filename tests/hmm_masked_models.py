"""TEST INFRASTRUCTURE: the Gaussian hidden-Markov-model scripts of tests/hmm_models.py with missing
observations and ragged sequence lengths (``Y.observe(y, mask=m)``), run statement for statement on
the reference (tools/make_golden_hmm_masked.py -> tests/golden/hmm_masked.npz) and on this framework
(tests/test_hmm_masked_host.py, tests/test_hmm_masked_gpu.py).  NaN stands at every masked position
of ``y``.

``mods``: as in tests/hmm_models.py."""
import numpy as np

from hmm_models import build_hmm

N_ITER = 4

CASES = ('a', 'b', 'c', 'd')
LEARNED = ('e', 'f')


def trailing(lengths, T):
    """(B, T) mask of sequences of the given lengths, padded at the end."""
    return np.arange(T)[None, :] < np.asarray(lengths)[:, None]


def make_masked_inputs(rs):
    g = {}

    def data(tag, plates, T, D, K, per_state):
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


def run_masked_cases(mods, g, only=None, n_iter=N_ITER, device_mask=None):
    """Per case the keys of ``hmm_models.run_hmm_cases`` plus <tag>_Z_mask and <tag>_Y_mask.
    ``device_mask``: callable that turns a host mask into what ``observe`` is given."""
    out = {}
    wrap = device_mask if device_mask is not None else (lambda m: m)
    for tag in CASES + LEARNED:
        if only is not None and tag not in only:
            continue
        kw = dict(a0_prior=g['b_a0'], A_prior=g['b_A']) if tag == 'b' else {}
        m = build_hmm(mods, g[tag + '_y'], g[tag + '_mu'], g[tag + '_Lambda'], observe=False,
                      learned=tag in LEARNED, **kw)
        if tag != 'd':
            m['Y'].observe(g[tag + '_y'], mask=wrap(g[tag + '_mask']))
        if tag in ('b', 'e'):
            m['Z'].initialize_from_value(g[tag + '_z0'])
        more = (m['mu'], m['Lambda']) if tag in LEARNED else ()
        Q = mods['VB'](m['Y'], m['Z'], m['A'], m['a0'], *more, **mods.get('vb_kwargs', {}))
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        if tag == 'd':
            m['Y'].observe(g['d_y0'], mask=wrap(g['d_mask0']))
            m['Y'].observe(g['d_y'], mask=wrap(g['d_mask']))
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
        out[tag + '_Z_mask'] = np.array(np.broadcast_to(m['Z'].mask, m['Z'].plates), dtype=bool)
        out[tag + '_Y_mask'] = np.array(np.broadcast_to(m['Y'].mask, m['Y'].plates), dtype=bool)
        out[tag + '_plan'] = Q
    return out
