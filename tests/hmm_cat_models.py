"""TEST INFRASTRUCTURE: the discrete hidden-Markov-model scripts (doc/source/examples/hmm.rst,
first half) that run, statement for statement, on the reference (tools/make_golden_hmm_cat.py ->
tests/golden/hmm_cat.npz) and on this framework (tests/test_hmm_cat_host.py,
tests/test_hmm_cat_gpu.py).

The reference checks the words of an observation whatever the mask says (categorical.py:
"Invalid category index" for any word outside [0, M), masked or not), so the inputs hold a valid
word (0) at every masked position.  ``fill`` writes another integer there before the data reach
this framework's nodes, which never use a masked word.

``mods``: dict(nodes=<module with Dirichlet, CategoricalMarkovChain, Mixture, Categorical>,
VB=<class>, vb_kwargs=<dict, optional>, after_vb=<callable(Q), optional>)."""
import numpy as np

N_ITER = 4

# hmm.rst, first model
RST_A0 = np.array([0.6, 0.4])
RST_A = np.array([[0.7, 0.3], [0.4, 0.6]])
RST_P = np.array([[0.1, 0.4, 0.5], [0.6, 0.3, 0.1]])

#       plates  T   K  M  learned roles      Z from labels
CASES = dict(
    i=((), 100, 2, 3, (), False),                       # hmm.rst verbatim: one update is exact
    ii=((), 40, 3, 5, ('a0', 'A', 'P'), False),         # one chain, everything from the prior
    iii=((5,), 12, 3, 4, ('a0', 'A', 'P'), True),       # a batch, Z from fixed labels
    iv=((3,), 2, 1, 1, ('a0', 'A', 'P'), False),        # T = 2, K = 1, M = 1
    v=((6,), 15, 3, 4, ('a0', 'A', 'P'), True),         # a full-shape mask: ragged tails and holes
    vi=((4,), 9, 2, 6, ('A', 'P'), False),              # observed after VB(...); a0 a constant
)


def trailing(lengths, T):
    return np.arange(T)[None, :] < np.asarray(lengths)[:, None]


def _sample(rs, plates, T, a0, A, P):
    K, M = P.shape
    z = np.empty(plates + (T,), dtype=np.int64)
    y = np.empty(plates + (T,), dtype=np.int64)
    for idx in np.ndindex(*plates):
        s = rs.choice(K, p=a0)
        for t in range(T):
            z[idx + (t,)] = s
            y[idx + (t,)] = rs.choice(M, p=P[s])
            s = rs.choice(K, p=A[s])
    return y


def make_inputs(rs):
    g = {}
    for tag, (plates, T, K, M, learned, labels) in CASES.items():
        if tag == 'i':
            a0, A, P = RST_A0, RST_A, RST_P
        else:
            a0 = rs.dirichlet(np.ones(K))
            A = rs.dirichlet(np.ones(K), size=K) * 0.4 + 0.6 * np.identity(K)
            P = rs.dirichlet(0.5 * np.ones(M), size=K) * 0.9 + 0.1 / M
        g[tag + '_y'] = _sample(rs, plates, T, a0, A, P)
        g[tag + '_a0'], g[tag + '_A'], g[tag + '_P'] = a0, A, P
        # asymmetric priors, so that the states are told apart from the first sweep on
        g[tag + '_a0_prior'] = 0.5 + rs.gamma(1.0, size=K)
        g[tag + '_A_prior'] = 0.5 + rs.gamma(1.0, size=(K, K))
        g[tag + '_P_prior'] = 0.5 + rs.gamma(1.0, size=(K, M))
        g[tag + '_z0'] = rs.randint(K, size=plates + (T,))
    m = trailing((15, 11, 8, 15, 4, 0), 15) & (rs.rand(6, 15) < 0.8)
    m[0, 0], m[3] = False, True
    g['v_mask'] = m
    g['v_y'] = np.where(m, g['v_y'], 0)
    g['vi_y0'] = g['vi_y'][::-1].copy()
    return g


def build(mods, g, tag, observe=True, fill=None, wrap=lambda m: m):
    N_ = mods['nodes']
    plates, T, K, M, learned, _ = CASES[tag]

    def role(nm, **kw):
        if nm in learned:
            return N_.Dirichlet(g['%s_%s_prior' % (tag, nm)], name=nm, **kw)
        return g['%s_%s' % (tag, nm)]
    a0, A, P = role('a0'), role('A'), role('P')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=plates, name='Z')
    Y = N_.Mixture(Z, N_.Categorical, P, name='Y')
    m = dict(a0=a0, A=A, P=P, Z=Z, Y=Y)

    def obs(key='y'):
        y = g['%s_%s' % (tag, key)]
        if tag + '_mask' in g:
            mask = g[tag + '_mask']
            Y.observe(y if fill is None else np.where(mask, y, fill), mask=wrap(mask))
        else:
            Y.observe(y)
    m['observe'] = obs
    if observe:
        obs()
    return m


def run_cases(mods, g, only=None, n_iter=N_ITER, fill=None, device_mask=None):
    """Per case: <tag>_L, <tag>_<node>_Lterm for Y, Z and the learned roles, <tag>_Z_u0 / _Z_u1,
    <tag>_<role>_u0 of the learned roles, with a mask <tag>_Z_mask and <tag>_Y_mask; the engine
    itself as <tag>_plan and the nodes as <tag>_model."""
    out = {}
    wrap = device_mask if device_mask is not None else (lambda m: m)
    for tag, (plates, T, K, M, learned, labels) in CASES.items():
        if only is not None and tag not in only:
            continue
        m = build(mods, g, tag, observe=tag != 'vi', fill=fill, wrap=wrap)
        if labels:
            m['Z'].initialize_from_value(g[tag + '_z0'])
        params = [m[nm] for nm in ('P', 'A', 'a0') if nm in learned]
        Q = mods['VB'](m['Y'], m['Z'], *params, **mods.get('vb_kwargs', {}))
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        if tag == 'vi':
            m['observe']('y0')
            m['observe']()
        Q.ignore_bound_checks = True
        n = 1 if tag == 'i' else n_iter
        if labels:
            Q.update(*params, m['Z'], repeat=n, verbose=False)
        else:
            Q.update(repeat=n, verbose=False)
        out[tag + '_L'] = np.array(Q.L[:n])
        for nm in ('Y', 'Z') + tuple(learned):
            out['%s_%s_Lterm' % (tag, nm)] = np.array(Q.l[m[nm]][:n])
        u = m['Z'].get_moments()
        out[tag + '_Z_u0'], out[tag + '_Z_u1'] = np.array(u[0]), np.array(u[1])
        for nm in learned:
            out['%s_%s_u0' % (tag, nm)] = np.array(m[nm].get_moments()[0])
        if tag + '_mask' in g:
            out[tag + '_Z_mask'] = np.array(np.broadcast_to(m['Z'].mask, m['Z'].plates), dtype=bool)
            out[tag + '_Y_mask'] = np.array(np.broadcast_to(m['Y'].mask, m['Y'].plates), dtype=bool)
        out[tag + '_plan'] = Q
        out[tag + '_model'] = m
    return out


def n_fixture_arrays():
    """Arrays ``run_cases`` returns for the fixture (plans and models apart)."""
    return sum(1 + 2 + len(c[4]) + 2 + len(c[4]) for c in CASES.values()) + 2
