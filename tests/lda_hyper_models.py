"""Latent-Dirichlet-allocation models with learnt concentrations (``DirichletConcentration`` parents
of p_topic and / or p_word), shared statement for statement by the fixture generator
tools/make_golden_lda_hyper.py, which runs them on the reference, and the tests, which run them on
this package.  ``mods`` is that of tests/lda_models.py plus ``params``: a function (Q, model) ->
(alpha of p_topic (D, K), alpha of p_word (K, V)), the Dirichlet parameters as each side keeps them."""
import numpy as np

D, N, V, SWEEPS = 12, 400, 30, 4
# regularization given as a pair: "prior" log-probability (a total over the count) and count
PAIR_TOPIC = (-6.0, 3.0)
PAIR_WORD = (-8.0, 2.0)
# tag -> (topics, regularization of the concentration of p_topic (None: constant parent), the same
# of p_word, the concentrations are updated first)
HYPER_CASES = {
    'topic': (5, True, None, False),
    'word': (5, None, False, False),
    'both': (5, True, False, False),
    'pair': (5, PAIR_TOPIC, PAIR_WORD, False),
    'first': (5, False, True, True),
    'k70': (70, True, True, False),
}
INPUT_K = (5, 70)


def make_hyper_inputs(rs):
    g = {'docs': rs.randint(D, size=N).astype(np.int64),
         'words': rs.randint(V, size=N).astype(np.int64)}
    for K in INPUT_K:
        g['k%d_theta0' % K] = rs.dirichlet(np.ones(K), size=D)
        g['k%d_beta0' % K] = rs.dirichlet(np.ones(V), size=K)
    return g


def build_hyper(mods, g, K, reg_topic, reg_word):
    """The model of lda.rst with a concentration node wherever a regularization is given."""
    N_ = mods['nodes']
    m = {}
    a, b = np.ones(K), np.ones(V)
    if reg_topic is not None:
        a = m['conc_topic'] = N_.DirichletConcentration(K, regularization=reg_topic,
                                                        name='conc_topic')
    if reg_word is not None:
        b = m['conc_word'] = N_.DirichletConcentration(V, regularization=reg_word, name='conc_word')
    m['p_topic'] = N_.Dirichlet(a, plates=(D,), name='p_topic')
    m['p_word'] = N_.Dirichlet(b, plates=(K,), name='p_word')
    m['topics'] = N_.Categorical(N_.Gate(g['docs'], m['p_topic']), plates=(N,), name='topics')
    m['words'] = N_.Categorical(N_.Gate(m['topics'], m['p_word']), name='words')
    m['words'].observe(g['words'])
    return m


def model_nodes(m, conc_first=False):
    """The nodes in update order: (words, topics, p_word, p_topic, concentrations) or the
    concentrations first."""
    four = [m['words'], m['topics'], m['p_word'], m['p_topic']]
    conc = [m[k] for k in ('conc_word', 'conc_topic') if k in m]
    return conc + four if conc_first else four + conc


def run_hyper_case(mods, g, tag, sweeps=SWEEPS, after_sweep=None):
    """{key: array}: the initial moments of every concentration, and after every sweep the bound,
    every per-node term, both Dirichlet parameter tables and both moments of every concentration."""
    K, reg_topic, reg_word, conc_first = HYPER_CASES[tag]
    m = build_hyper(mods, g, K, reg_topic, reg_word)
    m['p_topic'].initialize_from_value(g['k%d_theta0' % K])
    m['p_word'].initialize_from_value(g['k%d_beta0' % K])
    nodes = model_nodes(m, conc_first)
    Q = mods['VB'](*nodes, **mods.get('vb_kwargs', {}))
    if 'after_vb' in mods:
        mods['after_vb'](Q)
    Q.ignore_bound_checks = True
    conc = [k for k in ('conc_topic', 'conc_word') if k in m]
    out = {tag + '_plan': Q, tag + '_model': m}
    for k in conc:
        u = m[k].get_moments()
        out['%s_%s_init_u0' % (tag, k)] = np.array(u[0], dtype=np.float64)
        out['%s_%s_init_u1' % (tag, k)] = np.array(u[1], dtype=np.float64)
    at, ab = [], []
    cu = {k: ([], []) for k in conc}
    for it in range(sweeps):
        Q.update(repeat=1, verbose=False)
        a, b = mods['params'](Q, m)
        at.append(np.array(a, dtype=np.float64))
        ab.append(np.array(b, dtype=np.float64))
        for k in conc:
            u = m[k].get_moments()
            cu[k][0].append(np.array(u[0], dtype=np.float64))
            cu[k][1].append(np.array(u[1], dtype=np.float64))
        if after_sweep is not None:
            after_sweep(Q, it)
    out[tag + '_L'] = np.array(Q.L[:sweeps])
    out[tag + '_alpha_topic'], out[tag + '_alpha_word'] = np.array(at), np.array(ab)
    for k in conc:
        out['%s_%s_u0' % (tag, k)] = np.array(cu[k][0])
        out['%s_%s_u1' % (tag, k)] = np.array(cu[k][1])
    for nm in ['words', 'topics', 'p_word', 'p_topic'] + conc:
        out['%s_l_%s' % (tag, nm)] = np.array(Q.l[m[nm]][:sweeps])
    return out


def plan_params(Q, m):
    """The parameters as the fused plan keeps them (p_word transposed)."""
    plan = Q.plans[0]
    return plan.alpha_theta.cpu().numpy(), plan.alpha_beta_t.cpu().numpy().T


def generic_params(Q, m):
    """The parameters as the nodes give them on the generic engine."""
    return m['p_topic'].phi[0], m['p_word'].phi[0]
