"""Latent-Dirichlet-allocation models (doc/source/examples/lda.rst), shared statement for statement
by the fixture generator tools/make_golden_lda.py, which runs them on the reference, and the tests,
which run them on this package.  ``mods`` carries what differs between the two sides: the ``nodes``
module, ``VB``, ``CategoricalMoments``, the keyword arguments of ``VB`` (the engine), a hook called
with the new ``VB``, and ``raw_indices`` (case f with the raw index array after all)."""
import numpy as np

# tag -> (documents, tokens, vocabulary, topics, sweeps)
CASES = {
    'doc': (7, 400, 30, 4, 5),          # a. the doc model, small
    'k1': (5, 120, 12, 1, 3),           # b. one topic
    'k64': (3, 40, 9, 64, 3),           # b. 64 topics, few tokens
    'gaps': (9, 150, 25, 3, 4),         # c. documents without tokens, unused vocabulary entries
    'conc': (6, 300, 20, 5, 4),         # d. non-uniform concentration arrays
    'order': (7, 400, 30, 4, 0),        # e. partial update orders (sweeps are spelled out)
    'const': (7, 400, 30, 4, 3),        # f. Constant(CategoricalMoments(n), idx)
    'zinit': (6, 200, 15, 3, 3),        # topics initialised by value
}


def make_lda_inputs(rs):
    g = {}
    for tag, (D, n, V, K, _) in CASES.items():
        if tag == 'gaps':
            docs = rs.choice([0, 2, 3, 7], size=n)              # documents 1, 4, 5, 6, 8 are empty
            words = rs.choice(np.arange(0, V, 3), size=n)       # two thirds of the vocabulary unused
        else:
            docs = rs.randint(D, size=n)
            words = rs.randint(V, size=n)
        g[tag + '_docs'], g[tag + '_words'] = docs.astype(np.int64), words.astype(np.int64)
        g[tag + '_theta0'] = rs.dirichlet(np.ones(K), size=D)
        g[tag + '_beta0'] = rs.dirichlet(np.ones(V), size=K)
    g['conc_a'] = rs.gamma(2.0, 0.5, size=(6, 5)) + 0.05        # documents x topics
    g['conc_b'] = rs.gamma(1.0, 0.3, size=(5, 20)) + 0.05       # topics x vocabulary
    g['zinit_z0'] = rs.randint(3, size=200).astype(np.int64)
    return g


def build_lda(mods, docs, words, D, V, K, a=None, b=None, index_constant=False, name_suffix=''):
    N_ = mods['nodes']
    n = len(words)
    p_topic = N_.Dirichlet(np.ones(K) if a is None else a, plates=(D,), name='p_topic')
    p_word = N_.Dirichlet(np.ones(V) if b is None else b, plates=(K,), name='p_word')
    if index_constant:
        idx = N_.Constant(mods['CategoricalMoments'](D), docs, name='document_indices')
    else:
        idx = docs
    topics = N_.Categorical(N_.Gate(idx, p_topic), plates=(n,), name='topics')
    wnode = N_.Categorical(N_.Gate(topics, p_word), name='words')
    wnode.observe(words)
    return dict(p_topic=p_topic, p_word=p_word, topics=topics, words=wnode, idx=idx)


def run_lda_cases(mods, g, only=None, moments_of=('words', 'topics', 'p_word', 'p_topic')):
    """{key: array}: Q.L after every sweep, every Q.l[node], the final moments of the four nodes."""
    VB, kw = mods['VB'], mods.get('vb_kwargs', {})
    out = {}
    for tag, (D, n, V, K, sweeps) in CASES.items():
        if only is not None and tag not in only:
            continue
        a = g['conc_a'] if tag == 'conc' else None
        b = g['conc_b'] if tag == 'conc' else None
        m = build_lda(mods, g[tag + '_docs'], g[tag + '_words'], D, V, K, a=a, b=b,
                      index_constant=(tag == 'const' and not mods.get('raw_indices')))
        m['p_topic'].initialize_from_value(g[tag + '_theta0'])
        m['p_word'].initialize_from_value(g[tag + '_beta0'])
        if tag == 'zinit':
            m['topics'].initialize_from_value(g['zinit_z0'])
        nodes = [m['words'], m['topics'], m['p_word'], m['p_topic']]
        if tag == 'const' and not mods.get('raw_indices'):
            nodes.append(m['idx'])
        Q = VB(*nodes, **kw)
        if 'after_vb' in mods:
            mods['after_vb'](Q)
        Q.ignore_bound_checks = True
        if tag == 'order':
            Q.update('topics', verbose=False)
            Q.update('p_topic', 'p_word', verbose=False)
            Q.update('p_word', verbose=False)
            Q.update('topics', 'p_topic', verbose=False)
            Q.update(repeat=2, verbose=False)
            sweeps = 6
        else:
            Q.update(repeat=sweeps, verbose=False)
        out[tag + '_plan'] = Q
        order = ('words', 'topics', 'p_word', 'p_topic')
        out[tag + '_L'] = np.array(Q.L[:sweeps])
        for nm in order:
            out['%s_l_%s' % (tag, nm)] = np.array(Q.l[m[nm]][:sweeps])
            if nm in moments_of:
                out['%s_%s_u0' % (tag, nm)] = np.array(m[nm].get_moments()[0])
    return out


def run_lda_svi(mods, g, steps=4):
    """The stochastic-VI half of lda.rst on the 'doc' inputs: mini-batches of 100 tokens with
    ``plates_multiplier``, ``set_value`` on the index constant, ``gradient_step`` on the Dirichlets
    (mini-batches and step lengths fixed by a seed; one VB sweep first, so that the Dirichlets have
    parameters).  {key: array}."""
    N_, VB, kw = mods['nodes'], mods['VB'], mods.get('vb_kwargs', {})
    D, n, V, K, _ = CASES['doc']
    S = 100
    docs, corpus = g['doc_docs'], g['doc_words']
    rs = np.random.RandomState(31)
    p_topic = N_.Dirichlet(np.ones(K), plates=(D,), name='p_topic')
    p_word = N_.Dirichlet(np.ones(V), plates=(K,), name='p_word')
    idx = N_.Constant(mods['CategoricalMoments'](D), docs[:S], name='document_indices')
    topics = N_.Categorical(N_.Gate(idx, p_topic), plates=(S,), plates_multiplier=(n / S,),
                            name='topics')
    words = N_.Categorical(N_.Gate(topics, p_word), name='words')
    words.observe(corpus[:S])
    p_topic.initialize_from_value(g['doc_theta0'])
    p_word.initialize_from_value(g['doc_beta0'])
    Q = VB(words, topics, p_word, p_topic, idx, **kw)
    Q.ignore_bound_checks = True
    Q.update(verbose=False)
    for it in range(steps):
        subset = rs.choice(n, S)
        Q['words'].observe(corpus[subset])
        Q['document_indices'].set_value(docs[subset])
        Q.update('topics', verbose=False)
        Q.gradient_step('p_topic', 'p_word', scale=(it + 1) ** (-0.7))
    return {'svi_L': np.array(Q.L[:steps + 1]), 'svi_plan': Q,
            'svi_p_word_u0': np.array(p_word.get_moments()[0]),
            'svi_p_topic_u0': np.array(p_topic.get_moments()[0]),
            'svi_topics_u0': np.array(topics.get_moments()[0])}
