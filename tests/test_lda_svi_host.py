"""CPU: the mini-batch form of the fused latent-Dirichlet-allocation block (LDASVIPlan) on the
kernel double tests/lda_svi_host.py -- the stochastic-VI half of lda.rst against the live
reference's fixtures, the lazy recount after ``observe`` / ``set_value``, the matcher's declining
reasons under ``engine='fused'`` and the unchanged default engine."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tests'))

TRACE_TOL = dict(rtol=1e-8, atol=1e-8)       # tests/test_lda_host.py
MOM_TOL = dict(rtol=1e-7, atol=1e-9)


def _golden():
    g = np.load(os.path.join(GOLDEN, 'lda.npz'))
    return g, {k[3:]: g[k] for k in g.files if k.startswith('in_')}


class _DoubleVB:
    """``VB`` whose plan runs on the kernel double from the start."""

    def __new__(cls, *nodes, **kw):
        from bayespy_amd.inference import VB
        from bayespy_amd.device import Runtime
        from lda_svi_host import CPULDASVIKernels
        Q = VB(*nodes, **kw)
        plan = Q.plans[0]
        assert type(plan).__name__ == 'LDASVIPlan'
        rt = Runtime(device='cpu')
        plan._rt, plan._kernels = rt, CPULDASVIKernels(rt)
        return Q


def _mods(VB=None, **kw):
    import bayespy_amd.nodes as nodes
    from bayespy_amd.inference import VB as RealVB
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    return dict(nodes=nodes, VB=VB or RealVB, CategoricalMoments=CategoricalMoments, vb_kwargs=kw)


def _batch_model(m_topics=4.0, m_words=None, S=100, mask=None, concentration=False):
    """The mini-batch model of lda_models.run_lda_svi on the 'doc' inputs."""
    from bayespy_amd import nodes as N_
    from bayespy_amd.inference.vmp.nodes.categorical import CategoricalMoments
    _, gin = _golden()
    D, V, K = 7, 30, 4
    docs, corpus = gin['doc_docs'], gin['doc_words']
    a = N_.Concentration(K, name='c') if concentration else np.ones(K)
    p_topic = N_.Dirichlet(a, plates=(D,), name='p_topic')
    p_word = N_.Dirichlet(np.ones(V), plates=(K,), name='p_word')
    idx = N_.Constant(CategoricalMoments(D), docs[:S], name='document_indices')
    topics = N_.Categorical(N_.Gate(idx, p_topic), plates=(S,), plates_multiplier=(m_topics,),
                            name='topics')
    kw = {} if m_words is None else dict(plates_multiplier=(m_words,))
    words = N_.Categorical(N_.Gate(topics, p_word), name='words', **kw)
    if mask is None:
        words.observe(corpus[:S])
    else:
        words.observe(corpus[:S], mask=mask)
    nodes = [words, topics, p_word, p_topic, idx] + ([a] if concentration else [])
    return dict(words=words, topics=topics, p_word=p_word, p_topic=p_topic, idx=idx, nodes=nodes,
                docs=docs, corpus=corpus)


def test_svi_half_on_the_kernel_double_matches_reference():
    from lda_models import run_lda_svi
    g, gin = _golden()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        res = run_lda_svi(_mods(VB=_DoubleVB, engine='fused'), gin)
    assert not [str(w.message) for w in rec
                if 'engine' in str(w.message) or 'block' in str(w.message)]
    plans = res['svi_plan'].plans
    assert [type(p).__name__ for p in plans] == ['LDASVIPlan']
    np.testing.assert_allclose(res['svi_L'], g['svi_L'], **TRACE_TOL)
    for k in ('svi_p_word_u0', 'svi_p_topic_u0', 'svi_topics_u0'):
        np.testing.assert_allclose(res[k], g[k], err_msg=k, **MOM_TOL)


def test_one_token_pass_per_step_and_a_recount_when_the_bound_is_read():
    m = _batch_model()
    Q = _DoubleVB(*m['nodes'], engine='fused')
    Q.ignore_bound_checks = True
    Q.update(verbose=False)
    plan = Q.plans[0]
    calls = plan.kernels.calls
    rs = np.random.RandomState(5)

    def step(read_bound):
        sub = rs.choice(400, 100)
        del calls[:]
        m['words'].observe(m['corpus'][sub])
        m['idx'].set_value(m['docs'][sub])
        assert Q.plans[0] is plan and not calls          # nothing runs until it is needed
        if read_bound:
            assert np.isfinite(m['words'].lower_bound_contribution())
        m['topics'].update()
        return list(calls)
    assert step(False).count('token_pass') == 1
    assert step(False) == ['token_pass']
    got = step(True)
    assert got.count('token_pass') == 2 and got[0] == 'token_pass'      # the recount, then the update
    # the Dirichlet step reads the counts: no further pass after the update
    del calls[:]
    Q.gradient_step('p_topic', 'p_word', scale=0.5)
    assert calls == ['dirichlet_step', 'dirichlet_step']
    # ... but a recount when the batch changed and topics was not updated
    m['words'].observe(m['corpus'][:100])
    del calls[:]
    Q.gradient_step('p_word', scale=0.5)
    assert calls == ['token_pass', 'dirichlet_step']


def test_multiplier_is_read_at_every_operation():
    m = _batch_model(m_topics=4.0)
    Q = _DoubleVB(*m['nodes'], engine='fused')
    Q.update(verbose=False)
    plan = Q.plans[0]
    l4 = m['words'].lower_bound_contribution()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        m['topics'].plates_multiplier = (8.0,)
    assert Q.plans[0] is plan and plan.has_state()
    np.testing.assert_allclose(m['words'].lower_bound_contribution(), 2 * l4, rtol=1e-14)
    m['p_topic'].update()
    np.testing.assert_allclose(plan.alpha_theta.numpy(), 1.0 + 8.0 * plan.Ndk.numpy(), rtol=1e-15)


def test_engine_fused_raises_with_the_reason():
    from bayespy_amd.inference import VB
    m = _batch_model(mask=np.arange(100) % 2 == 0)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        with pytest.raises(NotImplementedError, match="engine='fused'.*fused LDA block.*mask"):
            VB(*m['nodes'], engine='fused')
    m = _batch_model(concentration=True)
    with pytest.raises(NotImplementedError, match='fused LDA block.*Concentration'):
        VB(*m['nodes'], engine='fused')
    # the environment variable selects the same engine
    m = _batch_model(m_topics=1.0, m_words=2.0)
    os.environ['BAYESPY_AMD_ENGINE'] = 'fused'
    try:
        with pytest.raises(NotImplementedError, match='unequal plates_multiplier'):
            VB(*m['nodes'])
    finally:
        del os.environ['BAYESPY_AMD_ENGINE']


def test_matcher_of_the_batch_form():
    from bayespy_amd.inference.plans.lda import LDASVIPlan, LDAPlan
    from bayespy_amd.inference.plans import PLAN_TYPES

    def match(m):
        why = []
        return LDASVIPlan.match(m['nodes'], why), why
    assert LDASVIPlan not in PLAN_TYPES and issubclass(LDASVIPlan, LDAPlan)
    for mt in (4.0, 1.0, 2.5):
        r, why = match(_batch_model(m_topics=mt))
        assert r is not None and why == []
    r, why = match(_batch_model(m_topics=1.0, m_words=2.0))
    assert r is None and len(why) == 1 and 'unequal plates_multiplier' in why[0]
    r, why = match(_batch_model(m_topics=-1.0))
    assert r is None and 'positive' in why[0]
    m = _batch_model()
    m['p_word'].plates_multiplier = (2.0,)
    r, why = match(m)
    assert r is None and 'Dirichlet carries' in why[0]
    m = _batch_model()
    m['topics'].shard(-1)
    r, why = match(m)
    assert r is None and 'sharded' in why[0]


def test_default_engine_still_gives_the_generic_plan():
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.generic import GenericPlan
    m = _batch_model()
    with pytest.warns(UserWarning, match='fused LDA block.*plates_multiplier'):
        plans = compile_model(m['nodes'])
    assert len(plans) == 1 and isinstance(plans[0], GenericPlan)
    # engine='fused' keeps its plan for a later VB over the same nodes; the default engine does not
    m = _batch_model()
    plans = compile_model(m['nodes'], engine='fused')
    assert [type(p).__name__ for p in plans] == ['LDASVIPlan']
    assert compile_model(m['nodes'], engine='fused')[0] is plans[0]
    with pytest.warns(UserWarning, match='fused LDA block.*plates_multiplier'):
        again = compile_model(m['nodes'])
    assert isinstance(again[0], GenericPlan)


def test_gradient_step_rules_on_the_double():
    m = _batch_model()
    m['p_topic'].initialize_from_value(_golden()[1]['doc_theta0'])
    Q = _DoubleVB(*m['nodes'], engine='fused')
    plan = Q.plans[0]
    with pytest.raises(NotImplementedError, match='engine="generic"'):
        Q.gradient_step('topics', scale=0.5)
    # observed nodes and constants are passed over, as on the generic engine
    Q.gradient_step('words', 'document_indices', scale=0.5)
    assert not plan.kernels.calls
    # a point mass steps from its prior: never a NaN table
    Q.gradient_step('p_topic', scale=0.25)
    a = plan.alpha_theta.numpy()
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(plan.elog_theta.numpy()))
    np.testing.assert_allclose(a, 1.0 + 0.25 * 4.0 * plan.Ndk.numpy(), rtol=1e-14)
    assert np.isfinite(m['p_topic'].lower_bound_contribution())
