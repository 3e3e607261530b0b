"""CPU: the matcher of plans/hmm_mult.py: its declines, and that only engine='fused+counts' tries it."""
import numpy as np
import pytest

B, T, K, M = 3, 5, 2, 4


def _build(M=M, n=6, Zkw={}):
    from bayespy_amd import nodes as N_
    a0, A = N_.Dirichlet(np.ones(K), name='a0'), N_.Dirichlet(np.ones((K, K)), name='A')
    P = N_.Dirichlet(np.ones((K, M)), name='P')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z', **Zkw)
    Y = N_.Mixture(Z, N_.Multinomial, n, P, name='Y')
    return [Y, Z, P, A, a0]


def _masked_over_T():
    nodes = _build()
    x = np.zeros((B, T, M), dtype=int)
    x[..., 0] = 6
    nodes[0].observe(x, mask=np.ones((B, 1), dtype=bool))
    return nodes


@pytest.mark.parametrize('make,text', [
    (lambda: _build(M=1025), 'M = 1025, K = 2 exceed the limits of the block (M <= 1024, K <= 64)'),
    (lambda: _build(n=np.full(K, 6)), 'the number of trials n has shape (2,)'),
    (lambda: _build(Zkw=dict(plates_multiplier=(2.5,))), 'plates_multiplier'),
    (_masked_over_T, 'mask of shape (3, 1)'),
])
def test_matcher_declines_with_a_reason(make, text):
    from bayespy_amd.inference.plans.hmm_mult import MultinomialHMMPlan
    why = []
    assert MultinomialHMMPlan.match(make(), why) is None and len(why) == 1
    assert why[0].startswith('fused hidden-Markov-model block (multinomial emissions), observed '
                             'node Y: ') and text in why[0]


@pytest.mark.parametrize('engine,blocks', [
    ('fused', 'fused hidden-Markov-model block, '),
    ('fused+words', 'fused hidden-Markov-model block, '),
    ('fused+chains', 'fused hidden-Markov-model block (long chains), '),
])
def test_other_engines_keep_their_answer(engine, blocks):
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.hmm_mult import MultinomialHMMPlan
    with pytest.raises(NotImplementedError) as exc:
        compile_model(_build(), engine=engine)
    assert str(exc.value) == ("engine='fused': no fused block covers Y, Z, P, A, a0 -- " + blocks
                              + "observed node Y: the mixed distribution is Multinomial, not Gaussian")
    nodes = _build()
    plans = compile_model(nodes, engine='fused+counts')
    assert [type(p) for p in plans] == [MultinomialHMMPlan]
    assert compile_model(nodes, engine='fused+counts')[0] is plans[0]
    with pytest.raises(NotImplementedError):    # such a plan is kept only where it is asked for
        compile_model(nodes, engine=engine)
