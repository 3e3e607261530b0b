"""CPU: the matcher of plans/hmm_states.py and that only engine='fused+states' tries it."""
import numpy as np
import pytest

B, T, M = 3, 5, 4


def _build(K):
    from bayespy_amd import nodes as N_
    a0, A = N_.Dirichlet(np.ones(K), name='a0'), N_.Dirichlet(np.ones((K, K)), name='A')
    P = N_.Dirichlet(np.ones((K, M)), name='P')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z')
    Y = N_.Mixture(Z, N_.Multinomial, 6, P, name='Y')
    return [Y, Z, P, A, a0]


def test_states_engine_builds_the_block_that_fits():
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.hmm_mult import MultinomialHMMPlan
    from bayespy_amd.inference.plans.hmm_states import WideStateMultinomialHMMPlan
    assert [type(p) for p in compile_model(_build(5), engine='fused+states')] == [MultinomialHMMPlan]
    nodes = _build(70)
    plans = compile_model(nodes, engine='fused+states')
    assert [type(p) for p in plans] == [WideStateMultinomialHMMPlan]
    assert compile_model(nodes, engine='fused+states')[0] is plans[0]
    for engine in ('fused+counts', 'fused'):    # such a plan is kept only where it is asked for
        with pytest.raises(NotImplementedError):
            compile_model(nodes, engine=engine)
    with pytest.raises(NotImplementedError, match=r'65 to 128 states\), observed node Y: M = 4, '
                                                  r'K = 129 exceed the limits of the block '
                                                  r'\(M <= 1024, K <= 128\)'):
        compile_model(_build(129), engine='fused+states')


@pytest.mark.parametrize('engine,reason', [
    ('fused+counts', 'M = 4, K = 70 exceed the limits of the block (M <= 1024, K <= 64)'),
    ('fused', 'the mixed distribution is Multinomial, not Gaussian'),
])
def test_other_engines_keep_their_answer(engine, reason):
    from bayespy_amd.inference.plans import compile_model
    with pytest.raises(NotImplementedError) as exc:
        compile_model(_build(70), engine=engine)
    assert reason in str(exc.value) and '65 to 128' not in str(exc.value)
