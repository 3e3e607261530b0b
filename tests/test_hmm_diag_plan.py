"""CPU: the matcher of plans/hmm_diag.py: its declines, and that only engine='fused+diagonal' tries it."""
import numpy as np
import pytest

B, T, K, D = 3, 5, 2, 4


def _build(D=D, const=False, tau_plates=None, Zkw={}, mask=None):
    from bayespy_amd import nodes as N_
    a0, A = N_.Dirichlet(np.ones(K), name='a0'), N_.Dirichlet(np.ones((K, K)), name='A')
    Z = N_.CategoricalMarkovChain(a0, A, states=T, plates=(B,), name='Z', **Zkw)
    if const:
        mu, tau = np.zeros((K, D)), np.ones((K, D))
    else:
        mu = N_.GaussianARD(0, 1e-3, shape=(D,), plates=(K,), name='mu')
        tau = N_.Gamma(1e-3, 1e-3, plates=tau_plates or (K, D), name='tau')
    Y = N_.Mixture(Z, N_.GaussianARD, mu, tau, 1, name='Y')
    if mask is not None:
        Y.observe(np.zeros((B, T, D)), mask=np.ones(mask, dtype=bool))
    return [Y, Z] + ([] if const else [mu, tau]) + [A, a0]


@pytest.mark.parametrize('kw,text', [
    (dict(D=1025), 'D = 1025, K = 2 exceed the limits of the block (D <= 1024, K <= 64)'),
    (dict(const=True), 'mu is Constant and tau is Constant: the block takes (GaussianARD, Gamma)'),
    (dict(mask=(B, 1)), 'mask of shape (3, 1)'),
    (dict(tau_plates=(K, 1)), 'plates of mu / tau are (2,) / (2, 1)'),
    (dict(Zkw=dict(plates_multiplier=(2.5,))), 'plates_multiplier'),
])
def test_matcher_declines_with_a_reason(kw, text):
    from bayespy_amd.inference.plans.hmm_diag import DiagGaussianHMMPlan
    why = []
    assert DiagGaussianHMMPlan.match(_build(**kw), why) is None and len(why) == 1
    assert why[0].startswith('fused hidden-Markov-model block (diagonal-Gaussian emissions), '
                             'observed node Y: ') and text in why[0]


def test_a_mask_per_element_never_reaches_the_matcher():
    """Y has plates (B, T) and shape (D,): the node itself refuses a mask of shape (B, T, D)."""
    with pytest.raises(ValueError, match='does not broadcast to plates'):
        _build(mask=(B, T, D))


@pytest.mark.parametrize('engine,blocks', [
    ('fused', 'fused hidden-Markov-model block, '),
    ('fused+counts', 'fused hidden-Markov-model block, '),
    ('fused+emissions', 'fused hidden-Markov-model block, '),
    ('fused+chains', 'fused hidden-Markov-model block (long chains), '),
])
def test_other_engines_keep_their_answer(engine, blocks):
    from bayespy_amd.inference.plans import compile_model
    from bayespy_amd.inference.plans.hmm_diag import DiagGaussianHMMPlan
    with pytest.raises(NotImplementedError) as exc:
        compile_model(_build(), engine=engine)
    assert ("engine='fused': no fused block covers Y, Z, mu, tau, A, a0 -- " + blocks
            + "observed node Y: the mixed distribution is GaussianARD, not Gaussian") in str(exc.value)
    nodes = _build(mask=(B, T))
    plans = compile_model(nodes, engine='fused+diagonal')
    assert [type(p) for p in plans] == [DiagGaussianHMMPlan]
    assert compile_model(nodes, engine='fused+diagonal')[0] is plans[0]
    with pytest.raises(NotImplementedError):    # such a plan is kept only where it is asked for
        compile_model(nodes, engine=engine)
