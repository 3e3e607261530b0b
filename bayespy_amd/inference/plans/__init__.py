"""
Compiled execution plans: each plan owns the HBM-resident state of one model
block and maps the reference's per-node operations (``update``,
``lower_bound_contribution``, ``get_moments``) onto HIP kernel launches.
"""
from .pca import PCAPlan
from .masked_pca import MaskedPCAPlan
from .gmm import GMMPlan, GMMSVIPlan
from .lssm import LSSMPlan
from .lssm_masked import MaskedLSSMPlan
from .lda import LDAPlan, LDASVIPlan
from .lda_wide import WideLDAPlan
from .lda_hyper import HyperLDAPlan, WideHyperLDAPlan
from .bmm import BernoulliMixturePlan, BernoulliMixtureSVIPlan
from .hmm import HMMPlan
from .hmm_cat import CategoricalHMMPlan
from .dgmm import DiagGaussianMixturePlan
from .dgmm_masked import MaskedDiagGaussianMixturePlan
from .dgmm_svi import DiagGaussianMixtureSVIPlan, MaskedDiagGaussianMixtureSVIPlan
from .cmm import CategoricalMixturePlan, CategoricalMixtureSVIPlan
from .pmm import PoissonMixturePlan, PoissonMixtureSVIPlan
from .mmm import MultinomialMixturePlan, MultinomialMixtureSVIPlan
from .binm import BinomialMixturePlan, BinomialMixtureSVIPlan

PLAN_TYPES = [PCAPlan, MaskedPCAPlan, GMMPlan, LSSMPlan, MaskedLSSMPlan, LDAPlan]
# engine='fused': a block's opt-in form takes the place of its default form
OPT_IN_FORMS = {LDAPlan: LDASVIPlan}
# engine='fused': blocks that have no default form (their models run on the generic engine otherwise)
OPT_IN_TYPES = [BernoulliMixturePlan, HMMPlan]
# engine='fused': further emission families of an opt-in block, each a plan class of its own, tried
# right after that block (the block itself declines them with a reason, so they join neither list
# above: CategoricalHMMPlan is HMMPlan with a table lookup in place of the Gaussian quadratic form)
OPT_IN_EMISSIONS = {HMMPlan: [CategoricalHMMPlan]}
# engine='fused': further forms of a default block, tried right after it -- the block keeps
# whatever it matches (GMMSVIPlan takes the mixture under mini-batches, which GMMPlan declines)
OPT_IN_AFTER = {GMMPlan: [GMMSVIPlan]}
# engine='fused': further opt-in blocks, tried after ``opt_in_types()``
OPT_IN_MORE = [DiagGaussianMixturePlan]
# engine='fused': the form of an opt-in block for missing observations, a plan class of its own,
# tried right after that block (which declines every mask with a reason)
OPT_IN_MASKED = {DiagGaussianMixturePlan: [MaskedDiagGaussianMixturePlan]}
# engine='fused': opt-in blocks tried after everything above (CategoricalMixturePlan takes the
# mixtures of Categorical, with or without a mask, that every block above passes over in silence)
OPT_IN_LAST = [CategoricalMixturePlan]
# engine='fused': opt-in blocks for count data, tried after ``OPT_IN_LAST`` (PoissonMixturePlan takes
# the mixtures of Poisson, with or without a mask, that every block above passes over in silence)
OPT_IN_COUNTS = [PoissonMixturePlan]
# engine='fused': opt-in blocks for count vectors, tried after ``OPT_IN_COUNTS`` (MultinomialMixturePlan
# takes the mixtures of Multinomial, which CategoricalMixturePlan declines with a reason)
OPT_IN_VECTORS = [MultinomialMixturePlan]
# engine='fused': opt-in blocks for successes out of trials, tried after ``OPT_IN_VECTORS``
# (BinomialMixturePlan takes the mixtures of Binomial, which BernoulliMixturePlan declines with a reason)
OPT_IN_TRIALS = [BinomialMixturePlan]
# engine='fused+batches': the form of a count-mixture block under mini-batches (stochastic VI,
# plans/_mixture_svi.py), a plan class of its own, tried right after that block (which declines every
# plates_multiplier with a reason).  Everything else is engine='fused'; plain 'fused' does not try
# these forms and keeps raising for such a model with the blocks' reasons
OPT_IN_BATCHES = {BernoulliMixturePlan: [BernoulliMixtureSVIPlan],
                  CategoricalMixturePlan: [CategoricalMixtureSVIPlan],
                  PoissonMixturePlan: [PoissonMixtureSVIPlan],
                  MultinomialMixturePlan: [MultinomialMixtureSVIPlan],
                  BinomialMixturePlan: [BinomialMixtureSVIPlan]}
# engine='fused+batches+gaussian': the forms of the two diagonal-Gaussian blocks under mini-batches
# (plans/dgmm_svi.py), each tried right after its block.  Everything else is engine='fused+batches';
# 'fused' and 'fused+batches' do not try these forms and keep raising for such a model
OPT_IN_GAUSSIAN_BATCHES = {DiagGaussianMixturePlan: [DiagGaussianMixtureSVIPlan],
                           MaskedDiagGaussianMixturePlan: [MaskedDiagGaussianMixtureSVIPlan]}
# engine='fused+topics': the form of the LDA block for 65 to 1024 topics (plans/lda_wide.py), a plan
# class of its own, tried right after that block (which declines K > 64 with a reason).  Everything
# else is engine='fused'; every other engine value does not try this form and keeps its answer
OPT_IN_TOPICS = {LDAPlan: [WideLDAPlan]}
# engine='fused+hyper' / 'fused+topics+hyper': the forms of the LDA block and of its wide-topic form
# with learnt concentrations (plans/lda_hyper.py), each a plan class of its own, tried right after
# its form (which declines a Concentration parent with a reason).  'fused+hyper' is engine='fused'
# plus HyperLDAPlan, 'fused+topics+hyper' is engine='fused+topics' plus both; every other engine
# value does not try these forms and keeps its answer
OPT_IN_HYPER = {LDAPlan: [HyperLDAPlan], WideLDAPlan: [WideHyperLDAPlan]}


def _with_masked(types):
    """``types`` with the plan classes of ``OPT_IN_MASKED`` inserted after their block."""
    return [Q for P in types for Q in [P] + OPT_IN_MASKED.get(P, [])]


def _with_batches(types):
    """``types`` with the plan classes of ``OPT_IN_BATCHES`` inserted after their block."""
    return [Q for P in types for Q in [P] + OPT_IN_BATCHES.get(P, [])]


def _with_gaussian_batches(types):
    """``types`` with the plan classes of ``OPT_IN_GAUSSIAN_BATCHES`` inserted after their block."""
    return [Q for P in types for Q in [P] + OPT_IN_GAUSSIAN_BATCHES.get(P, [])]


def _with_topics(types):
    """``types`` with the plan classes of ``OPT_IN_TOPICS`` inserted after their block (or after
    the opt-in form that stands in its place)."""
    after = {OPT_IN_FORMS.get(P, P): v for P, v in OPT_IN_TOPICS.items()}
    return [Q for P in types for Q in [P] + after.get(P, [])]


def _with_hyper(types):
    """``types`` with the plan classes of ``OPT_IN_HYPER`` inserted after their form (or after the
    opt-in form that stands in its place), where that form is among ``types``."""
    after = {OPT_IN_FORMS.get(P, P): v for P, v in OPT_IN_HYPER.items()}
    return [Q for P in types for Q in [P] + after.get(P, [])]


def opt_in_types():
    """``OPT_IN_TYPES`` with the plan classes of ``OPT_IN_EMISSIONS`` inserted after their block."""
    return [Q for P in OPT_IN_TYPES for Q in [P] + OPT_IN_EMISSIONS.get(P, [])]


def _reusable_plans(nodes, engine, options=None):
    """In the reference the state of q lives in the nodes, so a second ``VB`` over nodes that
    were already updated continues from their posteriors.  Here it lives in the plans: when the
    plans that own these nodes cover exactly what is asked for, they are kept."""
    from ...nodes.node import Stochastic
    from .generic import GenericPlan
    plans = []
    for n in nodes:
        if not isinstance(n, Stochastic):
            continue
        p = n._plan
        if p is None:
            return None
        if not any(p is q for q in plans):
            plans.append(p)
    if not plans:
        return None
    if engine == 'generic' and not all(isinstance(p, GenericPlan) for p in plans):
        return None
    if engine == 'fused' and any(isinstance(p, GenericPlan) for p in plans):
        return None
    if engine != 'fused' and any(type(p) in OPT_IN_FORMS.values() or type(p) in opt_in_types()
                                 or type(p) in OPT_IN_MORE
                                 or any(type(p) in v for v in OPT_IN_AFTER.values())
                                 or any(type(p) in v for v in OPT_IN_MASKED.values())
                                 or type(p) in OPT_IN_LAST or type(p) in OPT_IN_COUNTS
                                 or type(p) in OPT_IN_VECTORS or type(p) in OPT_IN_TRIALS
                                 or any(type(p) in v for v in OPT_IN_TOPICS.values())
                                 or any(type(p) in v for v in OPT_IN_HYPER.values())
                                 for p in plans):
        return None             # an opt-in form is kept only where it is asked for
    covered = set(id(m) for p in plans for m in p.nodes())
    if not all(id(n) in covered for n in nodes):
        return None
    if engine != 'generic' and all(isinstance(p, GenericPlan) for p in plans) \
            and getattr(plans[0], '_engine_request', None) == 'generic':
        # built on request for engine='generic'; without that request the fused blocks get their
        # chance again (the generic engine was kept silently)
        import warnings
        warnings.warn("the existing plan was built with engine='generic'; this VB matches the "
                      "fused blocks again (posterior state starts again from the nodes' "
                      "initialisation)")
        return None
    for p in plans:
        for key, val in (options or {}).items():
            have = {'stats': getattr(p, 'stats', None), 'layout': getattr(p, 'plate_layout', None),
                    'chunk': getattr(p, 'chunk', None)}.get(key, val)
            if val is not None and have is not None and have != val:
                import warnings
                warnings.warn('the existing plan was built with %s=%r; %s=%r asks for a new one '
                              '(posterior state starts again from the nodes\' initialisation)'
                              % (key, have, key, val))
                return None
    return plans


def compile_model(nodes, engine=None, **options):
    """Cover the stochastic nodes of ``nodes`` with plans.  Raises
    NotImplementedError (loudly -- there is no CPU fallback) when a node is not
    covered by any built plan."""
    from ...nodes.node import Stochastic
    import os
    if engine is None:
        engine = os.environ.get('BAYESPY_AMD_ENGINE', 'auto')
    gaussian = engine == 'fused+batches+gaussian'
    batches = gaussian or engine == 'fused+batches'
    hyper = engine in ('fused+hyper', 'fused+topics+hyper')
    topics = engine in ('fused+topics', 'fused+topics+hyper')
    if batches or topics or hyper:
        engine = 'fused'
    kept = _reusable_plans(nodes, engine, options)
    if kept is not None and not topics \
            and any(type(p) in v for p in kept for v in OPT_IN_TOPICS.values()):
        kept = None             # the wide-topic form is kept only where it is asked for
    if kept is not None and not hyper \
            and any(type(p) in v for p in kept for v in OPT_IN_HYPER.values()):
        kept = None             # a form with learnt concentrations is kept only where it is asked for
    if kept is not None and not batches \
            and any(type(p) in v for p in kept for v in OPT_IN_BATCHES.values()):
        kept = None             # a mini-batch form is kept only where it is asked for
    if kept is not None and not gaussian \
            and any(type(p) in v for p in kept for v in OPT_IN_GAUSSIAN_BATCHES.values()):
        kept = None
    if kept is not None:
        return kept
    stale = [n.name for n in nodes if isinstance(n, Stochastic) and n._plan is not None
             and getattr(n._plan, 'has_state', lambda: False)()]
    if stale:
        import warnings
        warnings.warn('nodes %s already hold posterior state in another execution plan; the new '
                      'plan starts from their initialisation' % ', '.join(stale))
    if engine == 'generic':
        from .generic import GenericPlan
        plan = GenericPlan(nodes)
        plan._engine_request = 'generic'
        return [plan]
    types = [Q for P in PLAN_TYPES for Q in [OPT_IN_FORMS.get(P, P)] + OPT_IN_AFTER.get(P, [])] \
        + _with_masked(opt_in_types() + OPT_IN_MORE) + OPT_IN_LAST + OPT_IN_COUNTS \
        + OPT_IN_VECTORS + OPT_IN_TRIALS \
        if engine == 'fused' \
        else PLAN_TYPES
    if batches:
        types = _with_batches(types)
    if gaussian:
        types = _with_gaussian_batches(types)
    if topics:
        types = _with_topics(types)
    if hyper:
        types = _with_hyper(types)
    remaining = [n for n in nodes]
    plans = []
    progress = True
    while progress:
        progress = False
        for P in types:
            roles = P.match(remaining)
            if roles is not None:
                plan = P(roles, **options)
                plans.append(plan)
                used = set(id(n) for n in roles.values())
                remaining = [n for n in remaining if id(n) not in used]
                progress = True
                break
    left = [n for n in remaining if isinstance(n, Stochastic)]
    if left and engine == 'fused':
        why = []
        for P in types:
            try:
                P.match(remaining, why)
            except TypeError:       # a test double without the diagnostic argument
                pass
        for p in plans:                 # the blocks that did match let go of their nodes
            for n in p.nodes():
                n._plan = None
        raise NotImplementedError(
            "engine='fused': no fused block covers %s%s" % (
                ', '.join(n.name for n in left),
                ' -- ' + '; '.join(dict.fromkeys(why)) if why else
                ' (the blocks: ' + '; '.join(P.describe() for P in types
                                             if hasattr(P, 'describe')) + ')'))
    if left:
        # nodes outside the fused blocks: the whole model runs on the generic device
        # message-passing engine (raises NotImplementedError for unknown node types).  A model
        # that RESEMBLES a fused block but misses its matcher is told why: the generic engine
        # keeps the reference's per-plate arrays ((N, K, K) second moments, (N, K, D, D) mixture
        # intermediates), which is the difference between milliseconds and out-of-memory at
        # large N.
        why = []
        for P in PLAN_TYPES:
            try:
                P.match(remaining, why)
            except TypeError:       # a test double without the diagnostic argument
                pass
        if why:
            import warnings
            warnings.warn('this model runs on the generic message-passing engine, not on a fused '
                          'block -- ' + '; '.join(dict.fromkeys(why))
                          + ' (engine="generic" selects this engine silently)',
                          stacklevel=3)
        from .generic import GenericPlan
        return [GenericPlan(nodes)]
    return plans
