"""
The multinomial-emission hidden-Markov-model block (plans/hmm_mult.py) for 65 to 128 states:
chromatin-state models over k-mer or mark counts, topic-segment and part-of-speech models over word
histograms, sub-phone states

    Z = CategoricalMarkovChain(a0, A, states=T)             plates () or (B,)
    Y = Mixture(Z, Multinomial, n, P);  Y.observe(x)        plates (T,) or (B, T), x (..., M)

with everything else exactly what ``MultinomialHMMPlan`` accepts (M <= 1024, counts of at most
65534, full-shape masks, labels); a categorical emission is the n = 1 case.

``WideStateMultinomialHMMPlan`` is ``MultinomialHMMPlan`` -- the pack, the tables, the Dirichlet
rows, masks, labels and ``save`` / ``load`` are inherited -- with the pass ``vmp_hmm_states_pass``
(csrc/vmp_hmm_states.hip): the lane-per-state chain kernel stops at 64 states, so the recursion
runs in the domain of scaled probabilities with its K x K products on the fp64 matrix cores.
What that gives up is range: an entry of <log A> below about -745 acts as -inf, and a step whose
predicted mass underflows entirely gives NaN, as an impossible observation does.

Opt-in: ``VB(..., engine='fused+states')``, which is ``engine='fused+counts'`` with the forms of
``plans.OPT_IN_WIDE_STATES`` tried right after their block (which declines K > 64 with a reason).
Every other engine value keeps its answer and never keeps such a plan on reuse.
"""
import ctypes

from .hmm_cat import _match
from .hmm_mult import MultHMMKernels, MultinomialHMMPlan, _trials_reason

from ... import _lib
from ...device import ptr
from ...nodes.multinomial import Multinomial

LABEL = 'fused hidden-Markov-model block (multinomial emissions, 65 to 128 states)'
_LIMITS = []


def hmm_states_limits():
    """(max K, min K, max M, largest count) of the built pass: host-only ``vmp_hmm_states_limits``."""
    if not _LIMITS:
        v = [ctypes.c_int32() for _ in range(4)]
        _lib.raise_for_status(_lib.load().vmp_hmm_states_limits(*[ctypes.byref(a) for a in v]))
        _LIMITS.append(tuple(a.value for a in v))
    return _LIMITS[0]


def _states_reason(Y):
    max_K, min_K = hmm_states_limits()[:2]
    K = Y.parents[0].parents[0].categories
    if K < min_K:
        return ('K = %d: the wide-state form takes %d <= K <= %d; the block with multinomial '
                'emissions takes fewer states' % (K, min_K, max_K))
    return _trials_reason(Y)


class WideStateHMMKernels(MultHMMKernels):

    def plan(self, B, T, M, K):
        """(chains of a workgroup, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_hmm_states_plan(B, T, M, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            lim = hmm_states_limits()
            _lib.raise_for_status(rc, 'the %s supports T >= 2, %d <= K <= %d, M <= %d and counts '
                                      'of at most %d' % (LABEL, lim[1], lim[0], lim[2], lim[3]))
        return c.value, w.value

    def pass_(self, B, T, M, K, xp, elogPt, elog_a0, elog_A, labels, mask, ws, z0sum, xisum, S,
              scal, gamma=None, z0=None, zz=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_hmm_states_pass(
            self.ctx, B, T, M, K, p(xp), p(elogPt), p(elog_a0), p(elog_A), p(labels), p(mask),
            p(ws), p(z0sum), p(xisum), p(S), p(scal), p(gamma), p(z0), p(zz)))


class WideStateMultinomialHMMPlan(MultinomialHMMPlan):
    """``MultinomialHMMPlan`` for 65 to 128 states.  Opt-in: ``VB(..., engine='fused+states')``,
    tried right after the multinomial-emission block."""

    _KIND, _EMISSIONS = 'hmm_states', 'multinomial (the wide-state form, 65 <= K <= 128)'

    @staticmethod
    def describe():
        lim = hmm_states_limits()
        return ("Mixture(CategoricalMarkovChain(a0, A, states=T), Multinomial, n, P) as the block "
                "with multinomial emissions takes it, with %d <= K <= %d, M <= %d, counts of at "
                "most %d; the chain pass works with scaled probabilities, so an entry of <log A> "
                "below about -745 acts as -inf" % (lim[1], lim[0], lim[2], lim[3]))

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, label=LABEL,
                      limits=lambda: (hmm_states_limits()[0], hmm_states_limits()[2]),
                      family=Multinomial, extra=_states_reason)

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = WideStateHMMKernels(self.rt)
        return self._kernels
