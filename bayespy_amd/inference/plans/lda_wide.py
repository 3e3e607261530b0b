"""
The latent-Dirichlet-allocation block (plans/lda.py) with 65 to 1024 topics: the wide-topic form

``LDAPlan`` puts the K topics of a token into one lane group of at most 64 lanes, so it stops at
K = 64.  ``WideLDAPlan`` is the same plan -- the same state in HBM, the same two sorted layouts, the
same bound from the counts, sum lse and the tables, the same Dirichlet rows and dot products, which
are general in K -- on the token pass ``vmp_lda_wide_token_pass`` (csrc/vmp_lda_wide.hip): one
wavefront walks a chunk of tokens and every lane holds K / 64 topics in registers.  Nothing of size
tokens x K exists outside ``topics.get_moments()``.

Opt-in: ``VB(..., engine='fused+topics')``, which is ``engine='fused'`` plus the forms of
``plans.OPT_IN_TOPICS``, each tried right after its block.  Every other engine value keeps its
answer for a model with more than 64 topics: the default runs it on the generic engine with the LDA
block's reason, ``'fused'`` raises with it.  K <= 64 is declined here ("use the LDA block"), so this
form never takes a model from ``LDAPlan``.

Scope: the full sweeps of lda.rst.  Mini-batches (``plates_multiplier``, ``gradient_step``) at more
than 64 topics are declined with a reason.
"""
import ctypes

from .lda import LDAKernels, LDAPlan, LDA_MAX_K, _match

from ... import _lib
from ...device import ptr

LDA_WIDE_MIN_K = LDA_MAX_K + 1      # vmp_lda_wide_limits
LDA_WIDE_MAX_K = 1024

LABEL = 'fused LDA block (wide topics)'


class WideLDAKernels(LDAKernels):

    def plan(self, n, K):
        """(registers per lane, tokens per chunk, workspace doubles) of the token pass."""
        r, c, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        rc = self.lib.vmp_lda_wide_plan(n, K, ctypes.byref(r), ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the wide-topic form of the fused LDA block supports '
                                      '%d <= K <= %d and fewer than 2^31 tokens'
                                      % (LDA_WIDE_MIN_K, LDA_WIDE_MAX_K))
        return r.value, c.value, w.value

    def token_pass(self, n, D, V, K, lay, labels, elog_theta, elog_beta_t, phases, lse, ws, Ndk,
                   Nvk, scal, orig=None, phi=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_lda_wide_token_pass(
            self.ctx, n, D, V, K, p(lay['doc_d']), p(lay['word_d']), p(lay['doc_off']),
            p(lay['word_w']), p(lay['doc_w']), p(lay['pos_w']), p(lay['word_off']), p(labels),
            p(elog_theta), p(elog_beta_t), phases, p(lse), p(ws), p(Ndk), p(Nvk), p(scal),
            p(orig), p(phi)))


def _no_batches(words, topics, p_word, p_topic):
    if any(any(m != 1 for m in n.plates_multiplier) for n in (words, topics, p_word, p_topic)):
        return ('plates_multiplier (mini-batches, stochastic VI) is not built for more than %d '
                'topics; it goes through the generic engine' % LDA_MAX_K)
    return None


def _wide_topics(K):
    if K <= LDA_MAX_K:
        return 'n_topics = %d: use the LDA block (it takes K <= %d)' % (K, LDA_MAX_K)
    if K > LDA_WIDE_MAX_K:
        return 'n_topics = %d exceeds the limit of this form (K <= %d)' % (K, LDA_WIDE_MAX_K)
    return None


class WideLDAPlan(LDAPlan):
    """``LDAPlan`` for 65 <= K <= 1024 on the wide-topic token pass.  Opt-in:
    ``VB(..., engine='fused+topics')``, tried right after the LDA block."""

    _KIND = 'lda_wide'

    @staticmethod
    def describe():
        return ("Categorical(Gate(Categorical(Gate(indices, Dirichlet(const, plates=(D,))), "
                "plates=(n,)), Dirichlet(const, plates=(K,)))), fully observed, %d <= K <= %d"
                % (LDA_WIDE_MIN_K, LDA_WIDE_MAX_K))

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, _no_batches, label=LABEL, topics_rule=_wide_topics)

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = WideLDAKernels(self.rt)
        return self._kernels

    def gradient_step(self, nodes, scale=1.0):
        raise NotImplementedError(
            '%s: gradient steps (stochastic VI) are not built for more than %d topics; use '
            'VB(..., engine="generic")' % (LABEL, LDA_MAX_K))
