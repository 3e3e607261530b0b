"""
The discrete hidden-Markov-model block (plans/hmm_cat.py) for large vocabularies: 129 to 65536 words

``CategoricalHMMPlan`` stops at M = 128 because its pass keeps a count histogram of M doubles per
lane in LDS.  ``VocabCategoricalHMMPlan`` is the same plan -- the same state in HBM, constants or
Dirichlet nodes for ``a0``, ``A`` and ``P``, masks of the full plate shape, fixed labels, the same
bound from the sums, ``save`` / ``load`` -- on the pass ``vmp_hmm_vocab_pass``
(csrc/vmp_hmm_vocab.hip): a chain kernel runs the recursion alone, gathers <log P>[y_t] from the
word-major table ahead of the step that uses it and leaves the posterior in the workspace; a count
kernel forms S (M, K) from it as a segmented sum over a WORD LAYOUT of the observed steps (their
positions sorted by word, and the first entry of every word), and a third kernel adds the
partials.  Nothing a workgroup keeps grows with M.  K <= 64.

The layout is built once per observation, beside the upload of ``y``: one stable ``torch.sort`` of
the observed words, a bincount and a cumsum.

Opt-in: ``VB(..., engine='fused+words')``, which is ``engine='fused'`` with the forms of
``plans.OPT_IN_WORDS`` tried right after their block.  Every other engine value keeps its answer
and never keeps such a plan on reuse.
"""
import ctypes

from .hmm_cat import CatHMMKernels, CategoricalHMMPlan, _match, hmm_cat_limits

from ... import _lib
from ...device import ptr

LABEL = 'fused hidden-Markov-model block (large vocabulary)'
_LIMITS = []


def hmm_vocab_limits():
    """(max K, max M) of the built pass: host-only ``vmp_hmm_vocab_limits``."""
    if not _LIMITS:
        k, m = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_hmm_vocab_limits(ctypes.byref(k), ctypes.byref(m)))
        _LIMITS.append((k.value, m.value))
    return _LIMITS[0]


def word_layout(torch, y, mask, M):
    """(order, word_offsets) of ``vmp_hmm_vocab_pass`` for ``y`` (B, T) int32 and ``mask`` (B, T)
    uint8 or None, on the device of ``y``: the positions b T + t of the observed steps with a word
    in [0, M), sorted by word and by ascending position inside a word (int32), and the index of
    every word's first entry, M + 1 int32."""
    flat = y.reshape(-1).to(torch.int64)
    seen = (flat >= 0) & (flat < M)
    if mask is not None:
        seen &= mask.reshape(-1) != 0
    pos = torch.nonzero(seen).reshape(-1)
    words, idx = torch.sort(flat[pos], stable=True)
    offsets = torch.zeros(M + 1, dtype=torch.int64, device=y.device)
    offsets[1:] = torch.cumsum(torch.bincount(words, minlength=M), 0)
    return pos[idx].to(torch.int32).contiguous(), offsets.to(torch.int32)


class VocabCatHMMKernels(CatHMMKernels):

    layout = None           # (order, word_offsets) of the plan; None: built per call

    def plan(self, B, T, M, K):
        """(chains of a workgroup, workspace doubles) of the pass; the workspace serves every
        layout of the shape (n_obs <= B T)."""
        c, ch, w = ctypes.c_int64(), ctypes.c_int32(), ctypes.c_int64()
        rc = self.lib.vmp_hmm_vocab_plan(B, T, M, K, B * T, ctypes.byref(c), ctypes.byref(ch),
                                         ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the large-vocabulary form of the fused hidden-Markov-model '
                                      'block supports T >= 2, B T < 2^31, K <= %d and M <= %d'
                                  % hmm_vocab_limits())
        return c.value, w.value

    def pass_(self, B, T, M, K, y, elogPt, elog_a0, elog_A, labels, mask, ws, z0sum, xisum, S, scal,
              gamma=None, z0=None, zz=None):
        def p(t):
            return ptr(t) if t is not None and t.numel() else None
        order, offsets = self.layout or word_layout(self.rt.torch, y, mask, M)
        self.rt.check(self.lib.vmp_hmm_vocab_pass(
            self.ctx, B, T, M, K, p(y), p(elogPt), p(elog_a0), p(elog_A), p(labels), p(mask),
            order.numel(), p(order), p(offsets), p(ws), p(z0sum), p(xisum), p(S), p(scal),
            p(gamma), p(z0), p(zz)))


class VocabCategoricalHMMPlan(CategoricalHMMPlan):
    """``CategoricalHMMPlan`` on the large-vocabulary pass.  Opt-in:
    ``VB(..., engine='fused+words')``, tried right after the discrete HMM block."""

    _KIND, _EMISSIONS = 'hmm_vocab', 'categorical (the large-vocabulary form)'

    def __init__(self, roles, runtime=None, kernels=None):
        super().__init__(roles, runtime, kernels)
        self._layout = None

    @staticmethod
    def describe():
        return (CategoricalHMMPlan.describe().rsplit(', M <=', 1)[0]
                + ', %d <= M <= %d, K <= %d' % ((hmm_cat_limits()[1] + 1,) + hmm_vocab_limits()[::-1]))

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, label=LABEL, limits=hmm_vocab_limits,
                      min_M=hmm_cat_limits()[1] + 1,
                      below='use the discrete HMM block (M <= %d)' % hmm_cat_limits()[1])

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = VocabCatHMMKernels(self.rt)
        self._kernels.layout = self._layout
        return self._kernels

    def _upload_y(self):
        super()._upload_y()
        self._layout = word_layout(self.rt.torch, self.yd, self.maskd, self.M)
