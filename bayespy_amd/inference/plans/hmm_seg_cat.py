"""
The discrete hidden-Markov-model block (plans/hmm_cat.py) for few long chains: the segmented,
time-parallel form

``CategoricalHMMPlan`` walks a chain one step at a time on one lane group: 2 (T - 1) dependent
steps, whatever the device has idle -- and the opening model of hmm.rst is one long sequence of
words.  ``SegmentedCategoricalHMMPlan`` is the same plan -- the same state in HBM, constants or
Dirichlet nodes for ``a0``, ``A`` and ``P``, masks of the full plate shape, the same bound from the
sums -- on the pass ``vmp_hmm_seg_pass_categorical`` (csrc/vmp_hmm_seg_cat.hip): the chain is cut
into segments of ``seg_len`` transitions, the K x K transfer of every segment is formed in parallel
with the <log P> table resident in LDS, one lane group carries the forward and backward state
across the segment boundaries, the recursion then runs inside all segments at once, and the count
table S is formed from the posterior by a histogram kernel of its own.  K <= 64, M <= 128.

``seg_len`` (attribute, default 0 = the library's choice for (B, T, K); set it before the first
update) is the number of transitions of a segment; any value of T - 1 or more is one segment.

Opt-in: ``VB(..., engine='fused+chains')``, which is ``engine='fused'`` with the forms of
``plans.OPT_IN_LONG_CHAINS`` standing in their block's place.  Every other engine value keeps its
answer and never keeps such a plan on reuse.
"""
import ctypes

from .hmm_cat import CatHMMKernels, CategoricalHMMPlan, _match

from ... import _lib
from ...device import ptr

LABEL = 'fused hidden-Markov-model block (long chains, categorical)'
_LIMITS = []


def hmm_seg_cat_limits():
    """(max K, max M) of the built pass: host-only ``vmp_hmm_seg_cat_limits``."""
    if not _LIMITS:
        k, m = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_hmm_seg_cat_limits(ctypes.byref(k), ctypes.byref(m)))
        _LIMITS.append((k.value, m.value))
    return _LIMITS[0]


class SegmentedCatHMMKernels(CatHMMKernels):

    seg_len = 0

    def plan(self, B, T, M, K):
        """(segment length in use, workspace doubles) of the pass for ``self.seg_len``."""
        used, w = ctypes.c_int32(), ctypes.c_int64()
        rc = self.lib.vmp_hmm_seg_cat_plan(B, T, M, K, int(self.seg_len), ctypes.byref(used),
                                           ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the long-chain form of the fused hidden-Markov-model block '
                                      'with categorical emissions supports T >= 2, seg_len >= 0, '
                                      'K <= %d and M <= %d' % hmm_seg_cat_limits())
        return used.value, w.value

    def pass_(self, B, T, M, K, y, elogPt, elog_a0, elog_A, labels, mask, ws, z0sum, xisum, S, scal,
              gamma=None, z0=None, zz=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_hmm_seg_pass_categorical(
            self.ctx, B, T, M, K, p(y), p(elogPt), p(elog_a0), p(elog_A), p(labels), p(mask),
            p(ws), p(z0sum), p(xisum), p(S), p(scal), p(gamma), p(z0), p(zz), int(self.seg_len)))


class SegmentedCategoricalHMMPlan(CategoricalHMMPlan):
    """``CategoricalHMMPlan`` on the time-parallel pass.  Opt-in:
    ``VB(..., engine='fused+chains')``, in the discrete HMM block's place."""

    _KIND, _EMISSIONS = 'hmm_seg_cat', 'categorical (the long-chain form)'

    def __init__(self, roles, runtime=None, kernels=None):
        super().__init__(roles, runtime, kernels)
        self._seg_len = 0

    @property
    def seg_len(self):
        """Transitions of a segment; 0 = the library's choice.  ``chains_per_wg`` of the
        materialised plan holds the length in use."""
        return self._seg_len

    @seg_len.setter
    def seg_len(self, value):
        value = int(value)
        if value < 0:
            raise ValueError('seg_len must be 0 (the library chooses) or positive')
        changed, self._seg_len = value != self._seg_len, value
        if self._ready and changed:
            # the workspace depends on the length; the sums do not
            self.chains_per_wg, wsd = self.kernels.plan(self.B, self.T, self.M, self.K)
            if int(wsd) > self.ws.numel():
                self.ws = self.rt.empty(int(wsd))

    @staticmethod
    def describe():
        return (CategoricalHMMPlan.describe().rsplit(', M <=', 1)[0]
                + ', M <= %d, K <= %d, parallel over time'
                % (hmm_seg_cat_limits()[1], hmm_seg_cat_limits()[0]))

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, label=LABEL, limits=hmm_seg_cat_limits)

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = SegmentedCatHMMKernels(self.rt)
        self._kernels.seg_len = self._seg_len
        return self._kernels
