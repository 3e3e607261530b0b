"""
The hidden-Markov-model block (plans/hmm.py) for few long chains: the segmented, time-parallel form

``HMMPlan`` and ``WideHMMPlan`` walk a chain one step at a time on one lane group: 2 (T - 1)
dependent steps, whatever the device has idle.  That suits 2e4 short chains and fails the model of
hmm.rst, a single sequence.  ``SegmentedHMMPlan`` is the same plan -- the same state in HBM, forms
(a) and (b), masks of the full plate shape, the same bound from the sums -- on the pass
``vmp_hmm_seg_pass`` (csrc/vmp_hmm_seg.hip): the chain is cut into segments of ``seg_len``
transitions, the K x K transfer of every segment is formed in parallel, one lane group carries the
forward and backward state across the segment boundaries, and the recursion then runs inside all
segments at once.  The emission table and the statistics are the matrix-core kernels of the
wide-emission form, so every Gaussian emission width of the block is served: 1 <= D <= 32, K <= 64.

``seg_len`` (attribute, default 0 = the library's choice for (B, T, K); set it before the first
update) is the number of transitions of a segment; any value of T - 1 or more is one segment.

Opt-in: ``VB(..., engine='fused+chains')``, which is ``engine='fused'`` with the forms of
``plans.OPT_IN_LONG_CHAINS`` standing in their block's place.  Every other engine value keeps its
answer and never keeps such a plan on reuse.  Categorical emissions: plans/hmm_seg_cat.py.
"""
import ctypes

from .hmm import HMMKernels, HMMPlan, _match

from ... import _lib
from ...device import ptr

LABEL = 'fused hidden-Markov-model block (long chains)'
_LIMITS = []


def hmm_seg_limits():
    """(max K, max D) of the built pass: host-only ``vmp_hmm_seg_limits``."""
    if not _LIMITS:
        k, d = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_hmm_seg_limits(ctypes.byref(k), ctypes.byref(d)))
        _LIMITS.append((k.value, d.value))
    return _LIMITS[0]


class SegmentedHMMKernels(HMMKernels):

    seg_len = 0

    def plan(self, B, T, D, K):
        """(segment length in use, workspace doubles) of the pass for ``self.seg_len``."""
        used, w = ctypes.c_int32(), ctypes.c_int64()
        rc = self.lib.vmp_hmm_seg_plan(B, T, D, K, int(self.seg_len), ctypes.byref(used),
                                       ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the long-chain form of the fused hidden-Markov-model block '
                                      'supports T >= 2, seg_len >= 0, K <= %d and D <= %d'
                                      % hmm_seg_limits())
        return used.value, w.value

    def pass_(self, B, T, D, K, Y, C, ldc, elog_a0, elog_A, labels, ws, z0sum, xisum, Tstat, scal,
              gamma=None, z0=None, zz=None, mask=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_hmm_seg_pass(
            self.ctx, B, T, D, K, p(Y), p(C), ldc, p(elog_a0), p(elog_A), p(labels), p(mask),
            p(ws), p(z0sum), p(xisum), p(Tstat), p(scal), p(gamma), p(z0), p(zz),
            int(self.seg_len)))


def _seg_dims(D, K):
    max_K, max_D = hmm_seg_limits()
    if K > max_K or D > max_D:
        return ('D = %d, K = %d exceed the limits of this form (D <= %d, K <= %d)'
                % (D, K, max_D, max_K))
    return None


class SegmentedHMMPlan(HMMPlan):
    """``HMMPlan`` for 1 <= D <= 32 on the time-parallel pass.  Opt-in:
    ``VB(..., engine='fused+chains')``, in the HMM block's place."""

    _KIND, _EMISSIONS = 'hmm_seg', 'Gaussian (the long-chain form)'

    def __init__(self, roles, runtime=None, kernels=None):
        super().__init__(roles, runtime=runtime, kernels=kernels)
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
            self.chains_per_wg, wsd = self.kernels.plan(self.B, self.T, self.D, self.K)
            if int(wsd) > self.ws.numel():
                self.ws = self.rt.empty(int(wsd))

    @staticmethod
    def describe():
        return ("Mixture(CategoricalMarkovChain(Dirichlet(const), Dirichlet(const, plates=(K,)), "
                "states=T), Gaussian, mu, Lambda) as the HMM block takes it, D <= %d, K <= %d, "
                "parallel over time" % (hmm_seg_limits()[1], hmm_seg_limits()[0]))

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, label=LABEL, dims_rule=_seg_dims)

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = SegmentedHMMKernels(self.rt)
        self._kernels.seg_len = self._seg_len
        return self._kernels
