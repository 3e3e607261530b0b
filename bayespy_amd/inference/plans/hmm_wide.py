"""
The hidden-Markov-model block (plans/hmm.py) with Gaussian emissions of 9 to 32 dimensions: the
wide-emission form

``HMMPlan`` forms the emission term of a step inside the chain pass from NF = D (D + 1) / 2 + D + 1
features held in LDS, so it stops at D = 8.  ``WideHMMPlan`` is the same plan -- the same state in
HBM, forms (a) and (b), masks of the full plate shape, the same bound from the sums, the mixture
block's kernels for ``mu`` and ``Lambda``, which are built for D <= 32 -- on the pass
``vmp_hmm_wide_pass`` (csrc/vmp_hmm_wide.hip): the emission table E (B, T, KP) and the statistics
T_k are products on the fp64 matrix cores over the whole (b, t) plate, the chain kernel keeps the
recursion alone.  Nothing of size (B, T-1, K, K) exists outside ``Z.get_moments()``; the workspace
holds E and the forward state (B, T, K).

Opt-in: ``VB(..., engine='fused+emissions')``, which is ``engine='fused'`` plus the forms of
``plans.OPT_IN_WIDE_EMISSIONS``, each tried right after its block.  Every other engine value keeps
its answer for such a model: the default runs it on the generic engine with the HMM block's reason,
the ``'fused...'`` values raise with it.  D <= 8 is declined here ("use the HMM block"), so this form
never takes a model from ``HMMPlan``.
"""
import ctypes

from .hmm import HMMKernels, HMMPlan, _match

from ... import _lib
from ...device import ptr

LABEL = 'fused hidden-Markov-model block (wide emissions)'
_LIMITS = []


def hmm_wide_limits():
    """(max K, max D) of the built pass: host-only ``vmp_hmm_wide_limits``."""
    if not _LIMITS:
        k, d = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_hmm_wide_limits(ctypes.byref(k), ctypes.byref(d)))
        _LIMITS.append((k.value, d.value))
    return _LIMITS[0]


def hmm_wide_min_d():
    from .hmm import hmm_limits
    return hmm_limits()[1] + 1


class WideHMMKernels(HMMKernels):

    def plan(self, B, T, D, K):
        """(chains of a workgroup of the chain kernel, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_hmm_wide_plan(B, T, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the wide-emission form of the fused hidden-Markov-model '
                                      'block supports T >= 2, K <= %d and D <= %d'
                                      % hmm_wide_limits())
        return c.value, w.value

    def pass_(self, B, T, D, K, Y, C, ldc, elog_a0, elog_A, labels, ws, z0sum, xisum, Tstat, scal,
              gamma=None, z0=None, zz=None, mask=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_hmm_wide_pass(
            self.ctx, B, T, D, K, p(Y), p(C), ldc, p(elog_a0), p(elog_A), p(labels), p(mask),
            p(ws), p(z0sum), p(xisum), p(Tstat), p(scal), p(gamma), p(z0), p(zz)))


def _wide_dims(D, K):
    max_K, max_D = hmm_wide_limits()
    if D < hmm_wide_min_d():
        return 'D = %d: use the HMM block (it takes D <= %d)' % (D, hmm_wide_min_d() - 1)
    if K > max_K or D > max_D:
        return ('D = %d, K = %d exceed the limits of this form (D <= %d, K <= %d)'
                % (D, K, max_D, max_K))
    return None


class WideHMMPlan(HMMPlan):
    """``HMMPlan`` for 9 <= D <= 32 on the wide-emission pass.  Opt-in:
    ``VB(..., engine='fused+emissions')``, tried right after the HMM block."""

    _KIND, _EMISSIONS = 'hmm_wide', 'Gaussian (the wide form, 9 <= D <= 32)'

    @staticmethod
    def describe():
        return ("Mixture(CategoricalMarkovChain(Dirichlet(const), Dirichlet(const, plates=(K,)), "
                "states=T), Gaussian, mu, Lambda) as the HMM block takes it, %d <= D <= %d, K <= %d"
                % (hmm_wide_min_d(), hmm_wide_limits()[1], hmm_wide_limits()[0]))

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, label=LABEL, dims_rule=_wide_dims)

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = WideHMMKernels(self.rt)
        return self._kernels
