"""
The full-covariance Gaussian-mixture block (plans/gmm.py) for 33 to 64 dimensions: the
high-dimensional form

``GMMPlan`` contracts over the compact feature list [y_a y_b (a <= b), y, 1] and keeps one matrix
element per lane in its per-cluster kernels, so it stops at D = 32.  ``HighDimGMMPlan`` is the same
plan -- the same state in HBM, updates, bound, moments and checkpoints -- on the kernels
``vmp_gmm_hd_*`` (csrc/vmp_gmm_hd.hip): the responsibilities and the statistics are products with
the D x D matrices themselves on the fp64 matrix cores, the per-cluster kernels keep their matrix
in LDS.  Nothing of size (N, K, D) exists.

Opt-in: ``VB(..., engine='fused+dims')``, which is ``engine='fused'`` plus the forms of
``plans.OPT_IN_HIGH_DIMS``, each tried right after its block.  Every other engine value keeps its
answer for such a model: the default runs it on the generic engine with the block's warning, the
``'fused...'`` values raise with its reason.  D <= 32 is declined here ("use the Gaussian-mixture
block"), so this form never takes a model from ``GMMPlan``.
"""
import ctypes

import numpy as np

from .gmm import GMMKernels, GMMPlan

from ... import _lib
from ...device import ptr

LABEL = 'fused Gaussian-mixture block (high dimensions)'
MIN_D, MAX_D, MAX_K = 33, 64, 64


class HighDimGMMKernels(GMMKernels):
    """``GMMKernels`` on the ``vmp_gmm_hd_*`` entry points (no annealed and no natural-gradient
    forms are built: the plan has ``ANNEALING = False``)."""

    def layout(self, D, K):
        L = _lib.GMMLayout()
        rc = self.lib.vmp_gmm_hd_get_layout(D, K, ctypes.byref(L))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the high-dimensional form of the fused GMM block supports '
                                      'D <= %d and K <= %d' % (MAX_D, MAX_K))
        return L

    def workspace_doubles(self, D, K):
        n = ctypes.c_size_t()
        self.rt.check(self.lib.vmp_gmm_hd_workspace_bytes(self.ctx, D, K, ctypes.byref(n)))
        return (n.value + 7) // 8

    def init_state(self, D, K, alpha0, beta0, n0, V0, state):
        a = np.ascontiguousarray(alpha0, dtype=np.float64)
        v = np.ascontiguousarray(V0, dtype=np.float64)
        self.rt.check(self.lib.vmp_gmm_hd_init_state(
            self.ctx, D, K, a.ctypes.data_as(ctypes.c_void_p), float(beta0), float(n0),
            v.ctypes.data_as(ctypes.c_void_p), ptr(state)))

    def stats_from_labels(self, Y, N, D, K, labels, R, state, ws):
        self.rt.check(self.lib.vmp_gmm_hd_stats_from_labels(self.ctx, ptr(Y), N, D, K, ptr(labels),
                                                            ptr(R), ptr(state), ptr(ws)))

    def update_mu(self, D, K, state):
        self.rt.check(self.lib.vmp_gmm_hd_update_mu(self.ctx, D, K, ptr(state)))

    def update_lambda(self, D, K, state):
        self.rt.check(self.lib.vmp_gmm_hd_update_lambda(self.ctx, D, K, ptr(state)))

    def prepare_z(self, D, K, prior_only, state):
        self.rt.check(self.lib.vmp_gmm_hd_prepare_z(self.ctx, D, K, 1 if prior_only else 0,
                                                    ptr(state)))

    def pass_(self, Y, N, D, K, R, state, ws):
        self.rt.check(self.lib.vmp_gmm_hd_pass(self.ctx, ptr(Y), N, D, K, ptr(R), ptr(state),
                                               ptr(ws)))

    def update_alpha(self, D, K, state):
        self.rt.check(self.lib.vmp_gmm_hd_update_alpha(self.ctx, D, K, ptr(state)))

    def lower_bound(self, D, K, state):
        self.rt.check(self.lib.vmp_gmm_hd_lower_bound(self.ctx, D, K, ptr(state)))


class HighDimGMMPlan(GMMPlan):
    """``GMMPlan`` for 33 <= D <= 64 on the ``vmp_gmm_hd_*`` kernels.  Opt-in:
    ``VB(..., engine='fused+dims')``, tried right after the Gaussian-mixture block."""

    KIND = 'gmm_hd'
    ANNEALING = False       # no annealed kernels in this form

    @staticmethod
    def _annealing(node):
        b = float(getattr(node, 'annealing', 1.0))
        if b != 1.0:
            raise NotImplementedError(
                "annealing is not built into the fused HighDimGMMPlan plan; build the engine with "
                "VB(..., engine='generic')")
        return b

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const)), Gaussian, GaussianARD(0, const, "
                "shape=(D,), plates=(K,)), Wishart(const, const, plates=(K,))), fully observed, "
                "%d <= D <= %d, K <= %d" % (MIN_D, MAX_D, MAX_K))

    @staticmethod
    def _dims(D, K):
        if D < MIN_D:
            return 'D = %d: use the Gaussian-mixture block (it takes D <= %d)' % (D, MIN_D - 1)
        if D > MAX_D or K > MAX_K:
            return ('D = %d, K = %d exceed the limits of this form (D <= %d, K <= %d)'
                    % (D, K, MAX_D, MAX_K))
        return None

    @staticmethod
    def match(nodes, why=None):
        """``GMMPlan.match`` with the limits of this form; mini-batches (which the block passes over
        in silence) and sharded plates are declined with a reason."""
        from ...nodes.gaussian import Gaussian
        from ...nodes.mixture import Mixture
        for Y in nodes:
            if not isinstance(Y, Mixture) or Y.node_class is not Gaussian:
                continue
            bad = None
            if any(any(m != 1 for m in n.plates_multiplier) for n in nodes):
                bad = 'a node carries a plates_multiplier (mini-batches)'
            elif any(getattr(n, '_shard_axis', None) is not None for n in [Y] + list(Y.parents)):
                bad = 'its plates are sharded over ranks (Node.shard)'
            if bad:
                if why is not None:
                    why.append('%s, observed node %s: %s' % (LABEL, Y.name or '<unnamed>', bad))
                return None
        return GMMPlan.match(nodes, why, label=LABEL, dims_rule=HighDimGMMPlan._dims)

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = HighDimGMMKernels(self.rt)
        return self._kernels

