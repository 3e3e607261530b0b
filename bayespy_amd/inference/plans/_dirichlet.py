"""
What the blocks with Dirichlet tables share: the wrappers of ``vmp_lda_dirichlet`` /
``vmp_lda_dot`` and the host table of a constant concentration.  Its users are the plans of lda.py,
hmm.py, hmm_cat.py and the plate-mixture blocks (bmm.py, dgmm.py, dgmm_masked.py, cmm.py, pmm.py,
through _mixture.py for the mixing weights).
"""
import numpy as np

from ...device import ptr


class DirichletKernels:
    """Mixin of a kernels class that has ``rt``, ``lib`` and ``ctx``."""

    def dirichlet(self, rows, cols, rs, cs, prior, counts, alpha, elog, ws, bound):
        self.rt.check(self.lib.vmp_lda_dirichlet(
            self.ctx, rows, cols, rs, cs, ptr(prior), ptr(counts) if counts is not None else None,
            ptr(alpha), ptr(elog), ptr(ws), ptr(bound)))

    def natural_step_workspace(self, kind, rows, cols, K):
        """The doubles of ``ws`` that ``natural_step`` needs for a table of that shape."""
        import ctypes
        w = ctypes.c_int64()
        self.rt.check(self.lib.vmp_mix_natural_step_workspace(kind, rows, cols, K, ctypes.byref(w)))
        return w.value

    def natural_step(self, kind, nodes, rows, cols, rs, cs, prior, prior_b, stat, cnt, per_element,
                     par, mom, K, prior_r, Nk, alpha_r, elog_r, mult, scale, ws, bound):
        """``vmp_mix_natural_step``: the parameter table of a mixture block (bit 1 of ``nodes``)
        and its weights row (bit 2) one step along their natural gradients, in one launch."""
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_mix_natural_step(
            self.ctx, kind, nodes, rows, cols, rs, cs, p(prior), p(prior_b), p(stat), p(cnt),
            per_element, p(par), p(mom), K, p(prior_r), p(Nk), p(alpha_r), p(elog_r), float(mult),
            float(scale), p(ws), p(bound)))

    def dot(self, m, a, b, ws, out):
        self.rt.check(self.lib.vmp_lda_dot(self.ctx, m, ptr(a), ptr(b), ptr(ws), ptr(out)))


def prior_table(node, shape):
    """The constant concentration of the Dirichlet / Beta ``node``, broadcast to ``shape``."""
    a = np.asarray(node.parents[0].value, dtype=np.float64)
    if np.any(a <= 0):
        raise ValueError("Natural parameters should be positive")
    return np.ascontiguousarray(np.broadcast_to(a, shape))
