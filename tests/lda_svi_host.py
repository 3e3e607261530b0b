"""TEST INFRASTRUCTURE for the mini-batch form of the fused latent-Dirichlet-allocation block
(inference/plans/lda.py LDASVIPlan): ``CPULDASVIKernels`` adds the Dirichlet step of
``vmp_lda_dirichlet_step`` in NumPy / SciPy to the kernel double of tests/lda_host.py.
It lives under tests/ and is never imported by the product."""
import numpy as np

from scipy import special

from lda_host import CPULDAKernels


def dirichlet_step_rows(prior, counts, mult, scale, alpha):
    """(alpha, elog, bound) of vmp_lda_dirichlet_step for rows x cols arrays: q = prior + mult *
    counts, alpha <- q for scale == 1 (the old alpha is not read), else alpha + scale * (q - alpha);
    elog and the bound are the formulas of lda_host.dirichlet_rows at the new alpha."""
    q = prior + (0.0 if counts is None else mult * counts)
    new = q if scale == 1 else alpha + scale * (q - alpha)
    elog = special.digamma(new) - special.digamma(new.sum(-1, keepdims=True))

    def g(a):
        return special.gammaln(a.sum(-1)) - special.gammaln(a).sum(-1)
    bound = float(np.sum((prior - new) * elog) + np.sum(g(prior) - g(new)))
    return new, elog, bound


class CPULDASVIKernels(CPULDAKernels):

    def dirichlet_step_ws(self, rows, cols, rs, cs):
        return max(rows, 1)

    def dirichlet_step(self, rows, cols, rs, cs, prior, counts, mult, scale, alpha, elog, ws,
                       bound):
        self.calls.append('dirichlet_step')

        def view(t):
            return np.lib.stride_tricks.as_strided(t.numpy().reshape(-1), shape=(rows, cols),
                                                   strides=(8 * rs, 8 * cs))
        al, el, b = dirichlet_step_rows(view(prior), None if counts is None else view(counts),
                                        mult, scale, view(alpha).copy())
        view(alpha)[...] = al
        view(elog)[...] = el
        bound.numpy()[...] = b
