"""
Stochastic variational inference on the two diagonal-Gaussian-mixture blocks (dgmm.py,
dgmm_masked.py): the recipe of bayespy/demos/stochastic_inference.py

    Z = Categorical(alpha, plates=(N, 1), plates_multiplier=(m, 1))
    Y = Mixture(Z, GaussianARD, mu, tau)
    per step:  Y.observe(next batch);  Q.update(Z);  Q.gradient_step(mu, tau, alpha, scale=s)

``Z`` and ``Y`` hold a mini-batch of N rows that stands for m times as many.  The bookkeeping is
``MixtureSVI`` (_mixture_svi.py): ``Y.observe`` keeps the device state and runs no pass, the
``update(Z)`` that follows forms the tables once and runs the pass once, whatever reads the
statistics before that runs the pass that is due first, the bound terms of ``Y`` and ``Z`` are
multiplied by m, and a checkpoint is the block's with the kind 'dgmm_svi'.

What differs is the step.  ``mu`` and ``tau`` are two tables, and the optimum of each reads the
moments of the other.  ``VB.gradient_step`` of the reference forms every node's gradient from the
state at entry and only then sets the parameters (vmp.py:432-440), and element (d, k) of ``mu``
couples only with element (d, k) of ``tau``: one thread reads both old moments, forms both optima
and writes both, so ``mu``, ``tau`` and the weights move in ONE launch (``vmp_dgmm_natural_step``,
csrc/vmp_dgmm_svi.hip):

    mu    in (lambda m, -lambda / 2):  lambda* = beta0 + m <tau> cnt,  (lambda m)* = beta0 m0 + m <tau> S1
    tau   in (a, b):                   a* = a0 + m cnt / 2,  b* = b0 + m (S2 - 2 <mu> S1 + <mu^2> cnt) / 2
    phi <- phi + scale (phi* - phi)

with cnt = N_k, or the count of the element M_dk in the block with missing observations.
``update(mu | tau | alpha)`` is that step with scale = 1.  A ``mu`` that is still a point mass steps
from the parameters of its prior, as on the generic engine.  A column of ``Y`` with nothing observed
in the batch has M = S = 0: its elements move toward the prior like any other, and the bound terms of
``mu`` and ``tau`` leave them out (expfamily.py:433-480: the mask of the node is False there).

Opt-in: ``VB(..., engine='fused+batches+gaussian')``, which is ``engine='fused+batches'`` plus the
forms of ``plans.OPT_IN_GAUSSIAN_BATCHES``, each tried right after its block; the other engine
values answer as before.  Declined with a reason: a multiplier on a global node, different or
non-positive factors on ``Z`` and ``Y``, a factor on another axis, sharded plates, and everything
the block itself declines.  No annealed form: a coefficient other than 1 is declined.
"""
import numpy as np

from . import _delta
from ._mixture import match_plate_mixture
from ._mixture_svi import MixtureSVI
from .dgmm import DiagGaussianMixturePlan, _SPEC, dgmm_limits
from .dgmm_masked import MaskedDiagGaussianMixturePlan, _MASKED_SPEC, dgmm_masked_limits


class DiagGaussianSVI(MixtureSVI):
    """``MixtureSVI`` for a block with the two coupled tables ``mu`` and ``tau``.  The subclass
    supplies ``match``, ``describe`` and ``_count``: (the count the updates read, whether it is
    per element)."""

    ANNEALING = False       # the natural-gradient step has no annealed form
    KIND = 'dgmm_svi'
    _BITS = (('mu', 1), ('tau', 2), ('alpha', 4))

    def _globals(self):
        return [self.mu, self.tau, self.alpha]

    def _step_setup(self):
        self.ws_step = self.rt.empty(self.kernels.natural_step_workspace(self.D, self.K))
        init = self.mu._init
        if init is not None and init[0] == 'value':
            # a point mass has no parameters; it steps from those of its prior (expfamily.py:193-212
            # leaves phi alone), so they stand in the table from the start and NaN never does
            self.mu_par.copy_(self.rt.torch.stack([self.m0.reshape(-1), self.beta0.reshape(-1)], -1))

    def _bit(self, node):
        for key, bit in self._BITS:
            if node is self.roles[key]:
                return bit
        return 0

    def _step(self, nodes, bits, scale):
        self._settle()
        m = self._multiplier()
        for node in nodes:
            self._annealing(node)
            _delta.updated(self._delta, self.roles, node)
        self.rt.sync_stream()
        cnt, per_element = self._count()
        self.kernels.natural_step(self.D, self.K, bits, self.m0, self.beta0, self.a0, self.b0,
                                  self.S1, self.S2, cnt, per_element, self.mu_par, self.mu_mom,
                                  self.tau_par, self.tau_mom, self.prior_r, self.Nk, self.alpha_r,
                                  self.elog_r, m, scale, self.ws_step, self.scal[3:6])
        for key, bit in self._BITS[:2]:
            if bits & bit:
                self._ab_fresh[key] = False
        self._version += 1

    def _unseen_terms(self):
        """What the elements of the columns with nothing observed in the present batch hold of the
        bound terms of ``mu`` and ``tau``.  Such an element keeps the posterior of earlier batches
        and moves like every other, but the reference leaves it out of both terms
        (expfamily.py:433-480).  A few rows, once per bound, on the host."""
        rows = self._unseen_rows()
        if not rows.size:
            return dict(mu=0.0, tau=0.0)
        from scipy.special import digamma, gammaln
        host = lambda a: a.cpu().numpy().reshape(-1)[rows]              # noqa: E731
        pair = lambda a: a.cpu().numpy().reshape(-1, 2)[rows].T         # noqa: E731
        m0, beta0, a0, b0 = (host(a) for a in (self.m0, self.beta0, self.a0, self.b0))
        m, lam = pair(self.mu_par)
        a, b = pair(self.tau_par)
        tau, log_tau = pair(self.tau_mom)
        mu = 0.5 * (np.log(beta0) - np.log(lam)) - 0.5 * beta0 * ((m - m0) ** 2 + 1 / lam) + 0.5
        ta = (a0 * np.log(b0) - gammaln(a0) - b0 * tau + a0 * log_tau) \
            - (a * (digamma(a) - 1.0) - gammaln(a))
        return dict(mu=float(np.sum(mu)), tau=float(np.sum(ta)))


class DiagGaussianMixtureSVIPlan(DiagGaussianSVI, DiagGaussianMixturePlan):
    """The block of dgmm.py under stochastic variational inference.  Opt-in:
    ``VB(..., engine='fused+batches+gaussian')``, tried right after ``DiagGaussianMixturePlan``."""

    @staticmethod
    def describe():
        return ('the model of the fused diagonal-Gaussian-mixture block with '
                'plates_multiplier=(m, 1) on Z (mini-batches: one positive factor on the row axis '
                'of Z and Y, none on mu, tau or alpha; D <= %d, K <= %d)' % dgmm_limits()[::-1])

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _SPEC, batches=True)

    def _count(self):
        return self.Nk, 0

    def _hand_over(self):
        if MaskedDiagGaussianMixtureSVIPlan.match(self.nodes()) is not None:
            # Y was observed with a mask of its full shape: the form for missing observations
            MaskedDiagGaussianMixtureSVIPlan(self.roles, runtime=self._rt)
        else:
            super()._hand_over()


class MaskedDiagGaussianMixtureSVIPlan(DiagGaussianSVI, MaskedDiagGaussianMixturePlan):
    """The block of dgmm_masked.py under stochastic variational inference: every batch comes with a
    mask of its full shape.  Opt-in: ``VB(..., engine='fused+batches+gaussian')``, tried right after
    ``MaskedDiagGaussianMixturePlan``."""

    @staticmethod
    def describe():
        return ('the model of the fused diagonal-Gaussian-mixture block with a mask of the full '
                'shape (N, D) and plates_multiplier=(m, 1) on Z (mini-batches: one positive factor '
                'on the row axis of Z and Y, none on mu, tau or alpha; D <= %d, K <= %d)'
                % dgmm_masked_limits()[::-1])

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _MASKED_SPEC, batches=True)

    def _count(self):
        return self.M, 1
