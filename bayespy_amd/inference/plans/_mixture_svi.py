"""
Stochastic variational inference on the count-mixture blocks (bmm.py, binm.py, cmm.py, mmm.py,
pmm.py): the recipe of bayespy/demos/stochastic_inference.py

    Z = Categorical(R, plates=(N, 1), plates_multiplier=(m, 1));  X = Mixture(Z, family, P)
    per step:  X.observe(next batch);  Q.update(Z);  Q.gradient_step(P, R, scale=s)

``Z`` and ``X`` hold a mini-batch of N rows that stands for m times as many.  ``MixtureSVI`` is the
mixin that turns a block into its form under mini-batches (a subclass in the block's file, as
``GMMSVIPlan`` is of ``GMMPlan``); the block supplies ``_step_table``, which says where its
parameter table lies.

A step.  ``X.observe`` keeps the device state and marks the data stale.  The next operation packs
the new batch but runs no pass: the pass with the old tables would be thrown away by the
``update(Z)`` that follows, which forms the tables and runs the pass once.  Whatever reads the
statistics or the moments of ``Z`` before that (a step of a global node, the bound, ``Z.get_moments``,
a checkpoint) runs the pass that is due first; the moments of the global nodes do not depend on the
batch and run nothing.  ``gradient_step`` moves the parameter node and the weights in one launch
(``vmp_mix_natural_step``):

    phi <- phi + scale (phi* - phi),    phi* = prior + m * statistic of the batch

every optimum from the statistics present before either node moves (vmp.py:432-440);
``update(P | R)`` is that step with scale = 1.  A parameter node that is still a point mass steps
from the parameters of its prior, as on the generic engine.  The bound terms of ``X`` and ``Z`` are
multiplied by m (expfamily.py:470-480) and the total is formed again from the terms.

Opt-in: ``VB(..., engine='fused+batches')``, which is ``engine='fused'`` plus the forms of
``plans.OPT_IN_BATCHES``; plain ``engine='fused'`` keeps raising for such a model with the blocks'
reasons.  Declined with a reason: a multiplier on a global node, different or non-positive factors on ``Z``
and ``X``, a factor on another axis, sharded plates.  Both diagonal-Gaussian blocks have such a
form too, with a step kernel of their own for their two coupled tables (dgmm_svi.py,
``engine='fused+batches+gaussian'``).
"""
import numpy as np

from . import _delta
from ._mixture import batch_multiplier, batch_reason


class MixtureSVI:
    """Mixin in front of a ``PlateMixturePlan``.  The subclass names ``PARAM`` (the role of the
    parameter node) and ``KIND``, and supplies ``match`` (the block's matcher with
    ``batches=True``), ``describe`` and ``_step_table``: a dict of the arguments ``kind``, ``rows``,
    ``cols``, ``rs``, ``cs``, ``prior``, ``prior_b``, ``stat``, ``cnt``, ``per_element``, ``par``
    and ``mom`` of ``natural_step``."""

    PARAM = 'P'

    def __init__(self, roles, runtime=None, kernels=None):
        super().__init__(roles, runtime=runtime, kernels=kernels)
        self._pass_due = False      # new data are packed, their pass waits for whoever needs it
        self._m_seen = batch_multiplier(self.Z)
        self._z_init_seen = None
        self._unseen = None         # rows of the parameter table without an observed entry

    # -- state ---------------------------------------------------------------------------------------
    def _globals(self):
        return [self.roles[self.PARAM], self.roles[self.WEIGHTS]]

    def _multiplier(self):
        """The factor of the mini-batch plate as the nodes carry it now (it has a setter)."""
        bad = batch_reason(self.roles[self.OBSERVED], self.Z, self._globals())
        if bad:
            raise ValueError('%s (stochastic VI): %s' % (self.LABEL, bad))
        return batch_multiplier(self.Z)

    def invalidate(self, node):
        X = self.roles[self.OBSERVED]
        if self._ready and node is self.Z and self.Z._init is self._z_init_seen \
                and X.observed and self._repacks(X) and type(self).match(self.nodes()) is not None:
            # the setter of plates_multiplier: the state stays, the next operation reads the factor
            self._m_seen = batch_multiplier(self.Z)
            self._version += 1
            return
        super().invalidate(node)

    def _materialize(self):
        fresh = not self._ready
        super()._materialize()
        if not fresh:
            return
        self._m_seen = batch_multiplier(self.Z)
        self._z_init_seen = self.Z._init
        self._pass_due = False
        self._step_setup()

    def _step_setup(self):
        """Once, after the set-up of the block: the workspace of the step, and the parameters a
        point mass steps from."""
        t = self._step_table()
        self.ws_step = self.rt.empty(self.kernels.natural_step_workspace(t['kind'], t['rows'],
                                                                         t['cols'], self.K))
        init = self.roles[self.PARAM]._init
        if init is not None and init[0] in ('value', 'random'):
            # a point mass has no parameters; it steps from those of its prior (expfamily.py:193-212
            # leaves phi alone), so they stand in the table from the start and NaN never does
            if t['kind'] == 0:
                t['par'].copy_(t['prior'])
            else:
                t['par'].copy_(self.rt.torch.stack([t['prior'].reshape(-1),
                                                    t['prior_b'].reshape(-1)], -1))

    def _restate(self):
        self._repack()
        self._pass_due = True
        self._unseen = None

    def _unseen_rows(self):
        """The rows d K + k of the parameter table whose column d of ``X`` has nothing observed in
        the present batch (host, found once per batch), or an empty array."""
        if self._unseen is None:
            m = self._host_mask() if self.roles[self.OBSERVED]._mask is not True else None
            cols = np.zeros(0, dtype=np.int64) if m is None else np.flatnonzero(~m.any(axis=0))
            self._unseen = (cols[:, None] * self.K + np.arange(self.K)).reshape(-1)
        return self._unseen

    def _unseen_term(self):
        """What the rows of ``_unseen_rows`` hold of the bound term of the parameter node.  Under
        mini-batches such a row keeps the posterior of earlier batches and moves like every other,
        but the mask of the node is False there and the reference leaves the row out of the term
        (expfamily.py:433-480).  A few rows, once per bound, on the host."""
        rows = self._unseen_rows()
        if not rows.size:
            return 0.0
        from scipy.special import digamma, gammaln
        t = self._step_table()
        host = lambda a: a.cpu().numpy().reshape(-1)        # noqa: E731
        if t['kind'] == 1:
            a0, b0 = host(t['prior'])[rows], host(t['prior_b'])[rows]
            a, b = host(t['par']).reshape(-1, 2)[rows].T
            return float(np.sum((a0 * np.log(b0) - gammaln(a0)) - (a * np.log(b) - gammaln(a))
                                + (b - b0) * a / b + (a0 - a) * (digamma(a) - np.log(b))))
        at = (rows[:, None] * t['rs'] + np.arange(t['cols']) * t['cs'])
        p, a = host(t['prior'])[at], host(t['par'])[at]

        def g(v):
            return gammaln(v.sum(-1)) - gammaln(v).sum(-1)
        elog = digamma(a) - digamma(a.sum(-1, keepdims=True))
        return float(np.sum((p - a) * elog) + np.sum(g(p) - g(a)))

    def _unseen_terms(self):
        """``_unseen_term`` per role whose bound term leaves the rows of ``_unseen_rows`` out."""
        return {self.PARAM: self._unseen_term()}

    def _run_pass(self, r_out=None):
        self._pass_due = False
        super()._run_pass(r_out)

    def _settle(self):
        """Ahead of whatever reads the statistics of the batch: the pass a re-observation put
        off, with the tables of the last ``Z`` update."""
        self._materialize()
        if self._pass_due:
            self._set_form()
            self._run_pass()

    # -- operations ----------------------------------------------------------------------------------
    def _bit(self, node):
        if node is self.roles[self.PARAM]:
            return 1
        if node is self.roles[self.WEIGHTS]:
            return 2
        return 0

    def _step(self, nodes, bits, scale):
        self._settle()
        m = self._multiplier()
        for node in nodes:
            _delta.updated(self._delta, self.roles, node)
        self.rt.sync_stream()
        t = self._step_table()
        self.kernels.natural_step(t['kind'], bits, t['rows'], t['cols'], t['rs'], t['cs'],
                                  t['prior'], t['prior_b'], t['stat'], t['cnt'], t['per_element'],
                                  t['par'], t['mom'], self.K, self.prior_r, self.Nk, self.alpha_r,
                                  self.elog_r, m, scale, self.ws_step, self.scal[3:5])
        self._version += 1

    def update(self, node):
        if node is self.Z:
            self._materialize()
            if self._pass_due:
                self._adopt_form()      # the tables and the pass of this update are the only ones
            return super().update(node)
        bit = self._bit(node)
        if not bit:
            return super().update(node)
        self._step([node], bit, 1.0)

    def gradient_step(self, nodes, scale=1.0):
        """phi <- phi + scale * (phi* - phi) for the parameter node and the weights among
        ``nodes``, in one launch."""
        from ...nodes.node import Stochastic
        bits, todo = 0, []
        for node in nodes:
            if not isinstance(node, Stochastic) or node.observed:
                continue
            if node is self.Z:
                raise NotImplementedError(
                    'gradient step of %s: the %s keeps no natural parameters of the '
                    'responsibilities to step from; update it (Q.update(%r)), or use '
                    'VB(..., engine="generic")' % (node.name, self.LABEL, node.name))
            if self._bit(node):
                bits |= self._bit(node)
                todo.append(node)
        if bits:
            self._step(todo, bits, scale)

    def responsibilities(self):
        self._materialize()
        if self._pass_due:
            self._set_form()            # the pass in its write mode is the one that was due
        return super().responsibilities()

    def _lower_bound_terms(self):
        self._settle()
        if self._L_version != self._version:
            super()._lower_bound_terms()
            # the mini-batch stands for m times as many rows (expfamily.py:470-480); the total is
            # formed again from the terms
            m = self._multiplier()
            t = self._L
            for key in (self.OBSERVED, 'Z'):
                t[key] = m * t[key]
            for key, left_out in self._unseen_terms().items():
                t[key] = t[key] - left_out
            total = t[self.TERMS[0]]
            for key in self.TERMS[1:]:
                total = total + t[key]
            t['total'] = total
        return _delta.bound_terms(self._L, self._delta)

    # -- persistence -----------------------------------------------------------------------------------
    def save_state(self, put, nodes, index):
        self._settle()
        super().save_state(put, nodes, index)

    def load_state(self, reader, nodes, index):
        self._settle()
        super().load_state(reader, nodes, index)
