"""
Execution plan of the binomial-mixture block (successes out of trials)

    R = Dirichlet(const);  Z = Categorical(R, plates=(N, 1))
    P = Beta(const, plates=(D, K));  X = Mixture(Z, Binomial, n, P);  X.observe(x[, mask=m])

with constant priors, ``n`` a constant of non-negative integers that broadcasts to (N, D, 1) (a
scalar, (D, 1), (N, 1, 1) or (N, D, 1)) of at most 65534, K <= 64 and D <= 1024; ``X`` fully
observed or observed with a mask of the full shape (N, D).  Opt-in: ``VB(..., engine='fused')``;
the default engine runs this model on the generic engine.  The plan owns, in HBM: the counts and the
trials as one uint16 per entry each (trials 0xFFFF = hidden), the parameters (alpha, beta) and the
moments (<log p>, <log(1-p)>) of ``P`` as (D K, 2) tables, those of ``R`` (K), the tables
l1 = <log p> - <log(1-p)>, l0 = <log(1-p)> and c that the last ``Z`` update used, and the statistics
S[d, k] = sum_n r_nk x_nd, T[d, k] = sum_n r_nk n_nd, N_k and counts = (S, T - S), the message to
``P``.  Nothing of size (N, K) or (N, D, K) exists: the responsibilities of ``Z`` are formed inside
``vmp_binm_pass`` and only on request written out (``Z.get_moments()``).

Two forms of the pass (csrc/vmp_binm_dev.h): two planes whenever the trials vary along the rows or
anything is hidden; one plane -- the Poisson block's pass on the counts alone, sum_d n_d l0[d, k]
inside c and T = n_d N_k -- when the pack found the trials constant along the rows and nothing hidden.
So a mask of ones gives the bits of the unmasked run.

All plate terms of the lower bound follow from the statistics, sum_n lse_n and the tables:
    <log p(X)>           = counts . (<log p>, <log(1-p)>) + sum_observed log C(n, x)   (the last sum
                           comes from the pack)
    <log p(Z)> + entropy = sum_k N_k <log pi_k> + sum_n lse_n - N_k . c_used - scal[2]
The tables are written by a ``Z`` update only, so ``Z.get_moments()`` after a later ``P`` update is
still that update's posterior.

Masks: ``X.observe(x, mask=m)`` with ``m`` a boolean host array or a ``DeviceMask`` of shape exactly
(N, D).  A hidden position is never interpreted: NaN, -1 or 1e300 may stand there.  A row with
nothing observed has ``Z.mask`` False: its moment is softmax(c) of the tables the last update used
and it enters neither N_k nor the bound term of ``Z``.  A column with nothing observed leaves its
``P`` at the prior, with a bound term of exactly zero.  A scalar mask or one that broadcasts over a
plate is declined (generic engine).

Checkpoints: the block writes its own ``plans/<i>/`` group (kind 'binm'); a checkpoint whose mask
differs is refused.
"""
import ctypes

import numpy as np

from . import _delta
from ._dirichlet import DirichletKernels, prior_table
from ._mixture_svi import MixtureSVI
from ._mixture import (MixtureSpec, PlateMixturePlan, _p, _takes_mask, full_mask_reason,
                       match_plate_mixture, observed_tensor, plates_of_p_reason)

from ... import _lib
from ...nodes.beta import Beta
from ...nodes.binomial import Binomial
from ...nodes.categorical_markov_chain import CategoricalMarkovChainToCategorical

_DTYPES = {'float64': 0, 'int64': 1, 'uint8': 2, 'int32': 3}
_LIMITS = []


def binm_limits():
    """(max K, max D, most trials) of the built pass: host-only ``vmp_binm_limits``."""
    if not _LIMITS:
        v = [ctypes.c_int32() for _ in range(3)]
        _lib.raise_for_status(_lib.load().vmp_binm_limits(*[ctypes.byref(a) for a in v]))
        _LIMITS.append(tuple(a.value for a in v))
    return _LIMITS[0]


def _limits_text():
    return 'K <= %d, D <= %d and at most %d trials' % binm_limits()


class BINMKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def plan(self, N, D, K):
        """(rows of a chunk, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_binm_plan(N, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused binomial-mixture block supports ' + _limits_text())
        return c.value, w.value

    def pack(self, N, D, dtype, x, trials, ts_n, ts_d, mask, xp, np_, flags, counts, lcoef, ws):
        self.rt.check(self.lib.vmp_binm_pack(self.ctx, N, D, dtype, _p(x), _p(trials), ts_n, ts_d,
                                             _p(mask), _p(xp), _p(np_), _p(flags), _p(counts),
                                             _p(lcoef), _p(ws)))

    def tables(self, D, K, form, elog_p, elog_pi, ncol, l1, l0, c, cfold=None):
        self.rt.check(self.lib.vmp_binm_tables(self.ctx, D, K, form, _p(elog_p), _p(elog_pi),
                                               _p(ncol), _p(l1), _p(l0), _p(c), _p(cfold)))

    def pass_(self, N, D, K, one_plane, xp, np_, ncol, labels, l1, l0, c, ws, S, T, Nk, counts,
              scal, r_out=None):
        self.rt.check(self.lib.vmp_binm_pass(self.ctx, N, D, K, one_plane, _p(xp), _p(np_),
                                             _p(ncol), _p(labels), _p(l1), _p(l0), _p(c), _p(ws),
                                             _p(S), _p(T), _p(Nk), _p(counts), _p(scal),
                                             _p(r_out)))


def trials_plane(X):
    """The trials of ``X`` without the cluster axis as a C-contiguous int64 array of shape (1 or N,
    1 or D) and its element strides (along N, along D), zero along an axis it does not vary over."""
    N, D = X.plates
    t = np.asarray(X._proto.trials, dtype=np.int64)
    if t.ndim > 3:
        raise ValueError('trials of shape %s do not broadcast to (N, D, 1)' % (t.shape,))
    t = t.reshape((1,) * (3 - t.ndim) + t.shape)[..., 0]
    if t.shape[0] not in (1, N) or t.shape[1] not in (1, D):
        raise ValueError('trials of shape %s do not broadcast to (N, D, 1)' % (t.shape,))
    t = np.ascontiguousarray(t)
    return t, (t.shape[1] if t.shape[0] > 1 else 0), (1 if t.shape[1] > 1 else 0)


def _limits_reason(r):
    X = r['X']
    D, K = X.plates[1], X.clusters
    max_k, max_d, max_trials = binm_limits()
    if K > max_k or D > max_d:
        return 'D = %d, K = %d exceed the limits of the block (%s)' % (D, K, _limits_text())
    t = np.asarray(X._proto.trials)
    if t.size and t.max() > max_trials:
        return '%d trials exceed the limits of the block (%s)' % (t.max(), _limits_text())


_SPEC = MixtureSpec(
    label='fused binomial-mixture block',
    # Bernoulli has a block of its own; a hidden Markov model: no block of this family
    takes=lambda X: X.node_class is Binomial
    and not isinstance(X.parents[0], CategoricalMarkovChainToCategorical),
    observed='X', weights='R', params=(('P', Beta, None),),
    parents='its parents are not (Categorical(Dirichlet), Beta)',
    constant='the parameter of %s is a node (%s), not a constant',
    role_plates='plates of Z / P / R are {} / {} / {}, not (N, 1) / (D, K) / ()',
    mask=full_mask_reason, plates=plates_of_p_reason, limits=_limits_reason)


class BinomialMixturePlan(PlateMixturePlan):

    KERNELS = BINMKernels
    LABEL, KIND = _SPEC.label, 'binm'
    TERMS = ('X', 'Z', 'P', 'R')
    _FLAGS = ('_used',)

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates=(N, 1)), Binomial, n, Beta(const, "
                "plates=(D, K))) with constant trials n that broadcast to (N, D, 1), fully observed "
                "or observed with a mask of the full shape (N, D), %s; a scalar mask or one that "
                "broadcasts over a plate is declined" % _limits_text())

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _SPEC)

    def __init__(self, roles, runtime=None, kernels=None):
        super().__init__(roles, runtime=runtime, kernels=kernels)
        self.one_plane = 0          # the form of the pass: 1 when the pack allows the one-plane form

    def _repacks(self, node):
        """With any mask of the full shape or none."""
        return _takes_mask(node)

    # -- set-up ------------------------------------------------------------------------------------
    def _pack(self):
        """``X._data`` and the trials as 16 bits per entry each; an observed count that fails a
        check is the reference's ValueError (binomial.py)."""
        rt, torch = self.rt, self.rt.torch
        N, D = self.N, self.D
        t, dtype = observed_tensor(rt, self.X, N, D, _DTYPES)
        tr, ts_n, ts_d = trials_plane(self.X)
        self.trials = torch.from_numpy(tr).to(rt.device)
        self.ncol = self._up(np.broadcast_to(tr[0] if len(tr) else 0, (D,)))
        self.xp = torch.zeros(max(N * D, 4), dtype=torch.int16, device=rt.device)
        self.np_ = torch.zeros(max(N * D, 4), dtype=torch.int16, device=rt.device)
        flags = torch.zeros(4, dtype=torch.int32, device=rt.device)
        counts = torch.zeros(3, dtype=torch.int64, device=rt.device)
        self.kernels.pack(N, D, dtype, t, self.trials, ts_n, ts_d, self.maskd, self.xp, self.np_,
                          flags, counts, self.lcoef, self.ws)
        f = flags.cpu().numpy()
        if f[1]:
            raise ValueError("Counts must be integer")
        if f[0] or f[2]:
            raise ValueError("Invalid count")
        if f[3]:
            raise NotImplementedError('fused binomial-mixture block: an entry has more than %d '
                                      'trials (%s); the generic engine takes such data'
                                      % (binm_limits()[2], _limits_text()))
        n = counts.cpu().numpy()
        self.n_observed, self.n_hidden = int(n[0]), int(n[1])
        self.trials_constant = bool(n[2])
        self._stale = False

    def _form(self):
        return 1 if self.trials_constant and self.n_hidden == 0 else 0

    def _adopt_form(self):
        self.one_plane = self._form()

    def _set_form(self):
        """The form of the pass for the packed data; when it changes, the tables of the last ``Z``
        update are formed again for the new one."""
        form = self.one_plane
        self._adopt_form()
        if form != self.one_plane:
            self._tables(self.elog_p_used if self._used else None, self.elog_r_used)

    def _materialize(self):
        if self._ready:
            if self._stale:
                self._restate()
            return
        self._delta = _delta.delta_roles(self.roles)
        rt, k = self.rt, self.kernels
        N, D, K = self.N, self.D, self.K
        rt.sync_stream()
        self._upload_mask()
        self.chunk, wsd = k.plan(N, D, K)
        self.ws = rt.empty(int(wsd))
        self.lcoef = rt.zeros(1)
        self._pack()
        self.one_plane = self._form()
        pp = prior_table(self.P, (D, K, 2)).reshape(D * K, 2)
        pr = prior_table(self.R, (K,))
        self.prior_p, self.prior_r = self._up(pp), self._up(pr)
        self.alpha_p, self.elog_p = rt.empty(D * K, 2), rt.empty(D * K, 2)
        self.elog_p_used, self.elog_r_used = rt.zeros(D * K, 2), rt.zeros(K)
        self._used = False          # whether the tables in use hold an observation term
        self.alpha_r, self.elog_r = rt.empty(K), rt.empty(K)
        self.l1, self.l0 = rt.zeros(D, K), rt.zeros(D, K)
        self.c, self.cfold = rt.zeros(K), rt.zeros(K)
        self.S, self.T, self.Nk = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
        self.counts = rt.zeros(D * K, 2)
        self.ws_small = rt.empty(max(D * K, 1024))
        # [0] sum lse, [1] N_k . c used, [2] S . l1 (+ T . l0) used, [3] bound of P, [4] of R,
        # [5] counts . <log p>, [6] N_k . <log pi>
        self.scal = rt.zeros(8)
        self._init_p(pp)
        self._weights_step(4, self._weights_init_counts(pr))
        self._labels_from_init()
        self.elog_r_used.copy_(self.elog_r)
        self._tables(None, self.elog_r_used)
        self._ready = True
        self._run_pass()

    def _init_p(self, prior):
        """Initial parameters and <log> table of ``P``: the prior, given parameters (device), or
        the logs of a value / of a draw from the prior (host, set-up)."""
        D, K = self.D, self.K
        init = self.P._init
        counts = None
        if init is not None and init[0] == 'parameters':
            a = np.asarray(init[1][0], dtype=np.float64)
            if np.any(a <= 0):
                raise ValueError("Natural parameters should be positive")
            counts = self._up(np.broadcast_to(a, (D, K, 2)).reshape(D * K, 2) - prior)
        self.kernels.dirichlet(D * K, 2, 2, 1, self.prior_p, counts, self.alpha_p, self.elog_p,
                               self.ws_small, self.scal[3:4])
        if init is None or init[0] == 'parameters':
            return
        if init[0] == 'value':
            p = np.broadcast_to(np.asarray(init[1], dtype=np.float64), (D, K))
        else:
            p = np.random.beta(prior[:, 0], prior[:, 1]).reshape(D, K)
        with np.errstate(divide='ignore'):
            e = np.stack([np.log(p), np.log(1 - p)], -1)
        self.elog_p.copy_(self._up(e.reshape(D * K, 2)))
        self.alpha_p.fill_(float('nan'))                # a point mass has no parameters

    def _tables(self, elog_p, elog_r):
        """The centred tables of the pass from the given moments (None: no observation term);
        ``cfold`` only in the one-plane form."""
        self.kernels.tables(self.D, self.K, 1, elog_p, elog_r,
                            self.ncol if self.one_plane else None, self.l1, self.l0, self.c,
                            self.cfold if self.one_plane else None)

    def _run_pass(self, r_out=None):
        """The statistics of the present ``Z`` state (tables or labels)."""
        self.kernels.pass_(self.N, self.D, self.K, self.one_plane, self.xp, self.np_, self.ncol,
                           self.labels, self.l1, self.l0,
                           self.cfold if self.one_plane else self.c, self.ws, self.S, self.T,
                           self.Nk, self.counts, self.scal, r_out)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        self.rt.sync_stream()
        D, K = self.D, self.K
        if node is self.Z:
            self.labels = None
            self.elog_p_used.copy_(self.elog_p)
            self.elog_r_used.copy_(self.elog_r)
            self._used = True
            self._tables(self.elog_p_used, self.elog_r_used)
            self._run_pass()
        elif node is self.P:
            self.kernels.dirichlet(D * K, 2, 2, 1, self.prior_p, self.counts, self.alpha_p,
                                   self.elog_p, self.ws_small, self.scal[3:4])
        elif node is self.R:
            self._weights_step(4, self.Nk)
        else:
            return
        self._version += 1

    def _bound_terms(self):
        k = self.kernels
        k.dot(2 * self.D * self.K, self.counts, self.elog_p, self.ws_small, self.scal[5:6])
        k.dot(self.K, self.Nk, self.elog_r, self.ws_small, self.scal[6:7])
        s, entropy = self._host_scal()
        lcoef = float(self.lcoef.cpu().numpy()[0])
        return dict(X=float(s[5]) + lcoef, Z=float(s[6]) + entropy, P=float(s[3]), R=float(s[4]))

    def get_moments(self, node):
        self._materialize()
        D, K = self.D, self.K
        if node is self.R:
            return [self.elog_r.cpu().numpy().reshape(self.R.plates + (K,)).copy()]
        if node is self.P:
            return [self.elog_p.cpu().numpy().reshape(D, K, 2).copy()]
        if node is self.Z:
            return [self.responsibilities().cpu().numpy().reshape(self.N, 1, K)]
        if node is self.X:
            xp = self.xp.cpu().numpy()[:self.N * D].view(np.uint16).reshape(self.N, D)
            return [xp.astype(np.float64)]
        raise NotImplementedError

    # -- persistence -----------------------------------------------------------------------------------
    _SAVED = ('alpha_p', 'elog_p', 'elog_p_used', 'alpha_r', 'elog_r', 'elog_r_used', 'l1', 'l0',
              'c', 'cfold', 'S', 'T', 'Nk', 'counts', 'scal')


class BinomialMixtureSVIPlan(MixtureSVI, BinomialMixturePlan):
    """The block under stochastic variational inference (_mixture_svi.py): ``Z`` and ``X`` hold a
    mini-batch that stands for ``m`` times as many rows (``plates_multiplier``), every step
    re-observes ``X`` -- the device state stays -- and updates ``Z`` (one pack, one pass), and
    ``gradient_step`` moves P and R along their natural gradients in one launch.  Opt-in:
    ``VB(..., engine='fused+batches')`` (everything of ``engine='fused'`` plus these forms),
    tried after ``BinomialMixturePlan``."""

    KIND, PARAM = 'binm_svi', 'P'

    @staticmethod
    def describe():
        return ('the model of the fused binomial-mixture block with plates_multiplier=(m, 1) on Z (mini-batches: one '
                'positive factor on the row axis of Z and X, none on P or R)')

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _SPEC, batches=True)

    def _step_table(self):
        DK = self.D * self.K
        return dict(kind=0, rows=DK, cols=2, rs=2, cs=1, prior=self.prior_p, prior_b=None,
                    stat=self.counts, cnt=None, per_element=0, par=self.alpha_p, mom=self.elog_p)
