"""
Execution plan of the multinomial-mixture block (mixture of unigrams, count-vector clustering)

    R = Dirichlet(const);  Z = Categorical(R, plates=(N,))
    P = Dirichlet(const, plates=(K,)) over M words;  X = Mixture(Z, Multinomial, n, P);  X.observe(x)

with constant concentrations, ``n`` a constant number of trials (a scalar, or one per row given as
(N, 1) beside the cluster axis), x (N, M) counts of at most 65534 whose rows add up to ``n``,
K <= 64 and M <= 1024; ``X`` fully observed.  Opt-in: ``VB(..., engine='fused')``; the default
engine runs this model on the generic engine as before.  The plan owns, in HBM: ``x`` as one uint16
per entry, the Dirichlet parameters and <log p> of ``P`` as (K, M) tables -- K Dirichlet rows that
one strided ``vmp_lda_dirichlet`` call updates --, those of ``R`` (K), the (M, K) word-major table
L = <log p_k> - <log p_0> and c = <log pi> less its maximum that the last ``Z`` update used, and
the statistics S[k, m] = sum_n r_nk x_nm and N_k.  Nothing of size (N, K) or (N, K, M) exists: the
responsibilities of ``Z`` are formed inside ``vmp_mmm_pass`` and only on request written out
(``Z.get_moments()``).

All plate terms of the lower bound follow from the statistics, sum_n lse_n and the tables:
    <log p(X)>           = S . <log p> + sum_n [lgamma(n_n + 1) - sum_m lgamma(x_nm + 1)]
                           (the present table; the last sum comes from the pack)
    <log p(Z)> + entropy = sum_k N_k <log pi_k> + sum_n lse_n - N_k . c_used - S . L_used
``L`` and ``c`` are written by a ``Z`` update only, so ``Z.get_moments()`` after a later ``P``
update is still that update's posterior.

Checkpoints: the block writes its own ``plans/<i>/`` group (kind 'mmm').
"""
import ctypes

import numpy as np

from . import _delta
from ._dirichlet import DirichletKernels, prior_table
from ._mixture_svi import MixtureSVI
from ._mixture import (PlateMixturePlan, _mask_shape, _p, batch_reason, cluster_plate_reason,
                       observed_tensor)
from .pmm import _largest_host_count

from ... import _lib
from ...nodes.node import Constant
from ...nodes.dirichlet import Dirichlet
from ...nodes.categorical import Categorical
from ...nodes.categorical_markov_chain import CategoricalMarkovChainToCategorical
from ...nodes.mixture import Mixture
from ...nodes.multinomial import Multinomial

_DTYPES = {'float64': 0, 'int64': 1, 'uint8': 2, 'int32': 3}
_LIMITS = []
LABEL = 'fused multinomial-mixture block'


def mmm_limits():
    """(max K, max M, largest count) of the built pass: host-only ``vmp_mmm_limits``."""
    if not _LIMITS:
        v = [ctypes.c_int32() for _ in range(3)]
        _lib.raise_for_status(_lib.load().vmp_mmm_limits(*[ctypes.byref(a) for a in v]))
        _LIMITS.append(tuple(a.value for a in v))
    return _LIMITS[0]


def _limits_text():
    return 'K <= %d, M <= %d and counts of at most %d' % mmm_limits()


class MMMKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def plan(self, N, M, K):
        """(rows of a chunk, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_mmm_plan(N, M, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the %s supports %s' % (LABEL, _limits_text()))
        return c.value, w.value

    def pack(self, N, M, dtype, x, trials, xp, flags, lcoef, ws):
        self.rt.check(self.lib.vmp_mmm_pack(self.ctx, N, M, dtype, _p(x), _p(trials), _p(xp),
                                            _p(flags), _p(lcoef), _p(ws)))

    def tables(self, M, K, elog_p, elog_pi, L, c):
        self.rt.check(self.lib.vmp_mmm_tables(self.ctx, M, K, _p(elog_p), _p(elog_pi), _p(L),
                                              _p(c)))

    def pass_(self, N, M, K, xp, labels, L, c, ws, S, Nk, scal, r_out=None):
        self.rt.check(self.lib.vmp_mmm_pass(self.ctx, N, M, K, _p(xp), _p(labels), _p(L), _p(c),
                                            _p(ws), _p(S), _p(Nk), _p(scal), _p(r_out)))


def row_trials(X):
    """The number of trials of every row of the Mixture of Multinomial ``X`` as (N,) int64, or None
    where ``n`` varies over the clusters or does not broadcast to the rows.  ``n`` stands beside the
    cluster axis of ``P``: a scalar, (1,) or (N, 1)."""
    t = np.asarray(X._proto.trials)
    if t.ndim >= 1:
        if t.shape[-1] != 1:
            return None
        t = t[..., 0]
    try:
        return np.array(np.broadcast_to(t, X.plates), dtype=np.int64)
    except ValueError:
        return None


def match_multinomial_mixture(nodes, why=None, batches=False):
    """The roles of the first Mixture of Multinomial among ``nodes`` that the block takes, or None;
    the reason of every one it looks at and declines goes to ``why`` (a list, or None).
    ``batches``: the form under stochastic VI, as in ``match_plate_mixture``."""
    label = LABEL + (' (stochastic VI)' if batches else '')
    for X in nodes:
        if not isinstance(X, Mixture) or X.node_class is not Multinomial \
                or isinstance(X.parents[0], CategoricalMarkovChainToCategorical):
            continue

        def no(msg, X=X):
            if why is not None:
                why.append('%s, observed node %s: %s' % (label, X.name or '<unnamed>', msg))
        if len(X.parents) != 2 or type(X.parents[0]) is not Categorical \
                or type(X.parents[0].parents[0]) is not Dirichlet \
                or type(X.parents[1]) is not Dirichlet:
            no('its parents are not (Categorical(Dirichlet), Dirichlet)')
            continue
        Z, P = X.parents
        R = Z.parents[0]
        below = (Z, P, R)
        if not all(any(n is m for m in nodes) for n in (X,) + below):
            continue
        if batches:
            msg = batch_reason(X, Z, (P, R))
            if msg is not None:
                no(msg)
                continue
        elif any(any(m != 1 for m in n.plates_multiplier) for n in (X,) + below):
            no('plates_multiplier (mini-batches) goes through the generic engine')
            continue
        if any(getattr(n, '_shard_axis', None) is not None for n in (X,) + below):
            no('a plate is sharded over ranks')
            continue
        if X._mask is not True:
            no('it has a mask of shape %s: the block takes fully observed count vectors only; a '
               'masked model goes through the generic engine' % (_mask_shape(X._mask),))
            continue
        bad = [(n, p) for n in (P, R) for p in n.parents if not isinstance(p, Constant)]
        if bad:
            no('the concentration of %s is a node (%s), not a constant'
               % (bad[0][0].name, type(bad[0][1]).__name__))
            continue
        msg = cluster_plate_reason(X)
        if msg is not None:
            no(msg)
            continue
        K = X.clusters
        if len(X.plates) != 1 or Z.plates != X.plates or P.plates != (K,) \
                or any(p != 1 for p in R.plates):
            no('plates of X / Z / P / R are %s / %s / %s / %s, not (N,) / (N,) / (K,) / ()'
               % (X.plates, Z.plates, P.plates, R.plates))
            continue
        if row_trials(X) is None:
            no('the number of trials n has shape %s: the block needs a constant integer array '
               'that broadcasts to the rows (N,), the same for every cluster'
               % (np.shape(X._proto.trials),))
            continue
        M = P.dims[0][0]
        max_k, max_m, max_count = mmm_limits()
        if K > max_k or M > max_m:
            no('M = %d, K = %d exceed the limits of the block (%s)' % (M, K, _limits_text()))
            continue
        big = _largest_host_count(X)
        if big is not None and big > max_count:
            no('a count of %d exceeds the limits of the block (%s)' % (big, _limits_text()))
            continue
        kids = [(R, [Z]), (Z, [X]), (X, []), (P, [X])]
        if any([c for c, _ in n.children] != want for n, want in kids):
            no('one of its roles has other children as well')
            continue
        if any(n.observed for n in below):
            no('Z, P or R is observed')
            continue
        bad = [(nm, n._init[0]) for n, nm, ok in ((Z, 'Z', ('value',)), (R, 'R', ('parameters',)))
               if n._init is not None and n._init[0] not in ok]
        if bad:
            no('%s is initialised by %s' % bad[0])
            continue
        return dict(X=X, Z=Z, P=P, R=R)
    return None


class MultinomialMixturePlan(PlateMixturePlan):

    KERNELS = MMMKernels
    LABEL, KIND = LABEL, 'mmm'
    TERMS = ('X', 'Z', 'P', 'R')
    DIMS = ('N', 'M', 'K')

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates=(N,)), Multinomial, n, "
                "Dirichlet(const, plates=(K,))) over M words with a constant number of trials n, "
                "fully observed, %s; every mask is declined" % _limits_text())

    @staticmethod
    def match(nodes, why=None):
        return match_multinomial_mixture(nodes, why)

    def _set_shape(self, roles):
        (self.N,), self.M = roles['X'].plates, roles['P'].dims[0][0]

    def _repacks(self, node):
        """Fully observed only."""
        return node._mask is True

    def get_mask(self, node):
        return np.array(True)

    # -- set-up ------------------------------------------------------------------------------------
    def _pack(self):
        """``X._data`` as 16 bits per entry and the sum of the multinomial coefficients; counts
        that are negative, no integers or do not add up to ``n`` are the reference's ValueError
        (multinomial.py), one above the cap NotImplementedError."""
        rt, torch = self.rt, self.rt.torch
        N, M = self.N, self.M
        trials = row_trials(self.X)
        if trials is None:
            raise ValueError('the number of trials of %s does not broadcast to its rows'
                             % self.X.name)
        t, dtype = observed_tensor(rt, self.X, N, M, _DTYPES)
        self.xp = torch.zeros(max(N * M, 4), dtype=torch.int16, device=rt.device)
        flags = torch.zeros(4, dtype=torch.int32, device=rt.device)
        nd = torch.from_numpy(trials if N else np.zeros(1, dtype=np.int64)).to(rt.device)
        self.kernels.pack(N, M, dtype, t, nd, self.xp, flags, self.lcoef, self.ws)
        f = flags.cpu().numpy()
        if f[0]:
            raise ValueError("Counts must be integers" if f[2] else "Counts must be non-negative")
        if f[1]:
            raise NotImplementedError('%s: an observed count exceeds %d (%s); the generic engine '
                                      'takes such data' % (LABEL, mmm_limits()[2], _limits_text()))
        if f[3]:
            raise ValueError("Counts must sum to the number of trials")
        self._stale = False

    def _materialize(self):
        if self._ready:
            if self._stale:
                self._restate()
            return
        self._delta = _delta.delta_roles(self.roles)
        rt, k = self.rt, self.kernels
        N, M, K = self.N, self.M, self.K
        rt.sync_stream()
        self.chunk, wsd = k.plan(N, M, K)
        self.ws = rt.empty(int(wsd))
        self.lcoef = rt.zeros(1)
        self._pack()
        pp = prior_table(self.P, (K, M))
        pr = prior_table(self.R, (K,))
        # K Dirichlet rows of M columns: element (k, m) at k M + m
        self.prior_p, self.prior_r = self._up(pp), self._up(pr)
        self.alpha_p, self.elog_p = rt.empty(K, M), rt.empty(K, M)
        self.alpha_r, self.elog_r = rt.empty(K), rt.empty(K)
        self.L, self.c = rt.zeros(M, K), rt.zeros(K)
        self.S, self.Nk = rt.zeros(K, M), rt.zeros(K)
        self.ws_small = rt.empty(max(M * K, 1024))
        # [0] sum lse, [1] N_k . c used, [2] S . L used, [3] bound of P, [4] bound of R,
        # [5] S . <log p>, [6] N_k . <log pi>
        self.scal = rt.zeros(8)
        self._init_p(pp)
        self._weights_step(4, self._weights_init_counts(pr))
        self._labels_from_init()
        self._tables(None)
        self._ready = True
        self._run_pass()

    def _init_p(self, prior):
        """Initial parameters and <log p> table: the prior, given parameters (device), or the logs
        of a value / of a draw from the prior (host, set-up)."""
        k = self.kernels
        K, M = self.K, self.M
        init = self.P._init
        counts = None
        if init is not None and init[0] == 'parameters':
            a = np.asarray(init[1][0], dtype=np.float64)
            if np.any(a <= 0):
                raise ValueError("Natural parameters should be positive")
            counts = self._up(np.broadcast_to(a, (K, M)) - prior)
        k.dirichlet(K, M, M, 1, self.prior_p, counts, self.alpha_p, self.elog_p, self.ws_small,
                    self.scal[3:4])
        if init is None or init[0] == 'parameters':
            return
        if init[0] == 'value':
            p = np.broadcast_to(np.asarray(init[1], dtype=np.float64), (K, M))
        else:
            g = np.random.gamma(prior)
            p = g / g.sum(axis=-1, keepdims=True)
        with np.errstate(divide='ignore'):
            e = np.log(p)
        self.elog_p.copy_(self._up(e))
        self.alpha_p.fill_(float('nan'))                # a point mass has no parameters

    def _tables(self, elog_p):
        """The tables of the pass from ``elog_p`` (None: no observation term) and ``elog_r``."""
        self.kernels.tables(self.M, self.K, elog_p, self.elog_r, self.L, self.c)

    def _run_pass(self, r_out=None):
        """The statistics of the present ``Z`` state (tables ``L`` / ``c`` or labels)."""
        self.kernels.pass_(self.N, self.M, self.K, self.xp, self.labels, self.L, self.c, self.ws,
                           self.S, self.Nk, self.scal, r_out)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        self.rt.sync_stream()
        K, M = self.K, self.M
        if node is self.Z:
            self.labels = None
            self._tables(self.elog_p)
            self._run_pass()
        elif node is self.P:
            self.kernels.dirichlet(K, M, M, 1, self.prior_p, self.S, self.alpha_p, self.elog_p,
                                   self.ws_small, self.scal[3:4])
        elif node is self.R:
            self._weights_step(4, self.Nk)
        else:
            return
        self._version += 1

    def _bound_terms(self):
        k = self.kernels
        k.dot(self.K * self.M, self.S, self.elog_p, self.ws_small, self.scal[5:6])
        k.dot(self.K, self.Nk, self.elog_r, self.ws_small, self.scal[6:7])
        s, entropy = self._host_scal()
        lcoef = float(self.lcoef.cpu().numpy()[0])
        return dict(X=float(s[5]) + lcoef, Z=float(s[6]) + entropy, P=float(s[3]), R=float(s[4]))

    def get_moments(self, node):
        self._materialize()
        N, M, K = self.N, self.M, self.K
        if node is self.R:
            return [self.elog_r.cpu().numpy().reshape(self.R.plates + (K,)).copy()]
        if node is self.P:
            return [self.elog_p.cpu().numpy().reshape(K, M).copy()]
        if node is self.Z:
            return [self.responsibilities().cpu().numpy().reshape(N, K)]
        if node is self.X:
            xp = self.xp.cpu().numpy()[:N * M].view(np.uint16).reshape(N, M)
            return [xp.astype(np.float64)]
        raise NotImplementedError

    # -- persistence -----------------------------------------------------------------------------------
    _SAVED = ('alpha_p', 'elog_p', 'alpha_r', 'elog_r', 'L', 'c', 'S', 'Nk', 'scal')


class MultinomialMixtureSVIPlan(MixtureSVI, MultinomialMixturePlan):
    """The block under stochastic variational inference (_mixture_svi.py): ``Z`` and ``X`` hold a
    mini-batch that stands for ``m`` times as many rows (``plates_multiplier``), every step
    re-observes ``X`` -- the device state stays -- and updates ``Z`` (one pack, one pass), and
    ``gradient_step`` moves P and R along their natural gradients in one launch.  Opt-in:
    ``VB(..., engine='fused+batches')`` (everything of ``engine='fused'`` plus these forms),
    tried after ``MultinomialMixturePlan``."""

    KIND, PARAM = 'mmm_svi', 'P'

    @staticmethod
    def describe():
        return ('the model of the fused multinomial-mixture block with plates_multiplier=(m,) on Z (mini-batches: one '
                'positive factor on the row axis of Z and X, none on P or R)')

    @staticmethod
    def match(nodes, why=None):
        return match_multinomial_mixture(nodes, why, batches=True)

    def _step_table(self):
        return dict(kind=0, rows=self.K, cols=self.M, rs=self.M, cs=1, prior=self.prior_p,
                    prior_b=None, stat=self.S, cnt=None, per_element=0, par=self.alpha_p,
                    mom=self.elog_p)
