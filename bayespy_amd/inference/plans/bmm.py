"""
Execution plan of the Bernoulli-mixture block (doc/source/examples/bmm.rst)

    R = Dirichlet(const);  Z = Categorical(R, plates=(N, 1))
    P = Beta(const [a, b], plates=(D, K));  X = Mixture(Z, Bernoulli, P);  X.observe(x)

with constant priors, K <= 64 and D <= 1024; ``X`` fully observed or observed with a mask of the
full shape (N, D) (below).  Opt-in: ``VB(...,
engine='fused')``; the default engine runs this model on the generic engine as before.  The plan
owns, in HBM: ``x`` as bits (ceil(D / 64) words per row), the Beta parameters and moments of ``P``
as a (D K, 2) table, those of ``R`` (K), the tables w = <log p> - <log(1 - p)> and c = <log pi> +
sum_d <log(1 - p)> the last ``Z`` update used, and the statistics S_dk = sum_n r_nk x_nd,
N_k = sum_n r_nk.  Nothing of size (N, D, K) or (N, K) exists: the responsibilities of ``Z`` are
formed inside ``vmp_bmm_pass`` and only on request written out (``Z.get_moments()``).

All plate terms of the lower bound follow from the statistics, sum_n lse_n and the tables:
    <log p(X)>           = sum_dk S_dk <log p_dk> + (N_k - S_dk) <log(1 - p_dk)>
    <log p(Z)> + entropy = sum_k N_k <log pi_k>
                           + sum_n lse_n - sum_k N_k c_used[k] - sum_dk S_dk w_used[d, k]

Masks: ``X.observe(x, mask=m)`` with ``m`` a boolean host array or a ``DeviceMask`` of shape
exactly (N, D).  The row then carries two bit planes, xm = x & m and m (N D / 4 bytes in all), and
the plan keeps ``M`` and ``l0`` beside ``S`` and ``w``:
    logit_nk = c[k] + sum_d xm_nd w[d, k] + sum_d m_nd l0[d, k],   l0 = <log(1 - p)>,
    c = <log pi> (less its maximum),  S_dk = sum_n r_nk xm_nd,  M_dk = sum_n r_nk m_nd,
    N_k = sum over the rows with an observed entry of r_nk,  message to P = (S, M - S).
The two bound formulas above hold on these sums with ``counts`` = (S, M - S) for the first and
S . w + M . l0 for the last product of the second.  A row with nothing observed has ``Z.mask``
False: its moment is softmax(<log pi>) of the tables the last update used and it enters neither
N_k nor the bound term of ``Z``.  A hidden position of ``x`` is never read by the kernels.  A
scalar mask or one that broadcasts over a plate is declined (generic engine).

Checkpoints: the block writes its own ``plans/<i>/`` group (kind 'bmm') like every fused plan.  A
checkpoint of the generic engine holds the natural parameters of every node, the (N, 1, K) array
of ``Z`` among them, which this block never keeps; the two are not interchangeable.  A masked plan
adds ``mask``, ``M`` and ``l0`` and refuses a checkpoint whose mask differs; an unmasked plan
writes what it always wrote.
"""
import ctypes

import numpy as np

from . import _delta
from ._dirichlet import DirichletKernels, prior_table
from ._mixture_svi import MixtureSVI
from ._mixture import (MixtureSpec, PlateMixturePlan, _p, _takes_mask, full_mask_reason,
                       match_plate_mixture, observed_tensor, plates_of_p_reason)

from ... import _lib
from ...device import ptr
from ...nodes.beta import Beta
from ...nodes.binomial import Bernoulli, Binomial

BMM_MAX_K = 64          # vmp_bmm_limits
BMM_MAX_D = 1024
BMM_MASKED_MAX_K = 64   # vmp_bmm_limits_masked as documented; the matcher reads the built values
BMM_MASKED_MAX_D = 1024

_DTYPES = {'float64': 0, 'int64': 1, 'bool': 2, 'uint8': 2}
_MASKED_LIMITS = []


def bmm_masked_limits():
    """(max K, max D) of the built masked pass: host-only ``vmp_bmm_limits_masked``."""
    if not _MASKED_LIMITS:
        k, d = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_bmm_limits_masked(ctypes.byref(k), ctypes.byref(d)))
        _MASKED_LIMITS.append((k.value, d.value))
    return _MASKED_LIMITS[0]


class BMMKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def plan(self, N, D, K):
        """(rows of a chunk, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_bmm_plan(N, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused Bernoulli-mixture block supports K <= %d and '
                                      'D <= %d' % (BMM_MAX_K, BMM_MAX_D))
        return c.value, w.value

    def pack(self, N, D, dtype, x, xw, flag):
        self.rt.check(self.lib.vmp_bmm_pack(self.ctx, N, D, dtype, ptr(x), ptr(xw), ptr(flag)))

    def tables(self, D, K, elog_p, elog_pi, w, c):
        self.rt.check(self.lib.vmp_bmm_tables(self.ctx, D, K, _p(elog_p), ptr(elog_pi), ptr(w),
                                              ptr(c)))

    def pass_(self, N, D, K, xw, labels, w, c, ws, S, Nk, counts, scal, r_out=None):
        self.rt.check(self.lib.vmp_bmm_pass(self.ctx, N, D, K, _p(xw), _p(labels), _p(w), _p(c),
                                            _p(ws), _p(S), _p(Nk), _p(counts), _p(scal),
                                            _p(r_out)))

    # -- missing observations: two bit planes per row, tables (w, l0, c), statistics (S, M) --------
    def plan_masked(self, N, D, K):
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_bmm_plan_masked(N, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused Bernoulli-mixture block with a mask supports '
                                      'K <= %d and D <= %d' % bmm_masked_limits())
        return c.value, w.value

    def pack_masked(self, N, D, dtype, x, mask, xw, flag):
        self.rt.check(self.lib.vmp_bmm_pack_masked(self.ctx, N, D, dtype, ptr(x), ptr(mask),
                                                   ptr(xw), ptr(flag)))

    def tables_masked(self, D, K, elog_p, elog_pi, w, l0, c):
        self.rt.check(self.lib.vmp_bmm_tables_masked(self.ctx, D, K, _p(elog_p), ptr(elog_pi),
                                                     ptr(w), ptr(l0), ptr(c)))

    def pass_masked(self, N, D, K, xw, labels, w, l0, c, ws, S, M, Nk, counts, scal, r_out=None):
        self.rt.check(self.lib.vmp_bmm_pass_masked(self.ctx, N, D, K, _p(xw), _p(labels), _p(w),
                                                   _p(l0), _p(c), _p(ws), _p(S), _p(M), _p(Nk),
                                                   _p(counts), _p(scal), _p(r_out)))


def _limits_reason(r):
    X = r['X']
    D, K = X.plates[1], X.clusters
    if K > BMM_MAX_K or D > BMM_MAX_D:
        return ('D = %d, K = %d exceed the limits of the block (D <= %d, K <= %d)'
                % (D, K, BMM_MAX_D, BMM_MAX_K))
    if X._mask is not True and (K > bmm_masked_limits()[0] or D > bmm_masked_limits()[1]):
        return ('D = %d, K = %d exceed the limits of the block with a mask (D <= %d, K <= %d)'
                % ((D, K) + bmm_masked_limits()[::-1]))


_SPEC = MixtureSpec(
    label='fused Bernoulli-mixture block',
    takes=lambda X: isinstance(X.node_class, type) and issubclass(X.node_class, Binomial),
    first=lambda X: None if X.node_class is Bernoulli else
    'the mixed distribution is %s, not Bernoulli' % X.node_class.__name__,
    observed='X', weights='R', params=(('P', Beta, None),),
    parents='its parents are not (Categorical(Dirichlet), Beta)',
    constant='the parameter of %s is a node (%s), not a constant',
    role_plates='plates of Z / P / R are not (N, 1), (D, K), ()',
    mask=full_mask_reason, plates=plates_of_p_reason, limits=_limits_reason)


class BernoulliMixturePlan(PlateMixturePlan):

    KERNELS = BMMKernels
    LABEL, KIND = _SPEC.label, 'bmm'
    TERMS = ('X', 'Z', 'P', 'R')

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates=(N, 1)), Bernoulli, Beta(const, "
                "plates=(D, K))), fully observed (D <= %d, K <= %d) or observed with a mask of "
                "the full shape (N, D) (D <= %d, K <= %d); a scalar mask or one that broadcasts "
                "over a plate is declined"
                % (BMM_MAX_D, BMM_MAX_K, BMM_MASKED_MAX_D, BMM_MASKED_MAX_K))

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _SPEC)

    def _repacks(self, node):
        """With a mask of the full shape or none; a built plan keeps to the one it has."""
        return _takes_mask(node) and (not self._ready
                                      or (node._mask is True) == (self.maskd is None))

    # -- set-up ------------------------------------------------------------------------------------
    def _pack(self):
        """``X._data`` as bits (with ``maskd``, uploaded before: two planes); a value that is
        neither 0 nor 1 is the reference's ValueError (binomial.py, through Bernoulli's observe)."""
        rt, torch = self.rt, self.rt.torch
        N, D = self.N, self.D
        t, dtype = observed_tensor(rt, self.X, N, D, _DTYPES, widen_bool=False)
        W = (D + 63) // 64
        planes = 1 if self.maskd is None else 2
        self.xw = torch.zeros(max(N, 1) * W * planes, dtype=torch.int64, device=rt.device)
        flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
        if self.maskd is None:
            self.kernels.pack(N, D, dtype, t, self.xw, flag)
        else:
            self.kernels.pack_masked(N, D, dtype, t, self.maskd, self.xw, flag)
        if int(flag.cpu().numpy()[0]) != 0:
            raise ValueError("Invalid count")
        self._stale = False

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
        masked = self.maskd is not None
        self.chunk, wsd = k.plan_masked(N, D, K) if masked else k.plan(N, D, K)
        self._pack()
        pp = prior_table(self.P, (D, K, 2)).reshape(D * K, 2)
        pr = prior_table(self.R, (K,))
        self.prior_p, self.prior_r = self._up(pp), self._up(pr)
        self.alpha_p, self.elog_p = rt.empty(D * K, 2), rt.empty(D * K, 2)
        self.alpha_r, self.elog_r = rt.empty(K), rt.empty(K)
        self.w, self.c = rt.zeros(D, K), rt.zeros(K)
        self.S, self.Nk, self.counts = rt.zeros(D, K), rt.zeros(K), rt.zeros(D * K, 2)
        if masked:
            self.l0, self.M = rt.zeros(D, K), rt.zeros(D, K)
        self.ws = rt.empty(int(wsd))
        self.ws_small = rt.empty(max(D * K, 1024))
        # [0] sum lse, [1] N_k . c used, [2] S . w (+ M . l0) used, [3] bound of P, [4] bound of R,
        # [5] counts . <log p>, [6] N_k . <log pi>
        self.scal = rt.zeros(8)
        self._init_p(pp)
        self._weights_step(4, self._weights_init_counts(pr))
        self._labels_from_init()
        self._tables(None)
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

    def _tables(self, elog_p):
        """The tables of the pass from ``elog_p`` (None: no observation term) and ``elog_r``."""
        if self.maskd is None:
            self.kernels.tables(self.D, self.K, elog_p, self.elog_r, self.w, self.c)
        else:
            self.kernels.tables_masked(self.D, self.K, elog_p, self.elog_r, self.w, self.l0,
                                       self.c)

    def _run_pass(self, r_out=None):
        """The statistics of the present ``Z`` state (tables ``w`` / ``c`` or labels)."""
        if self.maskd is None:
            self.kernels.pass_(self.N, self.D, self.K, self.xw, self.labels, self.w, self.c,
                               self.ws, self.S, self.Nk, self.counts, self.scal, r_out)
        else:
            self.kernels.pass_masked(self.N, self.D, self.K, self.xw, self.labels, self.w, self.l0,
                                     self.c, self.ws, self.S, self.M, self.Nk, self.counts,
                                     self.scal, r_out)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        self.rt.sync_stream()
        D, K = self.D, self.K
        if node is self.Z:
            self.labels = None
            self._tables(self.elog_p)
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
        return dict(X=float(s[5]), Z=float(s[6]) + entropy, P=float(s[3]), R=float(s[4]))

    def get_moments(self, node):
        self._materialize()
        if node is self.R:
            return [self.elog_r.cpu().numpy().reshape(self.R.plates + (self.K,)).copy()]
        if node is self.P:
            return [self.elog_p.cpu().numpy().reshape(self.D, self.K, 2).copy()]
        if node is self.Z:
            return [self.responsibilities().cpu().numpy().reshape(self.N, 1, self.K)]
        if node is self.X:
            x = self.X._data
            x = x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)
            return [np.array(np.broadcast_to(x, (self.N, self.D)), dtype=np.float64)]
        raise NotImplementedError

    # -- persistence -----------------------------------------------------------------------------------
    _SAVED = ('alpha_p', 'elog_p', 'alpha_r', 'elog_r', 'w', 'c', 'S', 'Nk', 'counts', 'scal')

    def _saved(self):
        return self._SAVED + (('M', 'l0') if self.maskd is not None else ())


class BernoulliMixtureSVIPlan(MixtureSVI, BernoulliMixturePlan):
    """The block under stochastic variational inference (_mixture_svi.py): ``Z`` and ``X`` hold a
    mini-batch that stands for ``m`` times as many rows (``plates_multiplier``), every step
    re-observes ``X`` -- the device state stays -- and updates ``Z`` (one pack, one pass), and
    ``gradient_step`` moves P and R along their natural gradients in one launch.  Opt-in:
    ``VB(..., engine='fused+batches')`` (everything of ``engine='fused'`` plus these forms),
    tried after ``BernoulliMixturePlan``."""

    KIND, PARAM = 'bmm_svi', 'P'

    @staticmethod
    def describe():
        return ('the model of the fused Bernoulli-mixture block with plates_multiplier=(m, 1) on Z (mini-batches: one '
                'positive factor on the row axis of Z and X, none on P or R)')

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _SPEC, batches=True)

    def _step_table(self):
        DK = self.D * self.K
        return dict(kind=0, rows=DK, cols=2, rs=2, cs=1, prior=self.prior_p, prior_b=None,
                    stat=self.counts, cnt=None, per_element=0, par=self.alpha_p, mom=self.elog_p)
