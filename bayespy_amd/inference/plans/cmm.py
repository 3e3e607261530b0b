"""
Execution plan of the categorical-mixture block (the latent class model)

    R = Dirichlet(const);  Z = Categorical(R, plates=(N, 1))
    P = Dirichlet(const, plates=(D, K));  X = Mixture(Z, Categorical, P);  X.observe(x)

with constant concentrations, x (N, D) integers in [0, M), K <= 64, 2 <= M <= 32 and a count table
of roundup(D, 64 / KP) M KP doubles (KP = 16, 32 or 64 lanes for the K clusters) within the LDS cap
of ``vmp_cmm_limits``; ``X`` fully observed or observed with a mask of the full shape (N, D).
Opt-in: ``VB(..., engine='fused')``; the default engine runs this model on the generic engine as
before.  The plan owns, in HBM: ``x`` as one byte per entry (255 = hidden), the Dirichlet
parameters and <log P> CATEGORY-MAJOR as (M, D K) tables -- a (d, k) row of ``P`` has row stride 1
and column stride D K, ``vmp_lda_dirichlet`` updates all D K rows in one launch and the K values
a lookup needs are contiguous --, those of ``R`` (K), the tables L = <log P> and c = <log pi> less
its maximum that the last ``Z`` update used, and the statistics
S[m, d, k] = sum_n r_nk [x_nd = m], N_k = sum_n r_nk.  Nothing of size (N, K), (N, D, K) or
(N, D, M) exists: the responsibilities of ``Z`` are formed inside ``vmp_cmm_pass`` and only on
request written out (``Z.get_moments()``).

All plate terms of the lower bound follow from the statistics, sum_n lse_n and the tables:
    <log p(X)>           = sum S . <log P>            (the present table)
    <log p(Z)> + entropy = sum_k N_k <log pi_k> + sum_n lse_n - N_k . c_used - S . L_used
``L`` and ``c`` are written by a ``Z`` update only, so ``Z.get_moments()`` after a later ``P``
update is still that update's posterior.

Masks: ``X.observe(x, mask=m)`` with ``m`` a boolean host array or a ``DeviceMask`` of shape
exactly (N, D).  A hidden position becomes the reserved byte when ``x`` is packed and is never
interpreted: NaN, -1 or 1e300 may stand there.  The pass is the same kernel with or without a mask
(a mask of ones gives the bits of the unmasked run) and the Dirichlet counts need no separate
M_dk: S already counts the observed entries only.  A row with nothing observed has ``Z.mask``
False: its moment is softmax(<log pi>) of the tables the last update used and it enters neither
N_k nor the bound term of ``Z``.  A column with nothing observed leaves its rows of ``P`` at the
prior, with a bound term of exactly zero.  A scalar mask or one that broadcasts over a plate is
declined (generic engine).

Checkpoints: the block writes its own ``plans/<i>/`` group (kind 'cmm'); a checkpoint whose mask
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
from ...device import ptr
from ...nodes.dirichlet import Dirichlet
from ...nodes.categorical import Categorical
from ...nodes.categorical_markov_chain import CategoricalMarkovChainToCategorical
from ...nodes.multinomial import Multinomial

_DTYPES = {'float64': 0, 'int64': 1, 'uint8': 2, 'int32': 3}
_LIMITS = []


def cmm_limits():
    """(max K, min M, max M, max cells of the LDS count table) of the built pass: host-only
    ``vmp_cmm_limits``."""
    if not _LIMITS:
        v = [ctypes.c_int32() for _ in range(4)]
        _lib.raise_for_status(_lib.load().vmp_cmm_limits(*[ctypes.byref(a) for a in v]))
        _LIMITS.append(tuple(a.value for a in v))
    return _LIMITS[0]


def cmm_supported(N, D, K, M):
    """Whether the built pass takes the shape: host-only ``vmp_cmm_plan``."""
    c, w = ctypes.c_int64(), ctypes.c_int64()
    return _lib.load().vmp_cmm_plan(N, D, K, M, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_OK


def _limits_text():
    return ('K <= %d, %d <= M <= %d and a count table of roundup(D, 64 / KP) M KP <= %d doubles '
            'in LDS (KP = 16, 32 or 64 lanes for the K clusters)' % cmm_limits())


class CMMKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def plan(self, N, D, K, M):
        """(rows of a chunk, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_cmm_plan(N, D, K, M, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused categorical-mixture block supports '
                                  + _limits_text())
        return c.value, w.value

    def pack(self, N, D, M, dtype, x, mask, xb, flag):
        self.rt.check(self.lib.vmp_cmm_pack(self.ctx, N, D, M, dtype, ptr(x), _p(mask), ptr(xb),
                                            ptr(flag)))

    def tables(self, D, K, M, elog_p, elog_pi, L, c):
        self.rt.check(self.lib.vmp_cmm_tables(self.ctx, D, K, M, _p(elog_p), ptr(elog_pi), ptr(L),
                                              ptr(c)))

    def pass_(self, N, D, K, M, xb, labels, L, c, ws, S, Nk, scal, r_out=None):
        self.rt.check(self.lib.vmp_cmm_pass(self.ctx, N, D, K, M, _p(xb), _p(labels), _p(L), _p(c),
                                            _p(ws), _p(S), _p(Nk), _p(scal), _p(r_out)))


def _limits_reason(r):
    X, P = r['X'], r['P']
    (N, D), K, M = X.plates, X.clusters, P.dims[0][0]
    if not cmm_supported(N, D, K, M):
        return ('D = %d, K = %d, M = %d exceed the limits of the block (%s)'
                % (D, K, M, _limits_text()))


_SPEC = MixtureSpec(
    label='fused categorical-mixture block',
    # a hidden Markov model: plans/hmm_cat.py gives its reasons
    takes=lambda X: isinstance(X.node_class, type)
    and issubclass(X.node_class, (Categorical, Multinomial))
    and not isinstance(X.parents[0], CategoricalMarkovChainToCategorical),
    first=lambda X: None if X.node_class is Categorical else
    'the mixed distribution is %s, not Categorical' % X.node_class.__name__,
    observed='X', weights='R', params=(('P', Dirichlet, None),),
    parents='its parents are not (Categorical(Dirichlet), Dirichlet)',
    constant='the concentration of %s is a node (%s), not a constant',
    role_plates='plates of Z / P / R are not (N, 1), (D, K), ()',
    mask=full_mask_reason, plates=plates_of_p_reason, limits=_limits_reason)


class CategoricalMixturePlan(PlateMixturePlan):

    KERNELS = CMMKernels
    LABEL, KIND = _SPEC.label, 'cmm'
    TERMS = ('X', 'Z', 'P', 'R')
    DIMS = ('N', 'D', 'K', 'M')

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates=(N, 1)), Categorical, "
                "Dirichlet(const, plates=(D, K))) over M categories, fully observed or observed "
                "with a mask of the full shape (N, D), %s; a scalar mask or one that broadcasts "
                "over a plate is declined" % _limits_text())

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _SPEC)

    def __init__(self, roles, runtime=None, kernels=None):
        self.M = roles['P'].dims[0][0]
        super().__init__(roles, runtime=runtime, kernels=kernels)

    def _repacks(self, node):
        """With any mask of the full shape or none."""
        return _takes_mask(node)

    # -- set-up ------------------------------------------------------------------------------------
    def _pack(self):
        """``X._data`` as bytes; an observed value that is no integer in [0, M) is the reference's
        ValueError (categorical.py)."""
        rt, torch = self.rt, self.rt.torch
        N, D = self.N, self.D
        t, dtype = observed_tensor(rt, self.X, N, D, _DTYPES)
        self.xb = torch.zeros(max(N * D, 8), dtype=torch.uint8, device=rt.device)
        flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
        self.kernels.pack(N, D, self.M, dtype, t, self.maskd, self.xb, flag)
        if int(flag.cpu().numpy()[0]) != 0:
            raise ValueError("Invalid category index")
        self._stale = False

    def _materialize(self):
        if self._ready:
            if self._stale:
                self._restate()
            return
        self._delta = _delta.delta_roles(self.roles)
        rt, k = self.rt, self.kernels
        N, D, K, M = self.N, self.D, self.K, self.M
        rt.sync_stream()
        self._upload_mask()
        self.chunk, wsd = k.plan(N, D, K, M)
        self._pack()
        pp = prior_table(self.P, (D, K, M))
        pr = prior_table(self.R, (K,))
        # D K Dirichlet rows of M columns in the category-major table: element (dk, m) at dk + m D K
        self.prior_p, self.prior_r = self._up(pp.reshape(D * K, M).T), self._up(pr)
        self.alpha_p, self.elog_p = rt.empty(M, D * K), rt.empty(M, D * K)
        self.alpha_r, self.elog_r = rt.empty(K), rt.empty(K)
        self.L, self.c = rt.zeros(M, D * K), rt.zeros(K)
        self.S, self.Nk = rt.zeros(M, D * K), rt.zeros(K)
        self.ws = rt.empty(int(wsd))
        self.ws_small = rt.empty(max(D * K, 1024))
        # [0] sum lse, [1] N_k . c used, [2] S . L used, [3] bound of P, [4] bound of R,
        # [5] S . <log P>, [6] N_k . <log pi>
        self.scal = rt.zeros(8)
        self._init_p(pp)
        self._weights_step(4, self._weights_init_counts(pr))
        self._labels_from_init()
        self._tables(None)
        self._ready = True
        self._run_pass()

    def _init_p(self, prior):
        """Initial parameters and <log P> table: the prior, given parameters (device), or the logs
        of a value / of a draw from the prior (host, set-up)."""
        rt, k = self.rt, self.kernels
        torch = rt.torch
        D, K, M = self.D, self.K, self.M
        init = self.P._init

        def major(a):       # (D, K, M) -> (M, D K)
            return torch.from_numpy(np.array(a.reshape(D * K, M).T, order='C')).to(rt.device)
        counts = None
        if init is not None and init[0] == 'parameters':
            a = np.asarray(init[1][0], dtype=np.float64)
            if np.any(a <= 0):
                raise ValueError("Natural parameters should be positive")
            counts = major(np.broadcast_to(a, (D, K, M)) - prior)
        k.dirichlet(D * K, M, 1, D * K, self.prior_p, counts, self.alpha_p, self.elog_p,
                    self.ws_small, self.scal[3:4])
        if init is None or init[0] == 'parameters':
            return
        if init[0] == 'value':
            p = np.broadcast_to(np.asarray(init[1], dtype=np.float64), (D, K, M))
        else:
            g = np.random.gamma(prior)
            p = g / g.sum(axis=-1, keepdims=True)
        with np.errstate(divide='ignore'):
            e = np.log(p)
        self.elog_p.copy_(major(e))
        self.alpha_p.fill_(float('nan'))                # a point mass has no parameters

    def _tables(self, elog_p):
        """The tables of the pass from ``elog_p`` (None: no observation term) and ``elog_r``."""
        self.kernels.tables(self.D, self.K, self.M, elog_p, self.elog_r, self.L, self.c)

    def _run_pass(self, r_out=None):
        """The statistics of the present ``Z`` state (tables ``L`` / ``c`` or labels)."""
        self.kernels.pass_(self.N, self.D, self.K, self.M, self.xb, self.labels, self.L, self.c,
                           self.ws, self.S, self.Nk, self.scal, r_out)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        self.rt.sync_stream()
        D, K, M = self.D, self.K, self.M
        if node is self.Z:
            self.labels = None
            self._tables(self.elog_p)
            self._run_pass()
        elif node is self.P:
            self.kernels.dirichlet(D * K, M, 1, D * K, self.prior_p, self.S, self.alpha_p,
                                   self.elog_p, self.ws_small, self.scal[3:4])
        elif node is self.R:
            self._weights_step(4, self.Nk)
        else:
            return
        self._version += 1

    def _bound_terms(self):
        k = self.kernels
        k.dot(self.M * self.D * self.K, self.S, self.elog_p, self.ws_small, self.scal[5:6])
        k.dot(self.K, self.Nk, self.elog_r, self.ws_small, self.scal[6:7])
        s, entropy = self._host_scal()
        return dict(X=float(s[5]), Z=float(s[6]) + entropy, P=float(s[3]), R=float(s[4]))

    def get_moments(self, node):
        self._materialize()
        if node is self.R:
            return [self.elog_r.cpu().numpy().reshape(self.R.plates + (self.K,)).copy()]
        if node is self.P:
            return [self.elog_p.cpu().numpy().reshape(self.M, self.D, self.K)
                    .transpose(1, 2, 0).copy()]
        if node is self.Z:
            return [self.responsibilities().cpu().numpy().reshape(self.N, 1, self.K)]
        if node is self.X:
            xb = self.xb.cpu().numpy()[:self.N * self.D].reshape(self.N, self.D)
            return [(xb[..., None] == np.arange(self.M)).astype(np.float64)]
        raise NotImplementedError

    # -- persistence -----------------------------------------------------------------------------------
    _SAVED = ('alpha_p', 'elog_p', 'alpha_r', 'elog_r', 'L', 'c', 'S', 'Nk', 'scal')


class CategoricalMixtureSVIPlan(MixtureSVI, CategoricalMixturePlan):
    """The block under stochastic variational inference (_mixture_svi.py): ``Z`` and ``X`` hold a
    mini-batch that stands for ``m`` times as many rows (``plates_multiplier``), every step
    re-observes ``X`` -- the device state stays -- and updates ``Z`` (one pack, one pass), and
    ``gradient_step`` moves P and R along their natural gradients in one launch.  Opt-in:
    ``VB(..., engine='fused+batches')`` (everything of ``engine='fused'`` plus these forms),
    tried after ``CategoricalMixturePlan``."""

    KIND, PARAM = 'cmm_svi', 'P'

    @staticmethod
    def describe():
        return ('the model of the fused categorical-mixture block with plates_multiplier=(m, 1) on Z (mini-batches: one '
                'positive factor on the row axis of Z and X, none on P or R)')

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _SPEC, batches=True)

    def _step_table(self):
        DK = self.D * self.K      # the category-major table: element (dk, m) at dk + m D K
        return dict(kind=0, rows=DK, cols=self.M, rs=1, cs=DK, prior=self.prior_p, prior_b=None,
                    stat=self.S, cnt=None, per_element=0, par=self.alpha_p, mom=self.elog_p)
