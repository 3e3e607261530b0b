"""
Execution plan of the Poisson-mixture block (count clustering)

    R = Dirichlet(const);  Z = Categorical(R, plates=(N, 1))
    lam = Gamma(const, const, plates=(D, K));  X = Mixture(Z, Poisson, lam);  X.observe(x[, mask=m])

with constant ``a``, ``a0``, ``b0``, x (N, D) counts of at most 65534, K <= 64 and D <= 1024; ``X``
fully observed or observed with a mask of the full shape (N, D).  Opt-in:
``VB(..., engine='fused')``; the default engine runs this model on the generic engine as before.
The plan owns, in HBM: ``x`` as one uint16 per entry (0xFFFF = hidden), the parameters (a, b) and
the moments (<lam>, <log lam>) of ``lam`` as (D K, 2) tables, those of ``R`` (K), the tables
l = <log lam>, lb = <lam> and c that the last ``Z`` update used, and the statistics
S[d, k] = sum_n r_nk x_nd, N_k and, with hidden entries, M[d, k] = sum_n r_nk m_nd.  Nothing of size
(N, K) or (N, D, K) exists: the responsibilities of ``Z`` are formed inside ``vmp_pmm_pass`` and
only on request written out (``Z.get_moments()``).

All plate terms of the lower bound follow from the statistics, sum_n lse_n and the tables:
    <log p(X)>           = S . <log lam> - M . <lam> - sum_observed lgamma(x + 1)   (M_dk = N_k
                           where nothing is hidden; the last sum comes from the pack)
    <log p(Z)> + entropy = sum_k N_k <log pi_k> + sum_n lse_n - N_k . c_used - scal[2]
``l``, ``lb`` and ``c`` are written by a ``Z`` update only, so ``Z.get_moments()`` after a later
``lam`` update is still that update's posterior.

Masks: ``X.observe(x, mask=m)`` with ``m`` a boolean host array or a ``DeviceMask`` of shape
exactly (N, D).  A hidden position becomes 0xFFFF when ``x`` is packed and is never interpreted:
NaN, -1 or 1e300 may stand there.  The pack counts the hidden entries; the pass runs its form with
two statistics only when there are any, so a mask of ones gives the bits of the unmasked run.  A
row with nothing observed has ``Z.mask`` False: its moment is softmax(c) of the tables the last
update used and it enters neither N_k nor the bound term of ``Z``.  A column with nothing observed
leaves its ``lam`` at the prior, with a bound term of exactly zero.  A scalar mask or one that
broadcasts over a plate is declined (generic engine).

Checkpoints: the block writes its own ``plans/<i>/`` group (kind 'pmm'); a checkpoint whose mask
differs is refused.
"""
import ctypes

import numpy as np

from . import _delta
from ._dirichlet import DirichletKernels, prior_table
from ._mixture_svi import MixtureSVI
from ._mixture import (MixtureSpec, PlateMixturePlan, _p, _takes_mask, cluster_plate_reason,
                       full_mask_reason, match_plate_mixture, observed_tensor)

from ... import _lib
from ...nodes.node import DeviceMask
from ...nodes.categorical_markov_chain import CategoricalMarkovChainToCategorical
from ...nodes.gamma import Gamma
from ...nodes.poisson import Poisson

_DTYPES = {'float64': 0, 'int64': 1, 'uint8': 2, 'int32': 3}
_LIMITS = []


def pmm_limits():
    """(max K, max D, largest count) of the built pass: host-only ``vmp_pmm_limits``."""
    if not _LIMITS:
        v = [ctypes.c_int32() for _ in range(3)]
        _lib.raise_for_status(_lib.load().vmp_pmm_limits(*[ctypes.byref(a) for a in v]))
        _LIMITS.append(tuple(a.value for a in v))
    return _LIMITS[0]


def _limits_text():
    return 'K <= %d, D <= %d and counts of at most %d' % pmm_limits()


class PMMKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def plan(self, N, D, K):
        """(rows of a chunk, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_pmm_plan(N, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused Poisson-mixture block supports ' + _limits_text())
        return c.value, w.value

    def pack(self, N, D, dtype, x, mask, xp, flags, counts, lgam, ws):
        self.rt.check(self.lib.vmp_pmm_pack(self.ctx, N, D, dtype, _p(x), _p(mask), _p(xp),
                                            _p(flags), _p(counts), _p(lgam), _p(ws)))

    def tables(self, D, K, form, lam_mom, elog_pi, l, lb, c, lsum=None):
        self.rt.check(self.lib.vmp_pmm_tables(self.ctx, D, K, form, _p(lam_mom), _p(elog_pi),
                                              _p(l), _p(lb), _p(c), _p(lsum)))

    def pass_(self, N, D, K, hidden, xp, labels, l, lb, c, ws, S, M, Nk, scal, r_out=None):
        self.rt.check(self.lib.vmp_pmm_pass(self.ctx, N, D, K, hidden, _p(xp), _p(labels), _p(l),
                                            _p(lb), _p(c), _p(ws), _p(S), _p(M), _p(Nk), _p(scal),
                                            _p(r_out)))

    def update(self, D, K, per_element, prior_a, prior_b, S, cnt, par, mom, bound):
        self.rt.check(self.lib.vmp_pmm_update(self.ctx, D, K, per_element, _p(prior_a),
                                              _p(prior_b), _p(S), _p(cnt), _p(par), _p(mom),
                                              _p(bound)))


def _largest_host_count(X):
    """The largest observed count where ``X`` holds a host array, else None (a device tensor is
    judged by the pack)."""
    x = X._data
    if x is None or not isinstance(x, (np.ndarray, list, tuple, int, float, np.number)):
        return None
    a = np.asarray(x)
    if a.dtype.kind not in 'iuf' or a.size == 0:
        return None
    m = X._mask
    if m is not True and not isinstance(m, DeviceMask):
        try:
            a = a[np.broadcast_to(np.asarray(m, dtype=bool), a.shape)]
        except ValueError:
            return None
    a = a[np.isfinite(a)] if a.dtype.kind == 'f' else a
    return a.max() if a.size else None


def _plates_reason(X, lam):
    if len(X.plates) != 2 or len(lam.plates) != 2:
        return ('it needs plates (N, D), X has plates %s and lam has plates %s'
                % (X.plates, lam.plates))


def _limits_reason(r):
    X = r['X']
    D, K = X.plates[1], X.clusters
    max_k, max_d, max_count = pmm_limits()
    if K > max_k or D > max_d:
        return 'D = %d, K = %d exceed the limits of the block (%s)' % (D, K, _limits_text())
    big = _largest_host_count(X)
    if big is not None and big > max_count:
        return 'a count of %d exceeds the limits of the block (%s)' % (big, _limits_text())


_SPEC = MixtureSpec(
    label='fused Poisson-mixture block',
    # a hidden Markov model: no block of this family
    takes=lambda X: X.node_class is Poisson
    and not isinstance(X.parents[0], CategoricalMarkovChainToCategorical),
    observed='X', weights='R', params=(('lam', Gamma, ('value', 'parameters')),),
    parents='its parents are not (Categorical(Dirichlet), Gamma)',
    constant='a parameter of %s is a node (%s), not a constant',
    role_plates='plates of Z / lam / R are {} / {} / {}, not (N, 1) / (D, K) / ()',
    mask=full_mask_reason,
    plates=lambda X, lam: cluster_plate_reason(X) or _plates_reason(X, lam),
    limits=_limits_reason)


class PoissonMixturePlan(PlateMixturePlan):

    KERNELS = PMMKernels
    LABEL, KIND = _SPEC.label, 'pmm'
    TERMS = ('X', 'Z', 'lam', 'R')
    _FLAGS = ('_used',)

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates=(N, 1)), Poisson, "
                "Gamma(const, const, plates=(D, K))), fully observed or observed with a mask of "
                "the full shape (N, D), %s; a scalar mask or one that broadcasts over a plate is "
                "declined" % _limits_text())

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _SPEC)

    def __init__(self, roles, runtime=None, kernels=None):
        super().__init__(roles, runtime=runtime, kernels=kernels)
        self.hidden = 0             # the form of the pass: 1 when the pack met a hidden entry

    def _repacks(self, node):
        """With any mask of the full shape or none."""
        return _takes_mask(node)

    # -- set-up ------------------------------------------------------------------------------------
    def _pack(self):
        """``X._data`` as 16 bits per entry; an observed value that is negative or no integer is
        the reference's ValueError (poisson.py), one above the cap NotImplementedError."""
        rt, torch = self.rt, self.rt.torch
        N, D = self.N, self.D
        t, dtype = observed_tensor(rt, self.X, N, D, _DTYPES)
        self.xp = torch.zeros(max(N * D, 4), dtype=torch.int16, device=rt.device)
        flags = torch.zeros(3, dtype=torch.int32, device=rt.device)
        counts = torch.zeros(2, dtype=torch.int64, device=rt.device)
        self.kernels.pack(N, D, dtype, t, self.maskd, self.xp, flags, counts, self.lgam, self.ws)
        f = flags.cpu().numpy()
        if f[0]:
            raise ValueError("Values must be integers" if f[2] else "Values must be positive")
        if f[1]:
            raise NotImplementedError('fused Poisson-mixture block: an observed count exceeds %d '
                                      '(%s); the generic engine takes such data'
                                      % (pmm_limits()[2], _limits_text()))
        n = counts.cpu().numpy()
        self.n_observed, self.n_hidden = int(n[0]), int(n[1])
        self._stale = False

    def _adopt_form(self):
        self.hidden = 1 if self.n_hidden > 0 else 0

    def _set_form(self):
        """The form of the pass for the packed data; when it changes, the tables of the last ``Z``
        update are formed again in the new one."""
        hidden = self.hidden
        self._adopt_form()
        if hidden != self.hidden:
            self._tables(self.lam_mom_used if self._used else None, self.elog_r_used)

    def _const(self, i, what):
        a = np.asarray(self.lam.parents[i].value, dtype=np.float64)
        if np.any(a <= 0):
            raise ValueError('%s of %s should be positive' % (what, self.lam.name))
        return np.ascontiguousarray(np.broadcast_to(a, (self.D, self.K)))

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
        self.lgam = rt.zeros(1)
        self._pack()
        self.hidden = 1 if self.n_hidden > 0 else 0
        a0, b0 = self._const(0, 'a0'), self._const(1, 'b0')
        pr = prior_table(self.R, (K,))
        self.a0, self.b0, self.prior_r = self._up(a0), self._up(b0), self._up(pr)
        self.lam_par, self.lam_mom = rt.empty(D * K, 2), rt.empty(D * K, 2)
        self.lam_mom_used, self.elog_r_used = rt.zeros(D * K, 2), rt.zeros(K)
        self._used = False          # whether the tables in use hold an observation term
        self.alpha_r, self.elog_r = rt.empty(K), rt.empty(K)
        self.l, self.lb, self.c = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
        self.l_now, self.lb_now, self.c_now = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
        self.lsum = rt.zeros(K)
        self.S, self.M, self.Nk = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
        self.ws_small = rt.empty(max(D * K, 1024))
        # [0] sum lse, [1] N_k . c used, [2] S . l - M . lb used, [3] bound of lam, [4] of R,
        # [5] S . <log lam>, [6] M . <lam> (N_k . sum_d <lam>), [7] N_k . <log pi>
        self.scal = rt.zeros(8)
        k.update(D, K, 0, self.a0, self.b0, None, None, self.lam_par, self.lam_mom,
                 self.scal[3:4])
        self._init_lam(a0, b0)
        self._weights_step(4, self._weights_init_counts(pr))
        self._labels_from_init()
        self.elog_r_used.copy_(self.elog_r)
        self._tables(None, self.elog_r_used)
        self._ready = True
        self._run_pass()

    def _init_lam(self, a0, b0):
        """A given initial state of ``lam`` (host, set-up): a point mass, or Gamma(a, b)."""
        init = self.lam._init
        if init is None:
            return
        D, K = self.D, self.K
        if init[0] == 'value':
            v = np.broadcast_to(np.asarray(init[1], dtype=np.float64), (D, K))
            if np.any(v <= 0):
                raise ValueError('the value given to %s should be positive' % self.lam.name)
            self.lam_mom.copy_(self._up(np.stack([v, np.log(v)], -1).reshape(D * K, 2)))
            self.lam_par.fill_(float('nan'))             # a point mass has no parameters
            return
        from scipy.special import digamma, gammaln
        a, b = (np.broadcast_to(np.asarray(v, dtype=np.float64), (D, K)) for v in init[1][:2])
        if np.any(a <= 0) or np.any(b <= 0):
            raise ValueError('the parameters given to %s should be positive' % self.lam.name)
        self.lam_par.copy_(self._up(np.stack([a, b], -1).reshape(D * K, 2)))
        self.lam_mom.copy_(self._up(np.stack([a / b, digamma(a) - np.log(b)],
                                             -1).reshape(D * K, 2)))
        bound = a0 * (np.log(b0) - np.log(b)) - gammaln(a0) + gammaln(a) + (a0 - a) * digamma(a) \
            + a - b0 * a / b
        self.scal[3:4].copy_(self._up([bound.sum()]))

    def _tables(self, lam_mom, elog_r):
        """The tables of the pass, in its present form and centred (column 0 of every row taken
        out: the logits stay small, the entropy does not notice), from the given moments (None: no
        observation term)."""
        self.kernels.tables(self.D, self.K, self.hidden | 2, lam_mom, elog_r, self.l, self.lb,
                            self.c)

    def _run_pass(self, r_out=None):
        """The statistics of the present ``Z`` state (tables ``l`` / ``lb`` / ``c`` or labels)."""
        self.kernels.pass_(self.N, self.D, self.K, self.hidden, self.xp, self.labels, self.l,
                           self.lb, self.c, self.ws, self.S, self.M, self.Nk, self.scal, r_out)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        rt, k = self.rt, self.kernels
        rt.sync_stream()
        D, K = self.D, self.K
        if node is self.Z:
            self.labels = None
            self.lam_mom_used.copy_(self.lam_mom)
            self.elog_r_used.copy_(self.elog_r)
            self._used = True
            self._tables(self.lam_mom_used, self.elog_r_used)
            self._run_pass()
        elif node is self.lam:
            k.update(D, K, self.hidden, self.a0, self.b0, self.S,
                     self.M if self.hidden else self.Nk, self.lam_par, self.lam_mom,
                     self.scal[3:4])
        elif node is self.R:
            self._weights_step(4, self.Nk)
        else:
            return
        self._version += 1

    def _bound_terms(self):
        k = self.kernels
        D, K = self.D, self.K
        k.tables(D, K, self.hidden, self.lam_mom, self.elog_r, self.l_now, self.lb_now,
                 self.c_now, self.lsum)
        k.dot(D * K, self.S, self.l_now, self.ws_small, self.scal[5:6])
        if self.hidden:
            k.dot(D * K, self.M, self.lb_now, self.ws_small, self.scal[6:7])
        else:
            k.dot(K, self.Nk, self.lsum, self.ws_small, self.scal[6:7])
        k.dot(K, self.Nk, self.elog_r, self.ws_small, self.scal[7:8])
        s, entropy = self._host_scal()
        lgam = float(self.lgam.cpu().numpy()[0])
        return dict(X=float(s[5] - s[6]) - lgam, Z=float(s[7]) + entropy, lam=float(s[3]),
                    R=float(s[4]))

    def get_moments(self, node):
        self._materialize()
        D, K = self.D, self.K
        if node is self.R:
            return [self.elog_r.cpu().numpy().reshape(self.R.plates + (K,)).copy()]
        if node is self.lam:
            m = self.lam_mom.cpu().numpy().reshape(D, K, 2)
            return [m[..., 0].copy(), m[..., 1].copy()]
        if node is self.Z:
            return [self.responsibilities().cpu().numpy().reshape(self.N, 1, K)]
        if node is self.X:
            xp = self.xp.cpu().numpy()[:self.N * D].view(np.uint16).reshape(self.N, D)
            return [np.where(xp == 0xFFFF, 0, xp).astype(np.float64)]
        raise NotImplementedError

    # -- persistence -----------------------------------------------------------------------------------
    _SAVED = ('lam_par', 'lam_mom', 'lam_mom_used', 'alpha_r', 'elog_r', 'elog_r_used', 'l', 'lb',
              'c', 'S', 'M', 'Nk', 'scal')


class PoissonMixtureSVIPlan(MixtureSVI, PoissonMixturePlan):
    """The block under stochastic variational inference (_mixture_svi.py): ``Z`` and ``X`` hold a
    mini-batch that stands for ``m`` times as many rows (``plates_multiplier``), every step
    re-observes ``X`` -- the device state stays -- and updates ``Z`` (one pack, one pass), and
    ``gradient_step`` moves lam and R along their natural gradients in one launch.  Opt-in:
    ``VB(..., engine='fused+batches')`` (everything of ``engine='fused'`` plus these forms),
    tried after ``PoissonMixturePlan``."""

    KIND, PARAM = 'pmm_svi', 'lam'

    @staticmethod
    def describe():
        return ('the model of the fused Poisson-mixture block with plates_multiplier=(m, 1) on Z (mini-batches: one '
                'positive factor on the row axis of Z and X, none on lam or R)')

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _SPEC, batches=True)

    def _step_table(self):
        # the Gamma pairs; with hidden entries M takes the place of N_k
        return dict(kind=1, rows=self.D * self.K, cols=2, rs=2, cs=1, prior=self.a0,
                    prior_b=self.b0, stat=self.S, cnt=self.M if self.hidden else self.Nk,
                    per_element=self.hidden, par=self.lam_par, mom=self.lam_mom)
