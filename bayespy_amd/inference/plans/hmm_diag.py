"""
The hidden-Markov-model block (plans/hmm.py) with diagonal-Gaussian emissions: every time step
carries D real numbers with one precision per dimension (39-dimensional speech features, hundreds
of sensor channels, spectrogram frames)

    a0 = Dirichlet(const (K,));  A = Dirichlet(const (K, K))
    Z   = CategoricalMarkovChain(a0, A, states=T)                   plates () or (B,)
    mu  = GaussianARD(const m0, const beta0, shape=(D,), plates=(K,))
    tau = Gamma(const a0, const b0, plates=(K, D))
    Y   = Mixture(Z, GaussianARD, mu, tau, 1);  Y.observe(y[, mask=m])     plates (T,) or (B, T)

with priors that broadcast to (K, D), T >= 2, K <= 64 and 1 <= D <= 1024
(``vmp_hmm_diag_limits``); the full-covariance forms stop at D = 32 because their feature count
grows as D^2.

``DiagGaussianHMMPlan`` is ``HMMPlan`` -- the chain-side bookkeeping (``a0``, ``A``, the used
tables, labels, masks and their contract, ``Z.get_moments()``, ``save`` / ``load``) is inherited --
with the emission side of the diagonal-Gaussian mixture block (plans/dgmm.py): ``mu`` and ``tau``
live in its (D K, 2) tables, ``vmp_dgmm_tables`` fills h = <tau><mu>, q = -1/2 <tau> (D x K) and
g[k] = sum_d (1/2 <log tau> - 1/2 <tau><mu^2>) (its ``gsum``), ``vmp_dgmm_update`` updates the two
nodes from S1, S2, Nk and gives their bound terms.  The pass is ``vmp_hmm_diag_pass``
(csrc/vmp_hmm_diag.hip): E = g + Y h + (Y o Y) q and S1 = Y^T Gamma, S2 = (Y o Y)^T Gamma over the
whole (b, t) plate on the fp64 matrix cores, the chain kernel of the wide-emission pass between
them.  Nothing of size (B, T, K, D) exists.

    <log p(Y)>           = S1 . h + S2 . q + Nk . g - 1/2 N_obs D log 2 pi     (present moments)
    <log p(Z)> + entropy = as in plans/hmm.py, with sum gamma . e from the pass

Opt-in: ``VB(..., engine='fused+diagonal')``, which is ``engine='fused'`` with the forms of
``plans.OPT_IN_DIAGONAL_EMISSIONS`` tried right after their block.  Every other engine value keeps
its answer and never keeps such a plan on reuse.
"""
import ctypes

import numpy as np

from . import _delta
from .dgmm import DGMMKernels
from .hmm import HMMPlan, _takes_mask, _mask_shape

from ... import _lib
from ...device import ptr
from ...nodes.node import Constant
from ...nodes.dirichlet import Dirichlet
from ...nodes.gaussian import GaussianARD
from ...nodes.gamma import Gamma
from ...nodes.categorical_markov_chain import (CategoricalMarkovChain,
                                               CategoricalMarkovChainToCategorical)
from ...nodes.mixture import Mixture

LABEL = 'fused hidden-Markov-model block (diagonal-Gaussian emissions)'
_LIMITS = []


def hmm_diag_limits():
    """(max K, max D) of the built pass: host-only ``vmp_hmm_diag_limits``."""
    if not _LIMITS:
        k, d = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_hmm_diag_limits(ctypes.byref(k), ctypes.byref(d)))
        _LIMITS.append((k.value, d.value))
    return _LIMITS[0]


class DiagHMMKernels(DGMMKernels):
    """``tables`` / ``update`` of the diagonal-Gaussian mixture block, the Dirichlet kernels and
    the pass of this block."""

    def plan(self, B, T, D, K):
        """(chains of a workgroup, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_hmm_diag_plan(B, T, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the %s supports T >= 2, K <= %d and D <= %d'
                                  % ((LABEL,) + hmm_diag_limits()))
        return c.value, w.value

    def pass_(self, B, T, D, K, y, h, q, g, elog_a0, elog_A, labels, mask, ws, z0sum, xisum, S1,
              S2, Nk, scal, gamma=None, z0=None, zz=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_hmm_diag_pass(
            self.ctx, B, T, D, K, p(y), p(h), p(q), p(g), p(elog_a0), p(elog_A), p(labels),
            p(mask), p(ws), p(z0sum), p(xisum), p(S1), p(S2), p(Nk), p(scal), p(gamma), p(z0),
            p(zz)))


def _broadcasts(node, shape):
    try:
        np.broadcast_to(node.value, shape)
        return True
    except ValueError:
        return False


def _match(nodes, why):
    for Y in nodes:
        if not isinstance(Y, Mixture) or not isinstance(Y.parents[0],
                                                        CategoricalMarkovChainToCategorical):
            continue
        if Y.node_class is not GaussianARD:
            continue            # another emission family: plans/hmm.py gives its reason

        def no(msg, Y=Y):
            if why is not None:
                why.append('%s, observed node %s: %s' % (LABEL, Y.name or '<unnamed>', msg))
        Zc = Y.parents[0]
        Z = Zc.parents[0]
        if type(Z) is not CategoricalMarkovChain or len(Y.parents) != 3:
            no('its parents are not (CategoricalMarkovChain, mu, tau)')
            continue
        if Y.ndim != 1:
            no('the mixed GaussianARD has ndim = %d: the block takes vectors, '
               'Mixture(Z, GaussianARD, mu, tau, 1)' % Y.ndim)
            continue
        a0, A = Z.parents
        mu, tau = Y.parents[1], Y.parents[2]
        if type(a0) is not Dirichlet or type(A) is not Dirichlet:
            no('the initial-state and transition probabilities are not Dirichlet nodes')
            continue
        if type(mu) is not GaussianARD or type(tau) is not Gamma:
            no('mu is %s and tau is %s: the block takes (GaussianARD, Gamma) nodes; constant '
               'emission parameters go through the generic engine'
               % (type(mu).__name__, type(tau).__name__))
            continue
        roles = (Y, Z, a0, A, mu, tau)
        if not all(any(n is m for m in nodes) for n in roles):
            continue
        chain = (Y, Zc) + roles[1:]
        if any(any(m != 1 for m in n.plates_multiplier) for n in chain):
            no('plates_multiplier (mini-batches) goes through the generic engine')
            continue
        if any(getattr(n, '_shard_axis', None) is not None for n in chain):
            no('a plate is sharded over ranks')
            continue
        if not _takes_mask(Y):
            no('it has a mask of shape %s: the block takes no mask or a mask of the full shape of '
               'the plates of Y, here %s ((T,) for one chain, (B, T) for a batch); a mask per '
               'element, a scalar mask or one that broadcasts over a plate goes through the '
               'generic engine' % (_mask_shape(Y._mask), tuple(Y.plates)))
            continue
        bad = [(n, i) for n in (a0, A, mu, tau) for i in (0, 1)[:len(n.parents)]
               if not isinstance(n.parents[i], Constant)]
        if bad:
            no('a parameter of %s is a node (%s), not a constant'
               % (bad[0][0].name, type(bad[0][0].parents[bad[0][1]]).__name__))
            continue
        K, T = Z.categories, Z.states
        D = Y.dims[0][0]
        if A.plates != (K,):
            no('A has plates %s, not (K,): a time plate or chain plates on the transition '
               'probabilities go through the generic engine' % (A.plates,))
            continue
        if any(p != 1 for p in a0.plates):
            no('a0 has plates %s' % (a0.plates,))
            continue
        if T < 2:
            no('the chain has T = %d < 2 time instances' % T)
            continue
        if len(Z.plates) > 1 or Y.plates != Z.plates + (T,) or Y.cluster_plate != -1:
            no('it needs plates (T,) or (B, T), Y has plates %s and Z has plates %s'
               % (Y.plates, Z.plates))
            continue
        max_K, max_D = hmm_diag_limits()
        if K > max_K or D > max_D:
            no('D = %d, K = %d exceed the limits of the block (D <= %d, K <= %d)'
               % (D, K, max_D, max_K))
            continue
        if mu.plates != (K,) or mu.shape != (D,) or tau.plates != (K, D):
            no('plates of mu / tau are %s / %s with shape %s of mu, not (K,) / (K, D) with shape '
               '(D,)' % (mu.plates, tau.plates, mu.shape))
            continue
        if not all(_broadcasts(p, (K, D)) for n in (mu, tau) for p in n.parents):
            no('a prior of mu or tau does not broadcast to (K, D)')
            continue
        kids = ((a0, [Z]), (A, [Z]), (Z, [Zc]), (Zc, [Y]), (Y, []), (mu, [Y]), (tau, [Y]))
        if any([c for c, _ in n.children] != want for n, want in kids):
            no('one of its roles has other children as well')
            continue
        bad = [n for n in (a0, A, mu, tau) if n.observed]
        if bad:
            no('%s is observed' % bad[0].name)
            continue
        bad = [n for n in (a0, A, mu, tau) if n._init is not None]
        if bad:
            no('%s is initialised by %s' % (bad[0].name, bad[0]._init[0]))
            continue
        return dict(Y=Y, Z=Z, A=A, a0=a0, Zc=Zc, mu=mu, tau=tau)
    return None


class DiagGaussianHMMPlan(HMMPlan):
    """``HMMPlan`` with one precision per dimension.  Opt-in: ``VB(..., engine='fused+diagonal')``,
    tried right after the HMM block."""

    _KIND, _EMISSIONS = 'hmm_diag', 'diagonal-Gaussian'
    _DIMS = '(B, T, D, K)'

    @staticmethod
    def describe():
        return ("Mixture(CategoricalMarkovChain(Dirichlet(const), Dirichlet(const, plates=(K,)), "
                "states=T), GaussianARD, GaussianARD(const, const, shape=(D,), plates=(K,)), "
                "Gamma(const, const, plates=(K, D)), 1), plates (T,) or (B, T), observed without a "
                "mask or with a boolean mask of exactly that shape, T >= 2, D <= %d, K <= %d"
                % hmm_diag_limits()[::-1])

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why)

    def __init__(self, roles, runtime=None, kernels=None):
        super().__init__(roles, runtime, kernels)
        self.tau = roles['tau']

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = DiagHMMKernels(self.rt)
        return self._kernels

    # -- set-up ------------------------------------------------------------------------------------
    def _prior(self, node, i, positive, what):
        """A constant prior as the dense (D, K) table of ``vmp_dgmm_update``."""
        a = np.asarray(node.parents[i].value, dtype=np.float64)
        if positive and np.any(a <= 0):
            raise ValueError('%s of %s should be positive' % (what, node.name))
        a = np.ascontiguousarray(np.broadcast_to(a, (self.K, self.D)).T)
        return self.rt.torch.from_numpy(a).to(self.rt.device)

    def _materialize(self):
        if self._ready:
            if self._y_stale:
                self._upload_y()
                self._run_pass(refresh=False)
            return
        self._delta = _delta.delta_roles(self.roles)
        rt, k = self.rt, self.kernels
        B, T, D, K = self.B, self.T, self.D, self.K
        rt.sync_stream()
        self.chains_per_wg, wsd = k.plan(B, T, D, K)
        self._upload_y()
        self.m0, self.beta0 = self._prior(self.mu, 0, False, 'm0'), self._prior(self.mu, 1, True, 'beta0')
        self.pa0, self.pb0 = self._prior(self.tau, 0, True, 'a0'), self._prior(self.tau, 1, True, 'b0')
        self.mu_par, self.mu_mom = rt.empty(D * K, 2), rt.empty(D * K, 2)
        self.tau_par, self.tau_mom = rt.empty(D * K, 2), rt.empty(D * K, 2)
        # the tables of the last Z update, and those of the present moments for <log p(Y)>
        self.h, self.q, self.g = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
        self.h_now, self.q_now, self.g_now = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
        self.zeroK, self.c_tmp = rt.zeros(K), rt.zeros(K)   # vmp_dgmm_tables: <log pi> = 0, its c
        self.S1, self.S2, self.Nk = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
        self.bnd_e = rt.zeros(2)                            # bound terms of mu and tau
        self.yscal = rt.zeros(4)                            # S1 . h, S2 . q, Nk . g
        self.ws_dot = rt.empty(max(D * K, 1024))
        self.ws = rt.empty(int(wsd))
        self._init_chain_state()
        # mu and tau under their priors
        k.update(D, K, 0, self.m0, self.beta0, None, None, None, None, self.mu_par, self.mu_mom,
                 self.bnd_e[0:1])
        k.update(D, K, 1, self.pa0, self.pb0, None, None, None, None, self.tau_par, self.tau_mom,
                 self.bnd_e[1:2])
        self._with_emissions = False
        self._ready = True
        self._run_pass()

    def _launch_pass(self, gamma, z0, zz):
        h = self.h if self._with_emissions else None
        self.kernels.pass_(self.B, self.T, self.D, self.K, self.Yd, h, self.q, self.g,
                           self.used_a0, self.used_A, self.labels, self.maskd, self.ws, self.z0sum,
                           self.xisum, self.S1, self.S2, self.Nk, self.scal, gamma, z0, zz)

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        if node is not self.Z and node is not self.mu and node is not self.tau:
            return super().update(node)
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        k, D, K = self.kernels, self.D, self.K
        self.rt.sync_stream()
        if node is self.Z:
            self.labels = None
            self._with_emissions = True
            k.tables(D, K, self.mu_mom, self.tau_mom, self.zeroK, self.h, self.q, self.c_tmp, self.g)
            self._run_pass()
        elif node is self.mu:
            k.update(D, K, 0, self.m0, self.beta0, self.S1, self.S2, self.Nk, self.tau_mom,
                     self.mu_par, self.mu_mom, self.bnd_e[0:1])
        else:
            k.update(D, K, 1, self.pa0, self.pb0, self.S1, self.S2, self.Nk, self.mu_mom,
                     self.tau_par, self.tau_mom, self.bnd_e[1:2])
        self._version += 1

    def _n_observed(self):
        return self.B * self.T if self.maskd is None else int(self.maskd.sum().item())

    def _lower_bound_terms(self):
        self._materialize()
        if self._L_version != self._version:
            k, D, K = self.kernels, self.D, self.K
            self.rt.sync_stream()
            k.tables(D, K, self.mu_mom, self.tau_mom, self.zeroK, self.h_now, self.q_now,
                     self.c_tmp, self.g_now)
            k.dot(D * K, self.S1, self.h_now, self.ws_dot, self.yscal[0:1])
            k.dot(D * K, self.S2, self.q_now, self.ws_dot, self.yscal[1:2])
            k.dot(K, self.Nk, self.g_now, self.ws_dot, self.yscal[2:3])
            s, chain = self._chain_terms()
            ys, be = self.yscal.cpu().numpy(), self.bnd_e.cpu().numpy()
            t = dict(Y=float(ys[0] + ys[1] + ys[2])
                     - 0.5 * self._n_observed() * D * np.log(2 * np.pi),
                     mu=float(be[0]), tau=float(be[1]), **chain)
            t['total'] = sum(t.values())
            self._L = t
            self._L_version = self._version
        return _delta.bound_terms(self._L, self._delta)

    def lower_bound_contribution(self, node):
        if node is self.tau:
            return self._lower_bound_terms()['tau']
        return super().lower_bound_contribution(node)

    def get_moments(self, node):
        if node is self.mu or node is self.tau:
            self._materialize()
            D, K = self.D, self.K
            t = (self.mu_mom if node is self.mu else self.tau_mom).cpu().numpy().reshape(D, K, 2)
            u0, u1 = t[..., 0].T.copy(), t[..., 1].T.copy()
            if node is self.tau:
                return [u0, u1]
            # q(mu) factorises over d: <mu mu^T> = <mu><mu>^T + diag(<mu^2> - <mu>^2)
            uu = u0[:, :, None] * u0[:, None, :]
            i = np.arange(D)
            uu[:, i, i] = u1
            return [u0, uu]
        return super().get_moments(node)

    # -- persistence -----------------------------------------------------------------------------------
    def _dims(self):
        return (self.B, self.T, self.D, self.K)

    @property
    def _SAVED(self):
        return self._SAVED_BOTH + ('mu_par', 'mu_mom', 'tau_par', 'tau_mom', 'h', 'q', 'g', 'S1',
                                   'S2', 'Nk', 'bnd_e')
