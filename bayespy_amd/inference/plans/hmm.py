"""
Execution plan of the hidden-Markov-model block (doc/source/examples/hmm.rst, second half)

    a0 = Dirichlet(const (K,));  A = Dirichlet(const (K, K))
    Z  = CategoricalMarkovChain(a0, A, states=T)            plates () or (B,)
    Y  = Mixture(Z, Gaussian, mu, Lambda);  Y.observe(y)    plates (T,) or (B, T)

with (a) constant emission parameters ``mu`` (K, D) and ``Lambda`` (D, D) or (K, D, D), or (b)
``mu = GaussianARD(0, const, shape=(D,), plates=(K,))`` and ``Lambda = Wishart(const, const (D, D),
plates=(K,))`` -- the priors of the Gaussian-mixture block; constant priors, ``Y`` observed without
a mask or with a mask of the full shape of its plates (below), T >= 2, K <= 64 and D <= 8.  Opt-in: ``VB(..., engine='fused')``;
the default engine runs this model on the generic engine as before.  The plan owns, in HBM: ``y``
(B, T, D), the coefficient table ``C`` of the emission log-likelihoods (filled once from the
constants), the Dirichlet parameters and <log> tables of ``a0`` and ``A``, the tables the last
``Z`` update used, and the sums  sum_b gamma_{b,0} (K),  sum_{b,t} xi_{b,t} (K, K)  and
T_k = sum gamma [1, y, y y^T].  Nothing of size (B, T-1, K, K) exists: xi is formed inside
``vmp_hmm_fused_pass`` and only on request written out (``Z.get_moments()``); the forward state of
the pass is (B, T, K) in its workspace.

All plate terms of the lower bound follow from the sums:
    <log p(Y)>           = sum_k T_k . C_k
    <log p(Z)> + entropy = z0 . <log a0> + xi . <log A>
                           + sum_b log Z_b - sum gamma . e - (z0 . <log a0> + xi . <log A>)_used
where the last bracket is taken with the tables of the last ``Z`` update (the two brackets cancel
until ``a0`` or ``A`` is updated after ``Z``, which is the reference's order).

Form (b) keeps ``mu`` and ``Lambda`` in a ``vmp_gmm_layout`` state whose <log pi> slot stays zero:
``vmp_gmm_prepare_z`` fills its ``C`` table, the pass reads it in place and leaves ``T`` in the
state, ``vmp_gmm_update_mu`` / ``vmp_gmm_update_lambda`` update from ``T`` and
``vmp_gmm_lower_bound`` gives <log p(Y)> (with the present ``mu`` and ``Lambda``) and the terms of
``mu`` and ``Lambda``.  No kernel of the mixture block is copied.

Masks: ``Y.observe(y, mask=m)`` with a boolean host array or a ``DeviceMask`` of shape ``Y.plates``
exactly.  The mask is kept as ``uint8`` (B, T) in HBM and the pass becomes
``vmp_hmm_fused_pass_masked``: a masked step sends a zero message to ``Z`` but stays a step of the
chain, contributes nothing to ``T_k``, sum gamma . e or <log p(Y)>, and its ``y`` is never read (NaN
is fine there).  ``Z.mask[b]`` is "any step of chain b observed"; a chain without one contributes
nothing to sum gamma_0, sum xi, sum log Z or the entropy, so the formulas above hold unchanged on
the masked sums.  Deviation: the reference leaves the moments of such a chain at their initial
values; here ``Z.get_moments()`` returns for it what the recursion gives without any emission term.
A scalar mask or one that broadcasts over a plate is declined.
"""
import ctypes

import numpy as np

from . import _delta
from ._dirichlet import DirichletKernels, prior_table

from ... import _lib
from ...device import get_runtime, ptr
from ...nodes.node import Constant, DeviceMask
from ...nodes.dirichlet import Dirichlet
from ...nodes.gaussian import Gaussian, GaussianARD
from ...nodes.wishart import Wishart
from ...nodes.categorical_markov_chain import (CategoricalMarkovChain,
                                               CategoricalMarkovChainToCategorical)
from ...nodes.mixture import Mixture
from .gmm import GMMKernels

_LIMITS = []
_KINDS = {'hmm': 'Gaussian', 'hmm_cat': 'categorical'}      # checkpoint kind -> emission family


def hmm_limits():
    """(max K, max D) of the built pass: host-only ``vmp_hmm_fused_limits``."""
    if not _LIMITS:
        k, d = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_hmm_fused_limits(ctypes.byref(k), ctypes.byref(d)))
        _LIMITS.append((k.value, d.value))
    return _LIMITS[0]


def n_features(D):
    return D * (D + 1) // 2 + D + 1


def emission_tables(mu, Lam):
    """(C compact (K, NF), C natural (K, 1 + D + D^2)) of E[log N(y | mu_k, Lambda_k^-1)] for
    constant parameters: compact = coefficients of y_a y_b (a <= b), y_d, 1 (the order of
    ``vmp_gmm_prepare_z``); natural = coefficients of [1, y, y y^T] (the order of T)."""
    K, D = mu.shape
    Lam = np.broadcast_to(Lam, (K, D, D))
    C = np.zeros((K, n_features(D)))
    Cn = np.zeros((K, 1 + D + D * D))
    for k in range(K):
        L = Lam[k]
        sign, logdet = np.linalg.slogdet(L)
        if sign <= 0:
            raise np.linalg.LinAlgError("Matrix not positive definite")
        b = L @ mu[k]
        c = 0.5 * logdet - 0.5 * D * np.log(2 * np.pi) - 0.5 * float(mu[k] @ b)
        f = 0
        for a in range(D):
            for bb in range(a, D):
                C[k, f] = -0.5 * L[a, a] if a == bb else -0.5 * (L[a, bb] + L[bb, a])
                f += 1
        C[k, f:f + D] = b
        C[k, f + D] = c
        Cn[k, 0] = c
        Cn[k, 1:1 + D] = b
        Cn[k, 1 + D:] = (-0.5 * L).reshape(-1)
    return C, Cn


class HMMKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx
        self.gmm = GMMKernels(rt)            # form (b): the state and updates of mu and Lambda

    def plan(self, B, T, D, K):
        """(chains of a workgroup, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_hmm_fused_plan(B, T, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused hidden-Markov-model block supports T >= 2, '
                                      'K <= %d and D <= %d' % hmm_limits())
        return c.value, w.value

    def pass_(self, B, T, D, K, Y, C, ldc, elog_a0, elog_A, labels, ws, z0sum, xisum, Tstat, scal,
              gamma=None, z0=None, zz=None, mask=None):
        """``mask``: (B, T) uint8, 1 = observed; with one the pass is ``vmp_hmm_fused_pass_masked``."""
        def p(t):
            return ptr(t) if t is not None else None
        head = (self.ctx, B, T, D, K, p(Y), p(C), ldc, p(elog_a0), p(elog_A), p(labels))
        tail = (p(ws), p(z0sum), p(xisum), p(Tstat), p(scal), p(gamma), p(z0), p(zz))
        if mask is None:
            self.rt.check(self.lib.vmp_hmm_fused_pass(*head, *tail))
        else:
            self.rt.check(self.lib.vmp_hmm_fused_pass_masked(*head, ptr(mask), *tail))


def _mask_shape(mask):
    return tuple(mask.shape) if isinstance(mask, DeviceMask) else np.shape(mask)


def _takes_mask(Y):
    """No mask, or one of the full shape of the plates of ``Y``."""
    return Y._mask is True or _mask_shape(Y._mask) == tuple(Y.plates)


def _match(nodes, why):
    for Y in nodes:
        if not isinstance(Y, Mixture) or not isinstance(Y.parents[0],
                                                        CategoricalMarkovChainToCategorical):
            continue

        def no(msg, Y=Y):
            if why is not None:
                why.append('fused hidden-Markov-model block, observed node %s: %s'
                           % (Y.name or '<unnamed>', msg))
        if Y.node_class is not Gaussian:
            no('the mixed distribution is %s, not Gaussian'
               % getattr(Y.node_class, '__name__', Y.node_class))
            continue
        Zc = Y.parents[0]
        Z = Zc.parents[0]
        if type(Z) is not CategoricalMarkovChain or len(Y.parents) != 3:
            no('its parents are not (CategoricalMarkovChain, mu, Lambda)')
            continue
        a0, A = Z.parents
        mu, Lam = Y.parents[1], Y.parents[2]
        if type(a0) is not Dirichlet or type(A) is not Dirichlet:
            no('the initial-state and transition probabilities are not Dirichlet nodes')
            continue
        if not all(any(n is m for m in nodes) for n in (Y, Z, a0, A)):
            continue
        chain = (Y, Zc, Z, a0, A)
        if any(any(m != 1 for m in n.plates_multiplier) for n in chain):
            no('plates_multiplier (mini-batches) goes through the generic engine')
            continue
        if any(getattr(n, '_shard_axis', None) is not None for n in chain):
            no('a plate is sharded over ranks')
            continue
        if not _takes_mask(Y):
            no('it has a mask of shape %s: the block takes no mask or a mask of the full shape of '
               'the plates of Y, here %s ((T,) for one chain, (B, T) for a batch); a scalar mask '
               'or one that broadcasts over a plate goes through the generic engine'
               % (_mask_shape(Y._mask), tuple(Y.plates)))
            continue
        bad = [n for n in (a0, A) if not isinstance(n.parents[0], Constant)]
        if bad:
            no('the concentration of %s is a node (%s), not a constant'
               % (bad[0].name, type(bad[0].parents[0]).__name__))
            continue
        learned = type(mu) is GaussianARD and type(Lam) is Wishart
        if not learned and not (isinstance(mu, Constant) and isinstance(Lam, Constant)):
            no('mu is %s and Lambda is %s: the block takes two constants or '
               '(GaussianARD, Wishart) nodes' % (type(mu).__name__, type(Lam).__name__))
            continue
        if learned and not all(any(n is m for m in nodes) for n in (mu, Lam)):
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
        max_K, max_D = hmm_limits()
        if K > max_K or D > max_D:
            no('D = %d, K = %d exceed the limits of the block (D <= %d, K <= %d)'
               % (D, K, max_D, max_K))
            continue
        if learned:
            if any(any(m != 1 for m in n.plates_multiplier) for n in (mu, Lam)) \
                    or any(getattr(n, '_shard_axis', None) is not None for n in (mu, Lam)):
                no('mu or Lambda has a plates_multiplier or a sharded plate')
                continue
            if mu.plates != (K,) or Lam.plates != (K,) or mu.shape != (D,):
                no('plates of mu / Lambda are not (K,), (K,) with shape (D,)')
                continue
            m0, b0 = mu.parents
            if not (isinstance(m0, Constant) and not np.any(m0.value)
                    and isinstance(b0, Constant) and b0.is_scalar()):
                no('the prior of the means is not N(0, c I) with constants')
                continue
            n0, V0 = Lam.parents
            if not (isinstance(n0, Constant) and isinstance(V0, Constant) and n0.is_scalar()
                    and V0.value.shape == (D, D)):
                no('the Wishart prior is not (constant scalar degrees, one constant D x D scale)')
                continue
            if mu.observed or Lam.observed:
                no('mu or Lambda is observed')
                continue
            bad = [n for n in (mu, Lam) if n._init is not None]
            if bad:
                no('%s is initialised by %s' % (bad[0].name, bad[0]._init[0]))
                continue
        elif mu.value.shape != (K, D) or Lam.value.shape not in ((D, D), (K, D, D)):
            no('mu has shape %s and Lambda %s, not (K, D) and (D, D) or (K, D, D)'
               % (mu.value.shape, Lam.value.shape))
            continue
        kids = ((a0, [Z]), (A, [Z]), (Z, [Zc]), (Zc, [Y]), (Y, []))
        if learned:
            kids += ((mu, [Y]), (Lam, [Y]))
        if any([c for c, _ in n.children] != want for n, want in kids):
            no('one of its roles has other children as well')
            continue
        if a0.observed or A.observed:
            no('a0 or A is observed')
            continue
        bad = [n for n in (a0, A) if n._init is not None]
        if bad:
            no('%s is initialised by %s' % (bad[0].name, bad[0]._init[0]))
            continue
        roles = dict(Y=Y, Z=Z, A=A, a0=a0, Zc=Zc)
        if learned:
            roles.update(mu=mu, Lambda=Lam)
        return roles
    return None


class HMMPlan:

    @staticmethod
    def describe():
        return ("Mixture(CategoricalMarkovChain(Dirichlet(const), Dirichlet(const, plates=(K,)), "
                "states=T), Gaussian, mu, Lambda) with constant mu and Lambda or GaussianARD(0, const, "
                "shape=(D,), plates=(K,)) and Wishart(const, const, plates=(K,)), plates (T,) or "
                "(B, T), observed without a mask or with a boolean mask of exactly that shape "
                "(missing observations, ragged lengths), T >= 2, D <= %d, K <= %d" % (hmm_limits()[1], hmm_limits()[0]))

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why)

    def __init__(self, roles, runtime=None, kernels=None):
        self.roles = roles
        self.Y, self.Z = roles['Y'], roles['Z']
        self.Zc = roles['Zc']
        self.a0, self.A = self.Z.parents                # the roles, or constants (hmm_cat.py)
        self.mu, self.Lam = roles.get('mu'), roles.get('Lambda')
        self.learned = self.mu is not None
        self.K, self.T = self.Z.categories, self.Z.states
        self.D = self.Y.dims[0][0]
        self.B = int(np.prod(self.Z.plates, dtype=np.int64))
        self._rt, self._kernels = runtime, kernels
        self._ready = False
        self._y_stale = False
        self.maskd = None                # uint8 (B, T) in HBM, or None without a mask
        self._version = 0
        self._L_version = -1
        self._L = None
        for nd in roles.values():
            nd._plan = self

    @property
    def rt(self):
        if self._rt is None:
            self._rt = get_runtime()
        return self._rt

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = HMMKernels(self.rt)
        return self._kernels

    def nodes(self):
        return list(self.roles.values())

    def has_state(self):
        return bool(self._ready)

    def invalidate(self, node):
        if node is self.Y and node.observed and _takes_mask(node):
            # new observations of the same shape, with a mask of the full shape or none: y and the
            # mask are uploaded and the sums formed again, the posteriors stay
            self._y_stale = True
            self._version += 1
            return
        _delta.warn_state_discarded(self, node)
        self._ready = False
        self._version += 1
        if type(self).match([n for n in self.nodes() if n is not self.Zc]) is None:
            from .generic import GenericPlan
            GenericPlan([n for n in self.nodes() if n is not self.Zc])

    # -- set-up ------------------------------------------------------------------------------------
    def _upload_y(self):
        rt, torch = self.rt, self.rt.torch
        shape = (self.B, self.T, self.D)
        y = self.Y._data
        if y is None:
            raise ValueError('Node %s has not been observed' % self.Y.name)
        if isinstance(y, torch.Tensor):
            t = y.to(rt.device).to(torch.float64)
            t = t.expand(self.Y.plates + (self.D,)).reshape(shape).contiguous()
        else:
            a = np.broadcast_to(np.asarray(y, dtype=np.float64), self.Y.plates + (self.D,))
            t = torch.from_numpy(np.array(a.reshape(shape), order='C')).to(rt.device)
        self.Yd = t
        self._upload_mask()
        self._y_stale = False

    def _upload_mask(self):
        rt, torch = self.rt, self.rt.torch
        m = self.Y._mask
        if m is True:
            self.maskd = None
        elif isinstance(m, DeviceMask):
            self.maskd = m.tensor.to(rt.device).reshape(self.B, self.T).to(torch.uint8).contiguous()
        else:
            self.maskd = torch.from_numpy(np.ascontiguousarray(
                np.asarray(m, dtype=bool).reshape(self.B, self.T).astype(np.uint8))).to(rt.device)

    def _labels(self, lab):
        lab = np.asarray(lab)
        if lab.dtype.kind == 'f':
            if np.any(lab != np.round(lab)):
                raise ValueError("Values must be integers")
        elif lab.dtype.kind not in 'iub':
            raise ValueError("Values must be integers")
        lab = np.array(np.broadcast_to(lab, self.Z.plates + (self.T,)), dtype=np.int64)
        if lab.size and (lab.min() < 0 or lab.max() >= self.K):
            raise ValueError("Invalid category index")
        return self.rt.torch.from_numpy(
            np.ascontiguousarray(lab.reshape(self.B, self.T).astype(np.int32))).to(self.rt.device)

    def _materialize(self):
        if self._ready:
            if self._y_stale:
                self._upload_y()
                self._run_pass(refresh=False)
            return
        self._delta = _delta.delta_roles(self.roles)
        rt, k = self.rt, self.kernels
        torch = rt.torch
        B, T, D, K = self.B, self.T, self.D, self.K
        rt.sync_stream()
        self.chains_per_wg, wsd = k.plan(B, T, D, K)
        self._upload_y()
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(rt.device)  # noqa: E731
        self.FS = 1 + D + D * D
        if self.learned:
            # mu and Lambda from their priors in a vmp_gmm_layout state; its <log pi> slot stays
            # zero, so that vmp_gmm_prepare_z leaves the emission term alone in C
            self.layout = L = k.gmm.layout(D, K)
            self.state = rt.zeros(int(L.total))
            k.gmm.init_state(D, K, np.ones(K), self.mu.parents[1].scalar(),
                             self.Lam.parents[0].scalar(),
                             np.array(self.Lam.parents[1].value, dtype=np.float64), self.state)
            self.state[L.off_alpha + L.KP:L.off_alpha + 2 * L.KP].zero_()
            self.C, self.ldc = self.state[L.off_C:L.off_C + L.KP * L.F2P], int(L.F2P)
            self.Tstat = self.state[L.off_T:L.off_T + K * self.FS].view(K, self.FS)
        else:
            C, Cn = emission_tables(np.asarray(self.Y.parents[1].value, dtype=np.float64),
                                    np.asarray(self.Y.parents[2].value, dtype=np.float64))
            self.C, self.Cn, self.ldc = up(C), up(Cn), C.shape[1]
            self.Tstat = rt.zeros(K, self.FS)
        self.ws = rt.empty(int(wsd))
        self._init_chain_state()
        self._with_emissions = False
        self._ready = True
        self._run_pass()

    def _init_chain_state(self):
        """The tables of ``a0`` and ``A``, the sums of the chain and the initial state of ``Z``
        (fixed labels, or its moments under the prior).  A role that is a constant (hmm_cat.py)
        has the logarithm of its value as its table, uploaded once, no update and no bound term."""
        rt, k, K, T = self.rt, self.kernels, self.K, self.T
        torch = rt.torch
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(rt.device)  # noqa: E731
        self.alpha_a0, self.alpha_A = rt.zeros(K), rt.zeros(K, K)
        self.used_a0, self.used_A = rt.empty(K), rt.empty(K, K)
        self.z0sum, self.xisum = rt.zeros(K), rt.zeros(K, K)
        self.ws_small = rt.empty(max(K * K, 1024))
        # [0] sum log Z, [1] sum gamma . e, [2] z0 . <log a0> used, [3] xi . <log A> used,
        # [4] T . C, [5] z0 . <log a0>, [6] xi . <log A>
        self.scal = rt.zeros(8)
        self.bnd = rt.zeros(2)                          # bound terms of a0 and A
        if isinstance(self.a0, Constant):
            self.elog_a0 = up(np.log(np.broadcast_to(self.a0.value, (K,))))
        else:
            self.prior_a0, self.elog_a0 = up(prior_table(self.a0, (K,))), rt.empty(K)
            k.dirichlet(1, K, K, 1, self.prior_a0, None, self.alpha_a0, self.elog_a0,
                        self.ws_small, self.bnd[0:1])
        if isinstance(self.A, Constant):
            self.elog_A = up(np.log(np.broadcast_to(self.A.value, (K, K))))
        else:
            self.prior_A, self.elog_A = up(prior_table(self.A, (K, K))), rt.empty(K, K)
            k.dirichlet(K, K, K, 1, self.prior_A, None, self.alpha_A, self.elog_A, self.ws_small,
                        self.bnd[1:2])
        # Z: fixed labels, or its moments under the prior (no emission term)
        self.labels = None
        init = self.Z._init
        if init is not None:
            if init[0] == 'value':
                self.labels = self._labels(init[1])
            elif init[0] == 'random':
                self.labels = self._labels(np.random.randint(K, size=self.Z.plates + (T,)))
            else:
                raise NotImplementedError('the fused hidden-Markov-model block initialises Z '
                                          'from its prior, a value or at random')

    def _run_pass(self, gamma=None, z0=None, zz=None, refresh=True):
        """The sums of the present ``Z`` state (the tables of its last update, or labels).
        ``refresh``: take the current <log a0> and <log A> as the tables of the pass."""
        if refresh:
            self._refresh_tables()
        self._launch_pass(gamma, z0, zz)
        if refresh or gamma is None:
            self._version += 1              # writing gamma / z0 / zz out changes no sum

    def _refresh_tables(self):
        self.used_a0.copy_(self.elog_a0)
        self.used_A.copy_(self.elog_A)

    def _launch_pass(self, gamma, z0, zz):
        C = self.C if self._with_emissions else None
        self.kernels.pass_(self.B, self.T, self.D, self.K, self.Yd, C, self.ldc, self.used_a0,
                           self.used_A, self.labels, self.ws, self.z0sum, self.xisum, self.Tstat,
                           self.scal, gamma, z0, zz, mask=self.maskd)

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        rt, k = self.rt, self.kernels
        rt.sync_stream()
        K = self.K
        if node is self.Z:
            self.labels = None
            self._with_emissions = True
            if self.learned:
                k.gmm.prepare_z(self.D, K, False, self.state)
            self._run_pass()
        elif self.learned and node is self.mu:
            k.gmm.update_mu(self.D, K, self.state)
        elif self.learned and node is self.Lam:
            k.gmm.update_lambda(self.D, K, self.state)
        elif node is self.a0 and not isinstance(node, Constant):
            k.dirichlet(1, K, K, 1, self.prior_a0, self.z0sum, self.alpha_a0, self.elog_a0,
                        self.ws_small, self.bnd[0:1])
        elif node is self.A and not isinstance(node, Constant):
            k.dirichlet(K, K, K, 1, self.prior_A, self.xisum, self.alpha_A, self.elog_A,
                        self.ws_small, self.bnd[1:2])
        else:
            return
        self._version += 1

    def _lower_bound_terms(self):
        self._materialize()
        if self._L_version != self._version:
            rt, k, K = self.rt, self.kernels, self.K
            rt.sync_stream()
            extra = {}
            if self.learned:
                L = self.layout
                k.gmm.lower_bound(self.D, K, self.state)
                host = self.state[L.off_scal:L.off_L + 8].cpu().numpy()
                if int(host[3]) != 0:
                    _lib.raise_for_status(int(host[3]))
                LY = float(host[8])
                extra = dict(mu=float(host[8 + 3]), Lambda=float(host[8 + 4]))
            else:
                k.dot(K * self.FS, self.Tstat, self.Cn, self.ws_small, self.scal[4:5])
            s, chain = self._chain_terms()
            t = dict(Y=LY if self.learned else float(s[4]), **chain, **extra)
            t['total'] = sum(t.values())
            self._L = t
            self._L_version = self._version
        return _delta.bound_terms(self._L, self._delta)

    def _chain_terms(self):
        """(scal on the host, the bound terms of Z, a0 and A) by the formula of the module's
        docstring; whatever the caller wants in scal[4] is launched before."""
        k, K = self.kernels, self.K
        k.dot(K, self.z0sum, self.elog_a0, self.ws_small, self.scal[5:6])
        k.dot(K * K, self.xisum, self.elog_A, self.ws_small, self.scal[6:7])
        s = self.scal.cpu().numpy()
        b = self.bnd.cpu().numpy()
        entropy = 0.0 if self.labels is not None else float(s[0] - s[1] - (s[2] + s[3]))
        return s, dict(Z=float(s[5] + s[6]) + entropy, a0=float(b[0]), A=float(b[1]))

    def lower_bound_contribution(self, node):
        terms = self._lower_bound_terms()
        for key in ('Y', 'Z', 'a0', 'A', 'mu', 'Lambda', 'P'):
            if node is self.roles.get(key):
                return terms[key]
        return 0.0

    def posterior(self, pairs=True):
        """(gamma (B, T, K), z0 (B, K), zz (B, T-1, K, K) or None without ``pairs``) of ``Z`` as
        device arrays: written by the pass from the tables of the last ``Z`` update; not kept."""
        self._materialize()
        rt = self.rt
        rt.sync_stream()
        B, T, K = self.B, self.T, self.K
        gamma, z0 = rt.empty(B, T, K), rt.empty(B, K)
        zz = rt.empty(B, T - 1, K, K) if pairs else None
        if B:
            self._run_pass(gamma, z0, zz, refresh=False)
        return gamma, z0, zz

    def _blk(self, off, shape):
        n = int(np.prod(shape))
        return self.state[off:off + n].cpu().numpy().reshape(shape).copy()

    def get_moments(self, node):
        self._materialize()
        K, T = self.K, self.T
        if node is self.a0:
            return [self.elog_a0.cpu().numpy().reshape(self.a0.plates + (K,)).copy()]
        if node is self.A:
            return [self.elog_A.cpu().numpy().reshape(K, K).copy()]
        if node is self.Z:
            _, z0, zz = self.posterior()
            return [z0.cpu().numpy().reshape(self.Z.plates + (K,)),
                    zz.cpu().numpy().reshape(self.Z.plates + (T - 1, K, K))]
        if node is self.Zc:
            return [self.posterior(pairs=False)[0].cpu().numpy().reshape(self.Z.plates + (T, K))]
        if self.learned and node is self.mu:
            L, D = self.layout, self.D
            m = self._blk(L.off_mu, (K, D))
            return [m, self._blk(L.off_Cmu, (K, D, D)) + m[:, :, None] * m[:, None, :]]
        if self.learned and node is self.Lam:
            L, D = self.layout, self.D
            return [self._blk(L.off_Lam, (K, D, D)), self._blk(L.off_logdetLam, (K,))]
        if node is self.Y:
            y = self.Yd.cpu().numpy().reshape(self.Y.plates + (self.D,))
            return [y, y[..., :, None] * y[..., None, :]]
        raise NotImplementedError

    def _host_mask(self):
        """The mask as a boolean host array of shape ``Y.plates``, or None without one."""
        m = self.Y._mask
        return None if m is True else np.asarray(m, dtype=bool).reshape(self.Y.plates)

    def get_mask(self, node):
        """``Y``: its mask; ``Z``: any step of the chain observed; every other node: True."""
        m = self._host_mask()
        if m is None:
            return np.array(True)
        if node is self.Y or node is self.Zc:
            return m.copy()
        if node is self.Z:
            return np.asarray(m.any(axis=-1))
        return np.array(True)

    # -- persistence -----------------------------------------------------------------------------------
    _KIND, _EMISSIONS = 'hmm', 'Gaussian'
    _DIMS = '(B, T, D, K, learned emissions)'

    def _dims(self):
        return (self.B, self.T, self.D, self.K, int(self.learned))

    _SAVED_BOTH = ('alpha_a0', 'elog_a0', 'alpha_A', 'elog_A', 'used_a0', 'used_A', 'z0sum',
                   'xisum', 'scal', 'bnd')

    @property
    def _SAVED(self):
        # form (b): T, C, mu and Lambda are parts of the state
        return self._SAVED_BOTH + (('state',) if self.learned else ('Tstat',))

    def save_state(self, put, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        _delta.save(put, base, self._delta)
        put(base + 'kind', np.array([ord(ch) for ch in self._KIND], dtype=np.uint8))
        put(base + 'dims', np.array(self._dims(), dtype=np.int64))
        put(base + 'flags', np.array([1 if self.labels is not None else 0,
                                      1 if self._with_emissions else 0], dtype=np.int64))
        if self.labels is not None:
            put(base + 'labels', self.labels.cpu().numpy())
        if self.maskd is not None:
            put(base + 'mask', self.maskd.cpu().numpy())
        for name in self._SAVED:
            put(base + name, getattr(self, name).cpu().numpy())

    def load_state(self, reader, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        kind = bytes(np.asarray(reader.get(base + 'kind'), dtype=np.uint8)).decode() \
            if reader.has(base + 'kind') else None
        if kind != self._KIND:
            raise Exception("File does not contain the state of the fused hidden-Markov-model "
                            "block with %s emissions%s"
                            % (self._EMISSIONS, '' if kind not in _KINDS else
                               ': it holds that of the block with %s emissions' % _KINDS[kind]))
        dims = tuple(int(v) for v in reader.get(base + 'dims'))
        if dims != self._dims():
            raise ValueError('checkpoint is for %s = %s, the model has %s'
                             % (self._DIMS, dims, self._dims()))
        saved = np.asarray(reader.get(base + 'mask'), dtype=np.uint8).reshape(-1) \
            if reader.has(base + 'mask') else None
        mine = None if self.maskd is None else self.maskd.cpu().numpy().reshape(-1)
        if (saved is None) != (mine is None) or (saved is not None
                                                 and not np.array_equal(saved != 0, mine != 0)):
            raise ValueError('checkpoint was saved with %s, the model has %s: observe Y with the '
                             'mask of the checkpoint before loading it'
                             % tuple('no mask on Y' if m is None else
                                     'a mask on Y with %d of %d steps observed'
                                     % (int(np.count_nonzero(m)), m.size) for m in (saved, mine)))
        torch = self.rt.torch
        self._delta = _delta.load(reader, base)
        flags = np.asarray(reader.get(base + 'flags')).ravel()
        if int(flags[0]):
            self.labels = torch.from_numpy(
                np.array(reader.get(base + 'labels'), dtype=np.int32)).to(self.rt.device)
        else:
            self.labels = None
        self._with_emissions = bool(int(flags[1]))
        for name in self._SAVED:
            getattr(self, name).copy_(torch.from_numpy(
                np.array(reader.get(base + name), dtype=np.float64)).reshape(
                    getattr(self, name).shape).to(self.rt.device))
        self._version += 1
