"""
Execution plan of the Gaussian-mixture block with one precision per dimension

    alpha = Dirichlet(const);  Z = Categorical(alpha, plates=(N, 1))
    mu = GaussianARD(const m0, const beta0, plates=(D, K))
    tau = Gamma(const a0, const b0, plates=(D, K))
    Y = Mixture(Z, GaussianARD, mu, tau);  Y.observe(y)                  y (N, D)

with constant priors (anything that broadcasts to (D, K)), K <= 64 and D <= 1024, ``Y`` fully
observed.  Opt-in: ``VB(..., engine='fused')``; the default engine runs this model on the generic
engine as before.  The plan owns, in HBM: ``y``, the parameters and moments of ``mu`` and ``tau``
as (D K, 2) tables, those of ``alpha`` (K), the tables h = <tau><mu>, q = -1/2 <tau> and
c = <log pi> + sum_d (1/2 <log tau> - 1/2 <tau><mu^2>) the last ``Z`` update used, and the
statistics N_k = sum_n r_nk, S1_dk = sum_n r_nk y_nd, S2_dk = sum_n r_nk y_nd^2.  Nothing of size
(N, D, K) or (N, K) exists: the responsibilities of ``Z`` are formed inside ``vmp_dgmm_pass`` and
only on request written out (``Z.get_moments()``).

All plate terms of the lower bound follow from the statistics, sum_n lse_n and the tables, with
g = sum_d (1/2 <log tau> - 1/2 <tau><mu^2>) of the PRESENT moments:
    <log p(Y)>           = S1 . h + S2 . q + N_k . g - 1/2 N D log 2 pi       (present moments)
    <log p(Z)> + entropy = N_k . <log pi>
                           + sum_n lse_n - N_k . c_used - (S1 . h_used + S2 . q_used)
The bound terms of ``mu`` and ``tau`` come from ``vmp_dgmm_update``, that of ``alpha`` from the
Dirichlet kernel.  Masks, mini-batches and sharded plates are declined (generic engine); a mask of
the full shape (N, D) is taken by the subclass of dgmm_masked.py, to which an unobserved model
goes over when ``Y`` is observed with such a mask.

Checkpoints: the block writes its own ``plans/<i>/`` group (kind 'dgmm') like every fused plan.
"""
import ctypes

import numpy as np

from . import _delta
from ._dirichlet import DirichletKernels, prior_table
from .bmm import _mask_shape

from ... import _lib
from ...device import get_runtime, ptr
from ...nodes.node import Constant
from ...nodes.dirichlet import Dirichlet
from ...nodes.categorical import Categorical
from ...nodes.gaussian import GaussianARD
from ...nodes.gamma import Gamma
from ...nodes.mixture import Mixture

_LIMITS = []


def dgmm_limits():
    """(max K, max D) of the built pass: host-only ``vmp_dgmm_limits``."""
    if not _LIMITS:
        k, d = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_dgmm_limits(ctypes.byref(k), ctypes.byref(d)))
        _LIMITS.append((k.value, d.value))
    return _LIMITS[0]


def _p(t):
    return ptr(t) if t is not None else None


class DGMMKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def plan(self, N, D, K):
        """(rows of a chunk, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_dgmm_plan(N, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused diagonal-Gaussian-mixture block supports K <= %d '
                                      'and D <= %d' % dgmm_limits())
        return c.value, w.value

    def tables(self, D, K, mu_mom, tau_mom, elog_pi, h, q, c, gsum=None):
        self.rt.check(self.lib.vmp_dgmm_tables(self.ctx, D, K, _p(mu_mom), _p(tau_mom),
                                               _p(elog_pi), _p(h), _p(q), _p(c), _p(gsum)))

    def pass_(self, N, D, K, y, labels, h, q, c, ws, S1, S2, Nk, scal, r_out=None):
        self.rt.check(self.lib.vmp_dgmm_pass(self.ctx, N, D, K, _p(y), _p(labels), _p(h), _p(q),
                                             _p(c), _p(ws), _p(S1), _p(S2), _p(Nk), _p(scal),
                                             _p(r_out)))

    def update(self, D, K, which, prior_a, prior_b, S1, S2, Nk, other, par, mom, bound):
        self.rt.check(self.lib.vmp_dgmm_update(self.ctx, D, K, which, _p(prior_a), _p(prior_b),
                                               _p(S1), _p(S2), _p(Nk), _p(other), _p(par), _p(mom),
                                               _p(bound)))


def _match(nodes, why, masked=False):
    """``masked``: the matcher of the block with missing observations (dgmm_masked.py), which takes
    a mask of the full shape of the plates of Y where this block takes none."""
    for Y in nodes:
        if not isinstance(Y, Mixture) or Y.node_class is not GaussianARD:
            continue

        def no(msg, Y=Y):
            if why is not None:
                why.append('fused diagonal-Gaussian-mixture block, observed node %s: %s'
                           % (Y.name or '<unnamed>', msg))
        if len(Y.parents) != 3:
            no('the mixed GaussianARD has further constructor arguments')
            continue
        Z, mu, tau = Y.parents
        if type(Z) is not Categorical or type(mu) is not GaussianARD or type(tau) is not Gamma \
                or type(Z.parents[0]) is not Dirichlet:
            no('its parents are not (Categorical(Dirichlet), GaussianARD, Gamma)')
            continue
        alpha = Z.parents[0]
        five = (Y, Z, mu, tau, alpha)
        if not all(any(n is m for m in nodes) for n in five):
            continue
        if any(any(m != 1 for m in n.plates_multiplier) for n in five):
            no('plates_multiplier (mini-batches) goes through the generic engine')
            continue
        if any(getattr(n, '_shard_axis', None) is not None for n in five):
            no('a plate is sharded over ranks')
            continue
        if not masked and Y._mask is not True:
            no('it has a mask: the block takes fully observed data only; a mask goes through the '
               'generic engine')
            continue
        if masked and Y._mask is True:
            continue                    # no mask: the model of the block without one, no reason
        if masked and _mask_shape(Y._mask) != tuple(Y.plates):
            no('it has a mask of shape %s: the block with missing observations takes a mask of '
               'the full shape of the plates of Y, here %s; a scalar mask or one that broadcasts '
               'over a plate goes through the generic engine'
               % (_mask_shape(Y._mask), tuple(Y.plates)))
            continue
        bad = [(n, p) for n in (mu, tau, alpha) for p in n.parents if not isinstance(p, Constant)]
        if bad:
            no('a parameter of %s is a node (%s), not a constant'
               % (bad[0][0].name, type(bad[0][1]).__name__))
            continue
        if Y.cluster_plate != -1:
            no('cluster_plate is %d, the block needs the clusters on the last plate axis (-1)'
               % Y.cluster_plate)
            continue
        if len(Y.plates) != 2 or len(mu.plates) != 2 or mu.ndim != 0 or Y.ndim != 0:
            no('it needs plates (N, D) and scalar GaussianARD variables, Y has plates %s and mu has '
               'plates %s and shape %s' % (Y.plates, mu.plates, mu.shape))
            continue
        N, D = Y.plates
        K = Y.clusters
        if Z.plates != (N, 1) or mu.plates != (D, K) or tau.plates != (D, K) \
                or any(p != 1 for p in alpha.plates):
            no('plates of Z / mu / tau / alpha are %s / %s / %s / %s, not (N, 1) / (D, K) / (D, K) '
               '/ ()' % (Z.plates, mu.plates, tau.plates, alpha.plates))
            continue
        if masked:
            from .dgmm_masked import dgmm_masked_limits
            max_k, max_d = dgmm_masked_limits()
        else:
            max_k, max_d = dgmm_limits()
        if K > max_k or D > max_d:
            no('D = %d, K = %d exceed the limits of the block%s (D <= %d, K <= %d)'
               % (D, K, ' with a mask' if masked else '', max_d, max_k))
            continue
        kids = ((alpha, [Z]), (Z, [Y]), (mu, [Y]), (tau, [Y]), (Y, []))
        if any([c for c, _ in n.children] != want for n, want in kids):
            no('one of its roles has other children as well')
            continue
        if Z.observed or mu.observed or tau.observed or alpha.observed:
            no('Z, mu, tau or alpha is observed')
            continue
        inits = ((Z, 'Z', ('value',)), (mu, 'mu', ('value', 'parameters')),
                 (tau, 'tau', ('parameters',)), (alpha, 'alpha', ('parameters',)))
        bad = [(nm, n._init[0]) for n, nm, ok in inits if n._init is not None and n._init[0] not in ok]
        if bad:
            no('%s is initialised by %s' % bad[0])
            continue
        return dict(Y=Y, Z=Z, mu=mu, tau=tau, alpha=alpha)
    return None


class DiagGaussianMixturePlan:

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates=(N, 1)), GaussianARD, "
                "GaussianARD(const, const, plates=(D, K)), Gamma(const, const, plates=(D, K))), "
                "fully observed (D <= %d, K <= %d)" % dgmm_limits()[::-1])

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why)

    def __init__(self, roles, runtime=None, kernels=None):
        self.roles = roles
        self.Y, self.Z, self.mu, self.tau, self.alpha = (roles[k] for k in
                                                         ('Y', 'Z', 'mu', 'tau', 'alpha'))
        self.N, self.D = self.Y.plates
        self.K = self.Y.clusters
        self._rt, self._kernels = runtime, kernels
        self._ready = False
        self._y_stale = False
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
            self._kernels = DGMMKernels(self.rt)
        return self._kernels

    def nodes(self):
        return list(self.roles.values())

    def has_state(self):
        return bool(self._ready)

    def invalidate(self, node):
        if node is self.Y and node.observed and node._mask is True:
            # new observations of the same shape: y is uploaded again, the posteriors stay
            self._y_stale = True
            self._version += 1
            return
        _delta.warn_state_discarded(self, node)
        self._ready = False
        self._version += 1
        if DiagGaussianMixturePlan.match(self.nodes()) is None:
            from .dgmm_masked import MaskedDiagGaussianMixturePlan
            if MaskedDiagGaussianMixturePlan.match(self.nodes()) is not None:
                # Y was observed with a mask of its full shape: the block for missing observations
                MaskedDiagGaussianMixturePlan(self.roles, runtime=self._rt)
                return
            from .generic import GenericPlan
            GenericPlan(self.nodes())

    # -- set-up ------------------------------------------------------------------------------------
    def _upload_y(self):
        rt, torch = self.rt, self.rt.torch
        N, D = self.N, self.D
        y = self.Y._data
        if y is None:
            raise ValueError('Node %s has not been observed' % self.Y.name)
        if isinstance(y, torch.Tensor):
            t = y.to(rt.device).to(torch.float64)
        else:
            t = torch.from_numpy(np.array(np.broadcast_to(np.asarray(y, dtype=np.float64), (N, D)),
                                          order='C')).to(rt.device)
        if tuple(t.shape) != (N, D) or not t.is_contiguous():
            t = t.expand(N, D).contiguous()
        self.y = t
        self._y_stale = False

    def _up(self, a):
        torch = self.rt.torch
        return torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(self.rt.device)

    def _const(self, node, i, positive, what):
        a = np.asarray(node.parents[i].value, dtype=np.float64)
        if positive and np.any(a <= 0):
            raise ValueError('%s of %s should be positive' % (what, node.name))
        return np.ascontiguousarray(np.broadcast_to(a, (self.D, self.K)))

    def _materialize(self):
        if self._ready:
            if self._y_stale:
                self._upload_y()
                self._run_pass()
            return
        self._delta = _delta.delta_roles(self.roles)
        rt, k = self.rt, self.kernels
        torch = rt.torch
        N, D, K = self.N, self.D, self.K
        rt.sync_stream()
        self.chunk, wsd = self._plan_pass()
        self._upload_y()
        m0, beta0 = self._const(self.mu, 0, False, 'm0'), self._const(self.mu, 1, True, 'beta0')
        a0, b0 = self._const(self.tau, 0, True, 'a0'), self._const(self.tau, 1, True, 'b0')
        pr = prior_table(self.alpha, (K,))
        self.m0, self.beta0, self.a0, self.b0 = (self._up(a) for a in (m0, beta0, a0, b0))
        self.prior_r = self._up(pr)
        self.mu_par, self.mu_mom = rt.empty(D * K, 2), rt.empty(D * K, 2)
        self.tau_par, self.tau_mom = rt.empty(D * K, 2), rt.empty(D * K, 2)
        self.alpha_r, self.elog_r = rt.empty(K), rt.empty(K)
        self.h, self.q, self.c = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
        self.h_now, self.q_now, self.c_now = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
        self.gsum = rt.zeros(K)
        self.S1, self.S2, self.Nk = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(K)
        self._alloc_more()
        self.ws = rt.empty(int(wsd))
        self.ws_small = rt.empty(max(D * K, 1024))
        # [0] sum lse, [1] N_k . c used, [2] S1 . h + S2 . q used, [3] bound of mu, [4] of tau,
        # [5] of alpha, [6] S1 . h, [7] S2 . q, [8] N_k . g (present moments), [9] N_k . <log pi>
        self.scal = rt.zeros(12)
        # the priors; a given initial state replaces them below
        k.update(D, K, 0, self.m0, self.beta0, None, None, None, None, self.mu_par, self.mu_mom,
                 self.scal[3:4])
        k.update(D, K, 1, self.a0, self.b0, None, None, None, None, self.tau_par, self.tau_mom,
                 self.scal[4:5])
        self._init_mu(m0, beta0)
        self._init_tau(a0, b0)
        counts = None
        init = self.alpha._init
        if init is not None:
            a = np.asarray(init[1][0], dtype=np.float64)
            if np.any(a <= 0):
                raise ValueError("Natural parameters should be positive")
            counts = self._up(np.broadcast_to(a, (K,)) - pr)
        k.dirichlet(1, K, K, 1, self.prior_r, counts, self.alpha_r, self.elog_r, self.ws_small,
                    self.scal[5:6])
        # Z: fixed labels, or its moments under the prior (no observation term)
        self.labels = None
        init = self.Z._init
        if init is not None:
            lab = np.asarray(init[1])
            if lab.dtype.kind == 'f':
                if np.any(lab != np.round(lab)):
                    raise ValueError("Values must be integers")
            elif lab.dtype.kind not in 'iub':
                raise ValueError("Values must be integers")
            lab = np.array(np.broadcast_to(lab, (N, 1)), dtype=np.int64).reshape(N)
            if lab.size and (lab.min() < 0 or lab.max() >= K):
                raise ValueError("Invalid category index")
            self.labels = torch.from_numpy(lab.astype(np.int32)).to(rt.device)
        self._tables(None, None)
        self._ready = True
        self._run_pass()

    def _init_mu(self, m0, beta0):
        """A given initial state of ``mu`` (host, set-up): a point mass, or N(m, 1 / lambda)."""
        init = self.mu._init
        if init is None:
            return
        D, K = self.D, self.K
        if init[0] == 'value':
            v = np.broadcast_to(np.asarray(init[1], dtype=np.float64), (D, K))
            self.mu_mom.copy_(self._up(np.stack([v, v * v], -1).reshape(D * K, 2)))
            self.mu_par.fill_(float('nan'))              # a point mass has no parameters
            return
        m, lam = (np.broadcast_to(np.asarray(a, dtype=np.float64), (D, K)) for a in init[1][:2])
        if np.any(lam <= 0):
            raise ValueError('the precision given to %s should be positive' % self.mu.name)
        self.mu_par.copy_(self._up(np.stack([m, lam], -1).reshape(D * K, 2)))
        self.mu_mom.copy_(self._up(np.stack([m, m * m + 1 / lam], -1).reshape(D * K, 2)))
        bound = 0.5 * (np.log(beta0) - np.log(lam)) - 0.5 * beta0 * ((m - m0) ** 2 + 1 / lam) + 0.5
        self.scal[3:4].copy_(self._up([bound.sum()]))

    def _init_tau(self, a0, b0):
        """A given initial state of ``tau`` (host, set-up): Gamma(a, b)."""
        init = self.tau._init
        if init is None:
            return
        from scipy.special import digamma, gammaln
        D, K = self.D, self.K
        a, b = (np.broadcast_to(np.asarray(v, dtype=np.float64), (D, K)) for v in init[1][:2])
        if np.any(a <= 0) or np.any(b <= 0):
            raise ValueError('the parameters given to %s should be positive' % self.tau.name)
        self.tau_par.copy_(self._up(np.stack([a, b], -1).reshape(D * K, 2)))
        self.tau_mom.copy_(self._up(np.stack([a / b, digamma(a) - np.log(b)],
                                             -1).reshape(D * K, 2)))
        bound = a0 * (np.log(b0) - np.log(b)) - gammaln(a0) + gammaln(a) + (a0 - a) * digamma(a) \
            + a - b0 * a / b
        self.scal[4:5].copy_(self._up([bound.sum()]))

    # where the block with missing observations (dgmm_masked.py) goes another way
    def _plan_pass(self):
        return self.kernels.plan(self.N, self.D, self.K)

    def _alloc_more(self):
        pass

    def _tables(self, mu_mom, tau_mom):
        """The tables of the pass from the given moments (None: no observation term)."""
        self.kernels.tables(self.D, self.K, mu_mom, tau_mom, self.elog_r, self.h, self.q, self.c)

    def _update_from_statistics(self, which, prior_a, prior_b, other, par, mom, bound):
        self.kernels.update(self.D, self.K, which, prior_a, prior_b, self.S1, self.S2, self.Nk,
                            other, par, mom, bound)

    def _run_pass(self, r_out=None):
        """The statistics of the present ``Z`` state (tables ``h`` / ``q`` / ``c`` or labels)."""
        self.kernels.pass_(self.N, self.D, self.K, self.y, self.labels, self.h, self.q, self.c,
                           self.ws, self.S1, self.S2, self.Nk, self.scal, r_out)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        rt, k = self.rt, self.kernels
        rt.sync_stream()
        K = self.K
        if node is self.Z:
            self.labels = None
            self._tables(self.mu_mom, self.tau_mom)
            self._run_pass()
        elif node is self.mu:
            self._update_from_statistics(0, self.m0, self.beta0, self.tau_mom, self.mu_par,
                                         self.mu_mom, self.scal[3:4])
        elif node is self.tau:
            self._update_from_statistics(1, self.a0, self.b0, self.mu_mom, self.tau_par,
                                         self.tau_mom, self.scal[4:5])
        elif node is self.alpha:
            k.dirichlet(1, K, K, 1, self.prior_r, self.Nk, self.alpha_r, self.elog_r,
                        self.ws_small, self.scal[5:6])
        else:
            return
        self._version += 1

    def _lower_bound_terms(self):
        self._materialize()
        if self._L_version != self._version:
            rt, k = self.rt, self.kernels
            rt.sync_stream()
            D, K = self.D, self.K
            k.tables(D, K, self.mu_mom, self.tau_mom, self.elog_r, self.h_now, self.q_now,
                     self.c_now, self.gsum)
            k.dot(D * K, self.S1, self.h_now, self.ws_small, self.scal[6:7])
            k.dot(D * K, self.S2, self.q_now, self.ws_small, self.scal[7:8])
            k.dot(K, self.Nk, self.gsum, self.ws_small, self.scal[8:9])
            k.dot(K, self.Nk, self.elog_r, self.ws_small, self.scal[9:10])
            s = self.scal.cpu().numpy()
            entropy = 0.0 if self.labels is not None else float(s[0] - s[1] - s[2])
            t = dict(Y=float(s[6] + s[7] + s[8]) - 0.5 * self.N * D * np.log(2 * np.pi),
                     Z=float(s[9]) + entropy, mu=float(s[3]), tau=float(s[4]), alpha=float(s[5]))
            t['total'] = t['Y'] + t['Z'] + t['mu'] + t['tau'] + t['alpha']
            self._L = t
            self._L_version = self._version
        return _delta.bound_terms(self._L, self._delta)

    def lower_bound_contribution(self, node):
        terms = self._lower_bound_terms()
        for key in ('Y', 'Z', 'mu', 'tau', 'alpha'):
            if node is self.roles[key]:
                return terms[key]
        return 0.0

    def responsibilities(self):
        """(N, K) responsibilities of ``Z`` as a device array: formed by the pass in its write mode
        from the tables of the last ``Z`` update; not kept."""
        self._materialize()
        rt = self.rt
        rt.sync_stream()
        r = rt.empty(self.N, self.K)
        if self.N:
            self._run_pass(r)
        return r

    def get_moments(self, node):
        self._materialize()
        D, K = self.D, self.K
        if node is self.alpha:
            return [self.elog_r.cpu().numpy().reshape(self.alpha.plates + (K,)).copy()]
        if node is self.mu or node is self.tau:
            m = (self.mu_mom if node is self.mu else self.tau_mom).cpu().numpy().reshape(D, K, 2)
            return [m[..., 0].copy(), m[..., 1].copy()]
        if node is self.Z:
            return [self.responsibilities().cpu().numpy().reshape(self.N, 1, K)]
        if node is self.Y:
            y = self.y.cpu().numpy()
            return [y, y * y]
        raise NotImplementedError

    def get_mask(self, node):
        return np.array(True)

    # -- persistence -----------------------------------------------------------------------------------
    _SAVED = ('mu_par', 'mu_mom', 'tau_par', 'tau_mom', 'alpha_r', 'elog_r', 'h', 'q', 'c', 'S1',
              'S2', 'Nk', 'scal')

    def save_state(self, put, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        _delta.save(put, base, self._delta)
        put(base + 'kind', np.array([ord(ch) for ch in 'dgmm'], dtype=np.uint8))
        put(base + 'dims', np.array([self.N, self.D, self.K], dtype=np.int64))
        put(base + 'flags', np.array([1 if self.labels is not None else 0], dtype=np.int64))
        if self.labels is not None:
            put(base + 'labels', self.labels.cpu().numpy())
        self._save_more(put, base)
        for name in self._saved():
            put(base + name, getattr(self, name).cpu().numpy())

    def _saved(self):
        return self._SAVED

    def _save_more(self, put, base):
        pass

    def _check_more(self, reader, base):
        """A checkpoint of the block with missing observations is not this block's."""
        if reader.has(base + 'mask'):
            saved = np.asarray(reader.get(base + 'mask'), dtype=np.uint8).reshape(-1)
            raise ValueError('checkpoint was saved with a mask on Y with %d of %d entries '
                             'observed, the model has no mask on Y: observe Y with the mask of '
                             'the checkpoint before loading it'
                             % (int(np.count_nonzero(saved)), saved.size))

    def load_state(self, reader, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        if not reader.has(base + 'kind') or bytes(np.asarray(reader.get(base + 'kind'),
                                                             dtype=np.uint8)) != b'dgmm':
            raise Exception("File does not contain the state of the fused diagonal-Gaussian-"
                            "mixture block")
        dims = tuple(int(v) for v in reader.get(base + 'dims'))
        if dims != (self.N, self.D, self.K):
            raise ValueError('checkpoint is for (N, D, K) = %s, the model has %s'
                             % (dims, (self.N, self.D, self.K)))
        self._check_more(reader, base)
        torch = self.rt.torch
        self._delta = _delta.load(reader, base)
        if int(np.asarray(reader.get(base + 'flags')).ravel()[0]):
            self.labels = torch.from_numpy(
                np.array(reader.get(base + 'labels'), dtype=np.int32)).to(self.rt.device)
        else:
            self.labels = None
        for name in self._saved():
            getattr(self, name).copy_(torch.from_numpy(
                np.array(reader.get(base + name), dtype=np.float64)).reshape(
                    getattr(self, name).shape).to(self.rt.device))
        self._version += 1
