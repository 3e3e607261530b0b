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
goes over when ``Y`` is observed with such a mask, and mini-batches by the forms of dgmm_svi.py
(``engine='fused+batches+gaussian'``).

Checkpoints: the block writes its own ``plans/<i>/`` group (kind 'dgmm') like every fused plan.
"""
import ctypes

import numpy as np

from . import _delta
from ._dirichlet import DirichletKernels, prior_table
from ._mixture import (MixtureSpec, PlateMixturePlan, _p, cluster_plate_reason,
                       match_plate_mixture)

from ... import _lib
from ...nodes.gaussian import GaussianARD
from ...nodes.gamma import Gamma

_LIMITS = []


def dgmm_limits():
    """(max K, max D) of the built pass: host-only ``vmp_dgmm_limits``."""
    if not _LIMITS:
        k, d = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_dgmm_limits(ctypes.byref(k), ctypes.byref(d)))
        _LIMITS.append((k.value, d.value))
    return _LIMITS[0]


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

    # stochastic VI (dgmm_svi.py); these take the place of the one-table forms of DirichletKernels
    def natural_step_workspace(self, D, K):
        """The doubles of ``ws`` that ``natural_step`` needs."""
        w = ctypes.c_int64()
        self.rt.check(self.lib.vmp_dgmm_natural_step_workspace(D, K, ctypes.byref(w)))
        return w.value

    def natural_step(self, D, K, nodes, m0, beta0, a0, b0, S1, S2, cnt, per_element, mu_par, mu_mom,
                     tau_par, tau_mom, prior_r, Nk, alpha_r, elog_r, mult, scale, ws, bound):
        """``vmp_dgmm_natural_step``: mu (bit 1 of ``nodes``), tau (bit 2) and the weights row
        (bit 4) one step along their natural gradients, in one launch; ``bound`` has three slots."""
        self.rt.check(self.lib.vmp_dgmm_natural_step(
            self.ctx, D, K, nodes, _p(m0), _p(beta0), _p(a0), _p(b0), _p(S1), _p(S2), _p(cnt),
            per_element, _p(mu_par), _p(mu_mom), _p(tau_par), _p(tau_mom), _p(prior_r), _p(Nk),
            _p(alpha_r), _p(elog_r), float(mult), float(scale), _p(ws), _p(bound)))

    # deterministic annealing
    def tables_annealed(self, D, K, annealing, mu_mom, tau_mom, elog_pi, h, q, c, gsum=None):
        self.rt.check(self.lib.vmp_dgmm_tables_annealed(self.ctx, D, K, float(annealing),
                                                        _p(mu_mom), _p(tau_mom), _p(elog_pi), _p(h),
                                                        _p(q), _p(c), _p(gsum)))

    def update_annealed(self, D, K, which, annealing, prior_a, prior_b, S1, S2, Nk, other, par, mom,
                        ab):
        """which 0 / 1: the annealed update of mu / tau; 2 / 3: only the parts ``ab`` = (A, B) of
        the bound term of the q that ``par`` and ``mom`` hold."""
        self.rt.check(self.lib.vmp_dgmm_update_annealed(
            self.ctx, D, K, which, float(annealing), _p(prior_a), _p(prior_b), _p(S1), _p(S2),
            _p(Nk), _p(other), _p(par), _p(mom), _p(ab)))


def _plates_reason(Y, mu):
    if len(Y.plates) != 2 or len(mu.plates) != 2 or mu.ndim != 0 or Y.ndim != 0:
        return ('it needs plates (N, D) and scalar GaussianARD variables, Y has plates %s and mu '
                'has plates %s and shape %s' % (Y.plates, mu.plates, mu.shape))


def _limits_reason(limits, which=''):
    """The check of D and K against ``limits()`` of the block (``which``: ' with a mask')."""
    def reason(r):
        D, K = r['Y'].plates[1], r['Y'].clusters
        max_k, max_d = limits()
        if K > max_k or D > max_d:
            return ('D = %d, K = %d exceed the limits of the block%s (D <= %d, K <= %d)'
                    % (D, K, which, max_d, max_k))
    return reason


# dgmm_masked.py replaces ``mask`` and ``limits``: it takes a mask of the full shape of the plates
# of Y where this block takes none
_SPEC = MixtureSpec(
    label='fused diagonal-Gaussian-mixture block',
    takes=lambda Y: Y.node_class is GaussianARD,
    observed='Y', weights='alpha',
    params=(('mu', GaussianARD, ('value', 'parameters')), ('tau', Gamma, ('parameters',))),
    arity='the mixed GaussianARD has further constructor arguments',
    parents='its parents are not (Categorical(Dirichlet), GaussianARD, Gamma)',
    constant='a parameter of %s is a node (%s), not a constant',
    role_plates='plates of Z / mu / tau / alpha are {} / {} / {} / {}, not (N, 1) / (D, K) / '
                '(D, K) / ()',
    mask=lambda Y: None if Y._mask is True else
    'it has a mask: the block takes fully observed data only; a mask goes through the generic '
    'engine',
    plates=lambda Y, mu: cluster_plate_reason(Y) or _plates_reason(Y, mu),
    limits=_limits_reason(dgmm_limits))


class DiagGaussianMixturePlan(PlateMixturePlan):

    KERNELS = DGMMKernels
    LABEL, KIND = _SPEC.label, 'dgmm'
    OBSERVED, WEIGHTS = 'Y', 'alpha'
    TERMS = ('Y', 'Z', 'mu', 'tau', 'alpha')
    ANNEALING = True        # VB.set_annealing: the updates and the bound read node.annealing

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates=(N, 1)), GaussianARD, "
                "GaussianARD(const, const, plates=(D, K)), Gamma(const, const, plates=(D, K))), "
                "fully observed (D <= %d, K <= %d)" % dgmm_limits()[::-1])

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _SPEC)

    def _repacks(self, node):
        return node._mask is True

    def _hand_over(self):
        from .dgmm_masked import MaskedDiagGaussianMixturePlan
        if MaskedDiagGaussianMixturePlan.match(self.nodes()) is not None:
            # Y was observed with a mask of its full shape: the block for missing observations
            MaskedDiagGaussianMixturePlan(self.roles, runtime=self._rt)
        else:
            super()._hand_over()

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
        self._stale = False

    def _repack(self):
        """New observations of the same shape: y again (with its mask in dgmm_masked.py)."""
        self._upload_y()

    def _const(self, node, i, positive, what):
        a = np.asarray(node.parents[i].value, dtype=np.float64)
        if positive and np.any(a <= 0):
            raise ValueError('%s of %s should be positive' % (what, node.name))
        return np.ascontiguousarray(np.broadcast_to(a, (self.D, self.K)))

    def _materialize(self):
        if self._ready:
            if self._stale:
                self._restate()
            return
        self._delta = _delta.delta_roles(self.roles)
        rt, k = self.rt, self.kernels
        D, K = self.D, self.K
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
        self.ws = rt.empty(int(wsd))
        self.ws_small = rt.empty(max(D * K, 1024))
        # [0] sum lse, [1] N_k . c used, [2] S1 . h + S2 . q used, [3] bound of mu, [4] of tau,
        # [5] of alpha, [6] S1 . h, [7] S2 . q, [8] N_k . g (present moments), [9] N_k . <log pi>
        self.scal = rt.zeros(12)
        # the parts (A, B) of the bound terms of mu and tau under annealing; a node's pair is formed
        # again at the request unless its last update was the annealed one, which leaves it here
        self.ab = rt.zeros(4)
        self._ab_fresh = dict(mu=False, tau=False)
        # whose q the plain entry points made (their single bound slots hold its term at T = 1);
        # scal[10] keeps the others as a bit set (1 mu, 2 tau, 4 alpha), so a checkpoint knows
        self._plain = dict(mu=True, tau=True, alpha=True)
        # the priors; a given initial state replaces them below
        k.update(D, K, 0, self.m0, self.beta0, None, None, None, None, self.mu_par, self.mu_mom,
                 self.scal[3:4])
        k.update(D, K, 1, self.a0, self.b0, None, None, None, None, self.tau_par, self.tau_mom,
                 self.scal[4:5])
        self._init_mu(m0, beta0)
        self._init_tau(a0, b0)
        self._weights_step(5, self._weights_init_counts(pr))
        self._labels_from_init()
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

    def _tables(self, mu_mom, tau_mom):
        """The tables of the pass from the given moments (None: no observation term)."""
        self.kernels.tables(self.D, self.K, mu_mom, tau_mom, self.elog_r, self.h, self.q, self.c)

    def _update_from_statistics(self, which, prior_a, prior_b, other, par, mom, bound):
        self.kernels.update(self.D, self.K, which, prior_a, prior_b, self.S1, self.S2, self.Nk,
                            other, par, mom, bound)

    # -- deterministic annealing (VB.set_annealing) --------------------------------------------------
    def _annealing(self, node):
        """The coefficient the node carries NOW; a form of the block that has no annealed kernels
        declines any other than 1 here too (the attribute can be set without VB.set_annealing)."""
        b = float(getattr(node, 'annealing', 1.0))
        if b != 1.0 and not type(self).ANNEALING:
            raise NotImplementedError(
                "annealing is not built into the fused %s plan; build the engine with "
                "VB(..., engine='generic')" % type(self).__name__)
        return b

    _PLAIN_BITS = dict(mu=1, tau=2, alpha=4)

    def _set_plain(self, key, plain):
        if self._plain[key] != plain:
            self._plain[key] = plain
            self.scal[10:11].fill_(float(sum(bit for k, bit in self._PLAIN_BITS.items()
                                             if not self._plain[k])))

    def load_state(self, reader, nodes, index):
        super().load_state(reader, nodes, index)
        bits = int(self.scal[10].item())
        self._plain = {k: not (bits & bit) for k, bit in self._PLAIN_BITS.items()}
        self._ab_fresh = dict(mu=False, tau=False)
        self._L_annealing = None

    def _tables_annealed(self, b):
        self.kernels.tables_annealed(self.D, self.K, b, self.mu_mom, self.tau_mom, self.elog_r,
                                     self.h, self.q, self.c)

    def _update_annealed(self, key, b):
        D, K = self.D, self.K
        if key == 'mu':
            self.kernels.update_annealed(D, K, 0, b, self.m0, self.beta0, self.S1, self.S2, self.Nk,
                                         self.tau_mom, self.mu_par, self.mu_mom, self.ab[0:2])
        else:
            self.kernels.update_annealed(D, K, 1, b, self.a0, self.b0, self.S1, self.S2, self.Nk,
                                         self.mu_mom, self.tau_par, self.tau_mom, self.ab[2:4])
        self._ab_fresh[key] = True

    def _weights_annealed(self, b):
        """alpha = b (prior + N_k): the shared Dirichlet kernel on the scaled prior and counts
        (its own bound term is of the scaled prior and is not used: scal[11] is a spare slot)."""
        K = self.K
        self.kernels.dirichlet(1, K, K, 1, b * self.prior_r, b * self.Nk, self.alpha_r, self.elog_r,
                               self.ws_small, self.scal[11:12])

    def _run_pass(self, r_out=None):
        """The statistics of the present ``Z`` state (tables ``h`` / ``q`` / ``c`` or labels)."""
        self.kernels.pass_(self.N, self.D, self.K, self.y, self.labels, self.h, self.q, self.c,
                           self.ws, self.S1, self.S2, self.Nk, self.scal, r_out)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        self.rt.sync_stream()
        # the coefficient of deterministic annealing; 1.0 runs exactly the plain entry points
        b = self._annealing(node)
        if node is self.Z:
            self.labels = None
            if b == 1.0:
                self._tables(self.mu_mom, self.tau_mom)
            else:
                self._tables_annealed(b)
            self._run_pass()
        elif node is self.mu:
            if b == 1.0:
                self._update_from_statistics(0, self.m0, self.beta0, self.tau_mom, self.mu_par,
                                             self.mu_mom, self.scal[3:4])
            else:
                self._update_annealed('mu', b)
            self._set_plain('mu', b == 1.0)
        elif node is self.tau:
            if b == 1.0:
                self._update_from_statistics(1, self.a0, self.b0, self.mu_mom, self.tau_par,
                                             self.tau_mom, self.scal[4:5])
            else:
                self._update_annealed('tau', b)
            self._set_plain('tau', b == 1.0)
        elif node is self.alpha:
            if b == 1.0:
                self._weights_step(5, self.Nk)
            else:
                self._weights_annealed(b)
            self._set_plain('alpha', b == 1.0)
        else:
            return
        if b == 1.0 and node is not self.Z and node is not self.alpha:
            self._ab_fresh['mu' if node is self.mu else 'tau'] = False
        self._version += 1

    def _lower_bound_terms(self):
        # the temperature of a term is its node's at the request: the cached terms hold for the
        # coefficients they were formed with
        ann = tuple(self._annealing(n) for n in (self.Z, self.mu, self.tau, self.alpha))
        if getattr(self, '_L_annealing', None) != ann:
            self._L_version = -1
            self._L_annealing = ann
        return super()._lower_bound_terms()

    def _annealed_term(self, key, b):
        """A - T B of mu or tau, T = 1 / b, from the parts of the q the tables hold."""
        D, K = self.D, self.K
        if not self._ab_fresh[key]:
            if key == 'mu':
                self.kernels.update_annealed(D, K, 2, 1.0, self.m0, self.beta0, None, None, None,
                                             None, self.mu_par, self.mu_mom, self.ab[0:2])
            else:
                self.kernels.update_annealed(D, K, 3, 1.0, self.a0, self.b0, None, None, None,
                                             None, self.tau_par, self.tau_mom, self.ab[2:4])
            self._ab_fresh[key] = True
        ab = self.ab.cpu().numpy()
        A, B = (ab[0], ab[1]) if key == 'mu' else (ab[2], ab[3])
        return float(A - B / b)

    def _annealed_weights_term(self, b):
        """A - T B of the Dirichlet weights from their K parameters and moments (host, K <= 64)."""
        from scipy.special import gammaln
        a0 = self.prior_r.cpu().numpy().astype(np.float64)
        a, e = self.alpha_r.cpu().numpy(), self.elog_r.cpu().numpy()
        A = gammaln(a0.sum()) - gammaln(a0).sum() + np.dot(a0, e)
        B = gammaln(a.sum()) - gammaln(a).sum() + np.dot(a, e)
        return float(A - B / b)

    def _bound_terms(self):
        k = self.kernels
        D, K = self.D, self.K
        bz, bmu, btau, bal = self._L_annealing
        if (bz, bmu, btau, bal) != (1.0, 1.0, 1.0, 1.0) or not all(self._plain.values()):
            return self._bound_terms_annealed(bz, bmu, btau, bal)
        k.tables(D, K, self.mu_mom, self.tau_mom, self.elog_r, self.h_now, self.q_now,
                 self.c_now, self.gsum)
        k.dot(D * K, self.S1, self.h_now, self.ws_small, self.scal[6:7])
        k.dot(D * K, self.S2, self.q_now, self.ws_small, self.scal[7:8])
        k.dot(K, self.Nk, self.gsum, self.ws_small, self.scal[8:9])
        k.dot(K, self.Nk, self.elog_r, self.ws_small, self.scal[9:10])
        s, entropy = self._host_scal()
        return dict(Y=float(s[6] + s[7] + s[8]) - 0.5 * self.N * D * np.log(2 * np.pi),
                    Z=float(s[9]) + entropy, mu=float(s[3]), tau=float(s[4]), alpha=float(s[5]))

    def _bound_terms_annealed(self, bz, bmu, btau, bal):
        """The terms when a coefficient is not 1, or a q was made by an annealed update: Y as ever,
        Z with its entropy part times T_z, mu / tau / alpha as A - T B (the single slots of the
        plain updates hold A - B of a q made by a plain update, and serve at T = 1)."""
        k = self.kernels
        D, K = self.D, self.K
        k.tables(D, K, self.mu_mom, self.tau_mom, self.elog_r, self.h_now, self.q_now,
                 self.c_now, self.gsum)
        k.dot(D * K, self.S1, self.h_now, self.ws_small, self.scal[6:7])
        k.dot(D * K, self.S2, self.q_now, self.ws_small, self.scal[7:8])
        k.dot(K, self.Nk, self.gsum, self.ws_small, self.scal[8:9])
        k.dot(K, self.Nk, self.elog_r, self.ws_small, self.scal[9:10])
        s, entropy = self._host_scal()
        t = dict(Y=float(s[6] + s[7] + s[8]) - 0.5 * self.N * D * np.log(2 * np.pi),
                 Z=float(s[9]) + entropy / bz)
        for key, b, slot in (('mu', bmu, 3), ('tau', btau, 4)):
            plain = b == 1.0 and self._plain[key]
            t[key] = float(s[slot]) if plain else self._annealed_term(key, b)
        t['alpha'] = float(s[5]) if bal == 1.0 and self._plain['alpha'] \
            else self._annealed_weights_term(bal)
        return t

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

    # -- persistence -----------------------------------------------------------------------------------
    _SAVED = ('mu_par', 'mu_mom', 'tau_par', 'tau_mom', 'alpha_r', 'elog_r', 'h', 'q', 'c', 'S1',
              'S2', 'Nk', 'scal')
