"""
Execution plan of the diagonal-Gaussian-mixture block (dgmm.py) with missing observations

    Y = Mixture(Z, GaussianARD, mu, tau);  Y.observe(y, mask=m)          y, m (N, D)

``m`` a boolean host array or a ``DeviceMask`` of shape exactly (N, D), a mask of ones included.
Opt-in: ``VB(..., engine='fused')``, tried right after ``DiagGaussianMixturePlan`` (registry
``OPT_IN_MASKED``); the default engine runs the model on the generic engine as before.  A scalar
mask or one that broadcasts over a plate is declined with a reason, and so is everything
``DiagGaussianMixturePlan`` declines, in its words.

With yt = m o y the logits are c + M g + Yt h + (Yt o Yt) q, g = 1/2 <log tau> - 1/2 <tau><mu^2>
(D, K) and c = <log pi> less its maximum: sum_d g leaves c and becomes a third product.  The plan
keeps the count of an element M_dk = sum_n r_nk m_nd beside S1 = sum r yt and S2 = sum r yt^2; it
takes the place of N_k in the updates of ``mu`` and ``tau``.  N_k and sum lse run over the rows
with an observed entry.  The plan's own copy of y holds one quiet-NaN bit pattern at the hidden
positions (``vmp_dgmm_pack_masked``) and the pass finds the mask again as y == y: what the caller's
y holds at a hidden position reaches nothing, and no second (N, D) array is read.

    <log p(Y)>           = S1 . h + S2 . q + M . g - 1/2 (#observed) log 2 pi     (present moments)
    <log p(Z)> + entropy = N_k . <log pi>
                           + sum lse - N_k . c_used - (S1 . h_used + S2 . q_used + M . g_used)

The masks of the parents are the reference's: ``Z`` (N, 1) any entry of the row observed, ``mu``
and ``tau`` (D, 1) any entry of the column, ``alpha`` () any entry.  A row with nothing observed
has ``Z`` moments softmax(<log pi> of the last Z update); a column with nothing observed leaves
``mu`` and ``tau`` at the moments of the prior with bound terms exactly zero.

Checkpoints: kind 'dgmm' with ``mask``, ``M`` and ``g`` added; a checkpoint whose mask differs is
refused.
"""
import ctypes

import numpy as np

from ._mixture import _mask_shape, _p, match_plate_mixture
from .dgmm import DiagGaussianMixturePlan, DGMMKernels, _SPEC, _limits_reason

from ... import _lib
from ...device import ptr

_LIMITS = []


def dgmm_masked_limits():
    """(max K, max D) of the built pass with a mask: host-only ``vmp_dgmm_limits_masked``."""
    if not _LIMITS:
        k, d = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_dgmm_limits_masked(ctypes.byref(k), ctypes.byref(d)))
        _LIMITS.append((k.value, d.value))
    return _LIMITS[0]


class MaskedDGMMKernels(DGMMKernels):

    def plan_masked(self, N, D, K):
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_dgmm_plan_masked(N, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused diagonal-Gaussian-mixture block with a mask '
                                      'supports K <= %d and D <= %d' % dgmm_masked_limits())
        return c.value, w.value

    def pack_masked(self, N, D, y, mask, out, count):
        self.rt.check(self.lib.vmp_dgmm_pack_masked(self.ctx, N, D, _p(y), _p(mask), _p(out),
                                                    ptr(count)))

    def tables_masked(self, D, K, mu_mom, tau_mom, elog_pi, h, q, g, c):
        self.rt.check(self.lib.vmp_dgmm_tables_masked(self.ctx, D, K, _p(mu_mom), _p(tau_mom),
                                                      _p(elog_pi), _p(h), _p(q), _p(g), _p(c)))

    def pass_masked(self, N, D, K, y, labels, h, q, g, c, ws, S1, S2, M, Nk, scal, r_out=None):
        self.rt.check(self.lib.vmp_dgmm_pass_masked(self.ctx, N, D, K, _p(y), _p(labels), _p(h),
                                                    _p(q), _p(g), _p(c), _p(ws), _p(S1), _p(S2),
                                                    _p(M), _p(Nk), _p(scal), _p(r_out)))

    def update_masked(self, D, K, which, prior_a, prior_b, S1, S2, M, other, par, mom, bound):
        self.rt.check(self.lib.vmp_dgmm_update_masked(self.ctx, D, K, which, _p(prior_a),
                                                      _p(prior_b), _p(S1), _p(S2), _p(M),
                                                      _p(other), _p(par), _p(mom), _p(bound)))


def _full_mask(node):
    """``node`` has a mask (host array or DeviceMask) of the full shape of its plates."""
    return node._mask is not True and _mask_shape(node._mask) == tuple(node.plates)


def _mask_reason(Y):
    if Y._mask is True:
        return ''                   # no mask: the model of the block without one, no reason
    if not _full_mask(Y):
        return ('it has a mask of shape %s: the block with missing observations takes a mask of '
                'the full shape of the plates of Y, here %s; a scalar mask or one that broadcasts '
                'over a plate goes through the generic engine'
                % (_mask_shape(Y._mask), tuple(Y.plates)))


_MASKED_SPEC = _SPEC._replace(mask=_mask_reason,
                              limits=_limits_reason(dgmm_masked_limits, ' with a mask'))


class MaskedDiagGaussianMixturePlan(DiagGaussianMixturePlan):

    ANNEALING = False       # the masked tables and updates have no annealed forms

    KERNELS = MaskedDGMMKernels

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates=(N, 1)), GaussianARD, "
                "GaussianARD(const, const, plates=(D, K)), Gamma(const, const, plates=(D, K))), "
                "observed with a mask of the full shape (N, D) (D <= %d, K <= %d); a scalar mask "
                "or one that broadcasts over a plate goes through the generic engine"
                % dgmm_masked_limits()[::-1])

    @staticmethod
    def match(nodes, why=None):
        return match_plate_mixture(nodes, why, _MASKED_SPEC)

    def _repacks(self, node):
        return _full_mask(node)

    # -- set-up ------------------------------------------------------------------------------------
    def _upload_y(self):
        """The mask, then the plan's own copy of y with the hidden pattern in it."""
        rt, torch = self.rt, self.rt.torch
        self._upload_mask()
        super()._upload_y()
        raw = self.y
        self.y = torch.empty_like(raw)
        self.n_obs = torch.zeros(1, dtype=torch.int64, device=rt.device)
        self.kernels.pack_masked(self.N, self.D, raw, self.maskd, self.y, self.n_obs)

    def _materialize(self):
        if not self._ready:
            rt, D, K = self.rt, self.D, self.K
            self.M, self.g, self.g_now = rt.zeros(D, K), rt.zeros(D, K), rt.zeros(D, K)
        super()._materialize()

    def _plan_pass(self):
        return self.kernels.plan_masked(self.N, self.D, self.K)

    def _tables(self, mu_mom, tau_mom):
        self.kernels.tables_masked(self.D, self.K, mu_mom, tau_mom, self.elog_r, self.h, self.q,
                                   self.g, self.c)

    def _update_from_statistics(self, which, prior_a, prior_b, other, par, mom, bound):
        self.kernels.update_masked(self.D, self.K, which, prior_a, prior_b, self.S1, self.S2,
                                   self.M, other, par, mom, bound)

    def _run_pass(self, r_out=None):
        self.kernels.pass_masked(self.N, self.D, self.K, self.y, self.labels, self.h, self.q,
                                 self.g, self.c, self.ws, self.S1, self.S2, self.M, self.Nk,
                                 self.scal, r_out)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def _bound_terms(self):
        k = self.kernels
        D, K = self.D, self.K
        k.tables_masked(D, K, self.mu_mom, self.tau_mom, self.elog_r, self.h_now, self.q_now,
                        self.g_now, self.c_now)
        k.dot(D * K, self.S1, self.h_now, self.ws_small, self.scal[6:7])
        k.dot(D * K, self.S2, self.q_now, self.ws_small, self.scal[7:8])
        k.dot(D * K, self.M, self.g_now, self.ws_small, self.scal[8:9])
        k.dot(K, self.Nk, self.elog_r, self.ws_small, self.scal[9:10])
        s, entropy = self._host_scal()
        n_obs = int(self.n_obs.cpu().numpy()[0])
        return dict(Y=float(s[6] + s[7] + s[8]) - 0.5 * n_obs * np.log(2 * np.pi),
                    Z=float(s[9]) + entropy, mu=float(s[3]), tau=float(s[4]), alpha=float(s[5]))

    def get_moments(self, node):
        if node is self.Y:
            self._materialize()
            y = self.rt.torch.nan_to_num(self.y, nan=0.0).cpu().numpy()     # yt = m o y
            return [y, y * y]
        return super().get_moments(node)

    # -- persistence -----------------------------------------------------------------------------------
    def _saved(self):
        return self._SAVED + ('M', 'g')
