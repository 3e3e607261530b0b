"""GaussianMarkovChain and its Gaussian view (gaussian_markov_chain.py:270-707, :1988-2098)."""
import os

import numpy as np

from .... import darray as da
from ....darray import DArray, fuse, contiguous
from ....nodes.node import Constant, Stochastic
from ....nodes.gaussian import is_gaussian_gamma
from ....utils import misc, linalg
from ....utils.shapes import broadcasted_shape, is_shape_subset, multiplier_factor
from ..lazy import (DerivedArray,
                    FactoredMoment,
                    LOG2PI,
                    LazyContract,
                    LazySum,
                    PlateSums,
                    Terms,
                    _CONSTS,
                    _Deferred,
                    _LazyList,
                    _arr,
                    _check_device,
                    _const,
                    _diag2,
                    _eye,
                    _factored_min_plates,
                    _gaussian_gradient,
                    _gaussian_q_term,
                    _inner_second,
                    _is_lazy,
                    _lazy_mvdot,
                    _multigammaln,
                    _ones,
                    _shape,
                    _sum_last,
                    _trail,
                    _wsum)
from .base import Family


class GaussianMarkovChainFamily(Family):
    """gaussian_markov_chain.py:270-707 with the joint-parent wrappers folded in; the
    smoother (compute_moments_and_cgf, :89-123) is ``linalg.block_banded_solve``."""

    def __init__(self, node):
        super().__init__(node)
        self.N, self.D = node.N, node.D
        N = self.N
        e0 = np.zeros(N); e0[0] = 1.0
        enl = np.ones(N); enl[-1] = 0.0
        self._e0v = DArray.from_host(e0.reshape(N, 1))
        self._e0 = DArray.from_host(e0.reshape(N, 1, 1))
        self._en0 = DArray.from_host((1.0 - e0).reshape(N, 1, 1))
        self._enl = DArray.from_host(enl.reshape(N, 1, 1))
        # A or nu carry an N-1 plate (GaussianMarkovChain only): the formulas keep the time axis
        self.time_varying = bool(getattr(node, 'time_varying', False))
        self._solve = None          # (x, V, C) of the last smoother run
        self._pair = None           # (x, sum_b <x_t x_t^T>, sum_b <x_t x_{t+1}^T>) made from it
        self.pair_stats_calls = 0   # messages answered from the plate sums of vmp_chain_pair_stats
        # input signals (the fifth parent, K-dimensional): A holds [A | B], rows of D + K
        self.Kin = int(getattr(node, 'K_inputs', 0))
        self._in = None             # (x, <u>, sums of vmp_chain_input_stats made from them)
        self.input_stats_calls = 0  # messages answered from the plate sums of vmp_chain_input_stats

    def plates_to_parent(self, index):
        if index < 2:
            return self.node.plates
        if index == 4:
            return self.node.plates + (self.N - 1,)
        return self.node.plates + (self.N - 1, self.D)

    def mask_to_parent(self, index, mask):
        if index < 2:
            return mask
        if index == 4:
            return mask.reshape(mask.shape + (1,))
        return mask.reshape(mask.shape + (1, 1))

    def constant_moments(self, index, value):
        v = _arr(value)
        if index == 0:
            return [v, linalg.outer(v, v)]
        if index == 1:
            return [v, linalg.chol_logdet(linalg.chol(v))]
        if index == 2 or index == 4:
            return [v, linalg.outer(v, v)]
        return [v, fuse(lambda a: da.log(a), v)]

    def _time_axis(self, x, tail, index):
        """Parent moments of A / nu with full row (and variable) axes ``tail`` and an explicit
        (unit) time axis before the row axis; plate-compressed moments are expanded as views."""
        x = _arr(x)
        par = self.node.parents[index]
        npl = len(par.value.shape) - (1 if index == 2 else 0) if isinstance(par, Constant) \
            else len(par.plates)
        nt = len(tail)
        lead = x.shape[:max(0, x.ndim - nt)]
        x = x.broadcast_to(lead + tuple(tail))
        if npl >= 2 and len(lead) >= 1:
            return x                      # (..., 1, D, ...) already carries the time axis
        return x.reshape(lead + (1,) + tuple(tail)) if x.t.is_contiguous() else \
            DArray(x.t.unsqueeze(len(lead)))

    def _dyn(self, up):
        """Moments of the dynamics with their time axis.  With input signals a row of ``A`` is
        [A | B], of D + K elements: the callers take the blocks."""
        D, R = self.D, self.D + self.Kin
        Am = self._time_axis(up[2][0], (D, R), 2)          # (..., 1, D, D)
        AA = self._time_axis(up[2][1], (D, R, R), 2)       # (..., 1, D, D, D)
        nu = self._time_axis(up[3][0], (D,), 3)            # (..., 1, D)
        lognu = self._time_axis(up[3][1], (D,), 3)
        return Am, AA, nu, lognu

    def _inputs(self, up):
        """Moments of the input signals with their (unit or N-1) time axis:
        <u> (..., T, K), <u u^T> (..., T, K, K)."""
        K = self.Kin
        z, zz = _arr(up[4][0]), _arr(up[4][1])
        if z.ndim < 2:
            z = z.reshape((1, K))
        if zz.ndim < 3:
            zz = zz.reshape((1, K, K))
        return z, zz

    def _phi0_of_inputs(self, up, Am, AA, nu):
        """The two shifted rows the inputs add to phi0 (gaussian_markov_chain.py:608-615):
        <nu B> z_t at the times 1 .. N-1 and (sum_d <nu A B>_d) z_t, to subtract, at 0 .. N-2."""
        D = self.D
        z, _ = self._inputs(up)
        nuB = fuse(lambda n, b: n * b, _trail(nu, 1), Am[..., D:])               # (..., T, D, K)
        nuAB = misc.sum_multiply(_trail(nu, 2), AA[..., :D, D:], axis=-3)        # (..., T, D, K)
        nxt = self._over_time(linalg.mvdot(nuB, z), 1)                           # (..., N-1, D)
        prv = self._over_time(linalg.mvdot(nuAB, z), 1)
        zero = _const(('zeros', (1, D)), lambda: np.zeros((1, D)))
        return misc.concatenate([zero, nxt], axis=-2), misc.concatenate([prv, zero], axis=-2)

    def _over_time(self, a, nvar):
        """``a`` with its (unit or N-1) time axis, ``nvar`` axes from the end, as N-1 blocks."""
        ax = a.ndim - nvar - 1
        if a.shape[ax] == self.N - 1:
            return a
        return a.broadcast_to(a.shape[:ax] + (self.N - 1,) + a.shape[ax + 1:])

    def _phi_time_varying(self, up):
        """phi of N-1 different transitions (gaussian_markov_chain.py:560-610): the blocks
        nu_t <a a^T>_t sit at the times 0..N-2 of phi1, diag(nu_t) at 1..N-1, nu_t A_t in phi2."""
        m, Lam = up[0][0], up[1][0]
        Am, AA, nu, _ = self._dyn(up)
        D = self.D
        Lm = linalg.mvdot(Lam, m)
        phi0 = fuse(lambda e, v: e * v, self._e0v, _arr(Lm).reshape(_shape(Lm)[:-1] + (1, D)))
        if self.Kin:
            nxt, prv = self._phi0_of_inputs(up, Am, AA, nu)
            phi0 = fuse(lambda p, a, b: p + a - b, phi0, nxt, prv)
            Am, AA = Am[..., :D], AA[..., :D, :D]
        nuAA = self._over_time(misc.sum_multiply(_trail(nu, 2), AA, axis=-3), 2)
        dnu = self._over_time(misc.diag(nu, ndim=1), 2)
        zero = _const(('zeros', (1, D, D)), lambda: np.zeros((1, D, D)))
        at_prev = misc.concatenate([nuAA, zero], axis=-3)                     # (..., N, D, D)
        at_next = misc.concatenate([zero, dnu], axis=-3)
        L = _arr(Lam)
        L = L.reshape(L.shape[:-2] + (1,) + L.shape[-2:])
        phi1 = fuse(lambda a, l, d, q: -0.5 * (a * l + d + q), self._e0, L, at_next, at_prev)
        phi2 = fuse(lambda n, a: n * a, _trail(nu, 1), Am).swapaxes(-1, -2)
        return [phi0, phi1, phi2]

    def phi_from_parents(self, up):
        if self.time_varying:
            return self._phi_time_varying(up)
        m, Lam = up[0][0], up[1][0]
        Am, AA, nu, _ = self._dyn(up)
        Lm = linalg.mvdot(Lam, m)
        phi0 = fuse(lambda e, v: e * v, self._e0v, _arr(Lm).reshape(_shape(Lm)[:-1] + (1, self.D)))
        if self.Kin:
            nxt, prv = self._phi0_of_inputs(up, Am, AA, nu)
            phi0 = fuse(lambda p, a, b: p + a - b, phi0, nxt, prv)
            Am, AA = Am[..., :self.D], AA[..., :self.D, :self.D]
        nuAA = misc.sum_multiply(_trail(nu, 2), AA, axis=-3)                  # (..., 1, D, D)
        dnu = misc.diag(nu, ndim=1)                                           # (..., 1, D, D)
        L = _arr(Lam)
        L = L.reshape(L.shape[:-2] + (1,) + L.shape[-2:])
        phi1 = fuse(lambda a, b, c, l, d, q: -0.5 * (a * l + b * d + c * q),
                    self._e0, self._en0, self._enl, L, dnu, nuAA)
        phi2 = fuse(lambda n, a: n * a, _trail(nu, 1), Am).swapaxes(-1, -2)   # nu_i A_ij -> [j][i]
        return [phi0, phi1, phi2]

    def moments_and_cgf(self, phi):
        A = fuse(lambda p: -2 * p, phi[1])
        B = fuse(lambda p: -p, phi[2])
        V, C, x, ld = linalg.block_banded_solve(A, B, phi[0])
        D = self.D
        xa = x.reshape(x.shape + (1,))
        xb = x.reshape(x.shape[:-1] + (1, D))
        u1 = fuse(lambda a, b, c: a * b + c, xa, xb, V)
        u2 = fuse(lambda a, b, c: a * b + c, xa[..., :-1, :, :], xb[..., 1:, :, :], C)
        g = fuse(lambda s, l: -0.5 * s + 0.5 * l,
                 misc.sum_multiply(x, phi[0], axis=(-1, -2)), ld)
        if self.time_varying or self.Kin:
            # kept for the plate sums of the messages -- only where they can be used (the solver
            # ran with shared matrices: V, C are not plate-sized)
            shared = all(p == 1 for p in V.shape[:-3])
            self._solve, self._pair = ((x, V, C) if shared else None), None
        return [x, u1, u2], g

    def cgf_from_parents(self, up):
        mm = up[0][1]
        Lam, logdet = up[1]
        _, _, _, lognu = self._dyn(up)
        s = misc.sum_multiply(lognu, axis=(-1, -2))
        # a unit time axis stands for N-1 equal rows, an N-1 axis was summed over the transitions
        reps = 1 if (self.time_varying and lognu.shape[-2] != 1) else self.N - 1
        g = fuse(lambda t, ld, ln: -0.5 * t + 0.5 * ld + 0.5 * reps * ln,
                 misc.sum_multiply(Lam, mm, axis=(-1, -2)), logdet, s)
        if not self.Kin:
            return g
        # -1/2 sum_t <u_t u_t^T> : sum_d <nu B B>_d (:638-655); a unit time axis counts N-1 times
        D = self.D
        _, AA, nu, _ = self._dyn(up)
        _, zz = self._inputs(up)
        nuBB = misc.sum_multiply(_trail(nu, 2), AA[..., D:, D:], axis=-3)        # (..., T, K, K)
        reps_in = self.N - 1 if (zz.shape[-3] == 1 and nuBB.shape[-3] == 1) else 1
        gin = misc.sum_multiply(zz, nuBB, axis=(-1, -2, -3))
        return fuse(lambda a, b: a - 0.5 * reps_in * b, g, gin)

    def fixed_moments_and_f(self, x):
        x = _arr(x)
        if x.shape[-2:] != (self.N, self.D):
            raise ValueError("Invalid shape")
        D = self.D
        xa = x.reshape(x.shape + (1,))
        xb = x.reshape(x.shape[:-1] + (1, D))
        u1 = fuse(lambda a, b: a * b, xa, xb)
        u2 = fuse(lambda a, b: a * b, xa[..., :-1, :, :], xb[..., 1:, :, :])
        return [x, u1, u2], -0.5 * self.N * D * LOG2PI

    def message_to_parent(self, index, u, up):
        x, XX, XpXn = _arr(u[0]), _arr(u[1]), _arr(u[2])
        if index < 2:
            # the initial state is a Gaussian(mu, Lambda) variable (:443-460)
            x0, x0x0 = x[..., 0, :], XX[..., 0, :, :]
            m, mm = up[0]
            L = up[1][0]
            if index == 0:
                return [linalg.mvdot(L, x0), fuse(lambda l: -0.5 * l, L)]
            xm, mx = linalg.outer(x0, m), linalg.outer(m, x0)
            return [fuse(lambda a, b, c, d: -0.5 * (a - b - c + d), x0x0, xm, mx, mm), 0.5]
        Am, AA, nu, _ = self._dyn(up)
        if index == 4:
            return self._inputs_message(x, Am, AA, nu)
        if self.Kin:
            return self._driven_dynamics_message(index, u, up, Am, AA, nu)
        pair = self._summed_pair_moments(index, u) if self.time_varying else None
        if pair is not None:
            # the sums over the sequences are made already: the formulas below are linear in the
            # second moments, and neither A nor nu carries a sequence plate here
            XX, XpXn = pair
        XnXp = XpXn.swapaxes(-1, -2)                     # [i][j] = <x_n[i] x_{n-1}[j]>
        XXp = XX[..., :-1, :, :]
        if pair is not None:
            out = _SummedMessage(self._dynamics_message(index, XX, XXp, XnXp, Am, AA, nu,
                                                         count=int(np.prod(self.node.plates))))
            out.plates_from = (1,) * len(self.node.plates) + (self.N - 1, self.D)
            return out
        return self._dynamics_message(index, XX, XXp, XnXp, Am, AA, nu)

    def _summed_pair_moments(self, index, u):
        """(sum_b <x_t x_t^T>, sum_b <x_t x_{t+1}^T>) with unit sequence plates from ONE read of the
        means (``vmp_chain_pair_stats``) plus ny times the covariances the solver returned once --
        when the solver ran with shared matrices, the chain has sequence plates, the mask to the
        parent is all true and the kernel has an instance for D (tune key chain_pair_stats);
        None otherwise: the general operations plate-sum the (ny, N, D, D) moments."""
        ent = self._solve
        if ent is None or ent[0] is not u[0]:
            return None             # moments not from this family's smoother (loaded, fixed value)
        x, V, C = ent
        node = self.node
        ny = int(np.prod(x.shape[:-2])) if x.ndim > 2 else 1
        if ny <= 1 or ny != int(np.prod(node.plates)) or any(p != 1 for p in V.shape[:-3]):
            return None
        if self._pair is None or self._pair[0] is not x:
            max_d, on, _ = linalg.chain_pair_stats_limits()
            if not on or self.D > max_d:
                return None
            plan = node._plan
            for idx in (2, 3):
                if isinstance(node.parents[idx], Constant):
                    continue
                mask, _ = plan._mask_factor(
                    (id(node), idx),
                    lambda idx=idx: self.mask_to_parent(idx, np.asarray(plan._mask_array(node))))
                if mask is not None:
                    return None
            Sxx, Sxp = linalg.chain_pair_stats(x)
            lead = (1,) * len(node.plates)
            N, D = self.N, self.D
            XX = fuse(lambda s, v: s + float(ny) * v, Sxx, V.reshape((N, D, D)))
            XpXn = fuse(lambda s, c: s + float(ny) * c, Sxp, C.reshape((N - 1, D, D)))
            self._pair = (x, XX.reshape(lead + (N, D, D)), XpXn.reshape(lead + (N - 1, D, D)))
        self.pair_stats_calls += 1
        return self._pair[1], self._pair[2]

    def _inputs_message(self, x, Am, AA, nu):
        """To the input signals (gaussian_markov_chain.py:504-525):
        m0_t = <nu B>^T x_{t+1} - (sum_d <nu A B>_d)^T x_t,  m1_t = -1/2 sum_d <nu B B>_d."""
        D = self.D
        nuB = fuse(lambda n, b: n * b, _trail(nu, 1), Am[..., D:])               # (..., T, D, K)
        nuAB = misc.sum_multiply(_trail(nu, 2), AA[..., :D, D:], axis=-3)        # (..., T, D, K)
        nuBB = misc.sum_multiply(_trail(nu, 2), AA[..., D:, D:], axis=-3)        # (..., T, K, K)
        a = misc.sum_multiply(nuB, _trail(contiguous(x[..., 1:, :]), 1), axis=-2)
        b = misc.sum_multiply(nuAB, _trail(contiguous(x[..., :-1, :]), 1), axis=-2)
        return [fuse(lambda p, q: p - q, a, b), fuse(lambda q: -0.5 * q, nuBB)]

    def _driven_dynamics_message(self, index, u, up, Am, AA, nu):
        """To [A | B] or nu of a chain with input signals (gaussian_markov_chain.py:485-498): the
        blocks <x_{t+1} x_t^T> | x_{t+1} z_t^T of the first and
        [[<x_t x_t^T>, x_t z_t^T], [z_t x_t^T, <z_t z_t^T>]] of the second moment, concatenated, go
        through the formulas of the chain without inputs."""
        x, XX, XpXn = _arr(u[0]), _arr(u[1]), _arr(u[2])
        summed = self._summed_input_moments(index, u, up)
        if summed is not None:
            XX, XpXn, xnz, xpz, zz = summed
        else:
            z, zz = self._inputs(up)
            xnz = linalg.outer(x[..., 1:, :], z)                  # (..., N-1, D, K)
            xpz = linalg.outer(x[..., :-1, :], z)
        XnXp = XpXn.swapaxes(-1, -2)
        XXp = XX[..., :-1, :, :]
        M0 = misc.concatenate([XnXp, xnz], axis=-1)               # (..., N-1, D, D+K)
        M1 = misc.concatenate([misc.concatenate([XXp, xpz], axis=-1),
                               misc.concatenate([xpz.swapaxes(-1, -2), zz], axis=-1)], axis=-2)
        if summed is None:
            return self._dynamics_message(index, XX, M1, M0, Am, AA, nu)
        out = _SummedMessage(self._dynamics_message(index, XX, M1, M0, Am, AA, nu,
                                                     count=int(np.prod(self.node.plates))))
        out.plates_from = (1,) * len(self.node.plates) + (self.N - 1, self.D)
        return out

    def _summed_input_moments(self, index, u, up):
        """(sum_b <x_t x_t^T>, sum_b <x_t x_{t+1}^T>, sum_b x_{t+1} z_t^T, sum_b x_t z_t^T,
        sum_b <z_t z_t^T>) with unit sequence plates: the first two as in
        ``_summed_pair_moments``, the cross terms from ONE read of the means of the states and of
        the inputs (``vmp_chain_input_stats``) -- under the conditions of ``_summed_pair_moments``,
        when the kernel has an instance for (D, K), the inputs carry all the sequence plates or
        none, and the tune key chain_input_stats is on; None otherwise: the general operations
        form the outer products and plate-sum them."""
        ent = self._solve
        if ent is None or ent[0] is not u[0]:
            return None
        x = ent[0]
        node = self.node
        N, D, K = self.N, self.D, self.Kin
        ny = int(np.prod(node.plates))
        z, zz = self._inputs(up)
        zrows = int(np.prod(z.shape[:-2]))
        if ny <= 1 or zrows not in (1, ny) or (zrows == ny and len(z.shape[:-2]) > len(node.plates)):
            return None
        max_d, max_k, on, _ = linalg.chain_input_stats_limits()
        if not on or D > max_d or K > max_k:
            return None
        pair = self._summed_pair_moments(index, u)
        if pair is None:
            return None
        lead = (1,) * len(node.plates)
        if self._in is None or self._in[0] is not x or self._in[1] is not up[4][0]:
            constant = isinstance(node.parents[4], Constant)
            zt = contiguous(self._over_time(z, 1))
            # the inputs' own second moment: a constant's is z z^T, summed by the kernel with the
            # rest; a node's holds its covariance: plate-summed by the general operations
            Snz, Spz, Szz = linalg.chain_input_stats(x, zt, with_zz=constant and zrows == ny)
            if Szz is None:
                zzt = self._over_time(zz, 2)
                if zrows == ny:
                    Szz = misc.sum_multiply(zzt.reshape((ny, N - 1, K, K)), axis=0)
                else:
                    Szz = fuse(lambda q: float(ny) * q, zzt.reshape((N - 1, K, K)))
            self._in = (x, up[4][0], Snz.reshape(lead + (N - 1, D, K)),
                        Spz.reshape(lead + (N - 1, D, K)), Szz.reshape(lead + (N - 1, K, K)))
        self.input_stats_calls += 1
        return pair + self._in[2:]

    def _dynamics_message(self, index, XX, XXp, XnXp, Am, AA, nu, count=1):
        """``count``: the sequences already summed into the second moments."""
        if index == 2:
            # to the dynamics matrix, weighted by the innovation precision (:462-475,
            # gaussian.py:2354-2360)
            m0 = (XnXp, _trail(nu, 1))
            m1 = (fuse(lambda q: -0.5 * q, XXp.reshape(XXp.shape[:-2] + (1,) + XXp.shape[-2:])),
                  _trail(nu, 2))
            return [m0, m1]
        t1 = misc.sum_multiply(XnXp, Am, axis=-1)
        t2 = misc.sum_multiply(XXp.reshape(XXp.shape[:-2] + (1,) + XXp.shape[-2:]), AA,
                               axis=(-1, -2))
        t3 = misc.get_diag(XX[..., 1:, :, :], ndim=1)
        return [fuse(lambda a, b, c: a - 0.5 * b - 0.5 * c, t1, t2, t3), 0.5 * count]


class _SummedMessage(list):
    """A message whose factors are summed over some of the child's plates already:
    ``plates_from`` stands for ``plates_to_parent`` when the router sums what is left."""
    plates_from = None


class ChainToGaussianFamily:
    """``_MarkovChainToGaussian`` (gaussian_markov_chain.py:1988-2098): the time axis of a
    chain becomes the last plate; the cross-time moment is dropped."""
    deterministic = True

    def __init__(self, node):
        self.node = node

    def moments(self, ups):
        return list(ups[0][:2])

    def mask_to_parent(self, index, mask):
        mask = np.asarray(mask)
        return np.any(mask, axis=-1) if mask.ndim >= 1 else mask

    def message_to_parent(self, index, m_child, ups, mask=None):
        out = []
        for i, m in enumerate(m_child[:2]):
            if m is None:
                out.append(None)
            elif mask is not None:
                # the last plate turns into a variable axis: apply its mask here
                out.append(fuse(lambda a, w: a * w, _arr(m), _trail(mask, 1 + i)))
            else:
                out.append(m)
        return out + [None]
