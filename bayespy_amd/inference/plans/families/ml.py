"""Point-estimate families: the maximum-likelihood hyperparameter nodes GammaShape (gamma.py:273-334)
and Concentration (dirichlet.py:234-330).

They have no natural parameters and no log-normaliser.  The plan (``point_estimate = True``) sums the
children's messages to the node's plates with its usual routing and hands them to ``ml_update``,
ONE library launch (csrc/vmp_ml.hip) on the context's stream -- recordable into a sweep graph.
"""
import ctypes

import numpy as np

from .... import darray as da
from ....darray import DArray, fuse, contiguous
from ....device import get_runtime
from ....utils import misc
from ..lazy import _arr, _const
from .base import Family

_ERR_INF = ("Cannot estimate DirichletConcentration because of infs. This means that there are "
            "numerically zero probabilities in the child Dirichlet node.")


def _dense(x, shape):
    """``x`` (a device array, a lazy sum, a number or None = 0) as a contiguous array of ``shape``."""
    shape = tuple(shape)
    if x is None:
        return _const(('zeros', shape), lambda: np.zeros(shape))
    x = _arr(x)
    if type(x) is not DArray:
        x = fuse(lambda a: a + 0.0, x)         # (a lazily evaluated sum: its dense form)
    return contiguous(x.broadcast_to(shape))


def _vp(a):
    return ctypes.c_void_p(a.t.data_ptr())


class _PointFamily(Family):
    point_estimate = True

    def _unsupported(self, what):
        raise NotImplementedError('%s of %s: a maximum-likelihood node has no distribution (the '
                                  'reference does not define it either)'
                                  % (what, type(self.node).__name__))

    def phi_from_parents(self, up):
        self._unsupported('natural parameters')

    def moments_and_cgf(self, phi):
        self._unsupported('natural parameters')

    def gradient(self, rg, u, phi):
        self._unsupported('gradient')

    def _own(self, key, value, shape):
        """A constant of the node (its "prior" messages) dense on the device, uploaded once per
        value (a set-up step outside the sweep; a changed value is uploaded again)."""
        cache = self.__dict__.setdefault('_own_cache', {})
        hit = cache.get(key)
        v = np.asarray(value, dtype=np.float64)
        if hit is None or hit[0].shape != v.shape or not np.array_equal(hit[0], v, equal_nan=True):
            arr = np.ascontiguousarray(np.broadcast_to(v, tuple(shape)))
            hit = (v.copy(), DArray.from_host(arr))
            cache[key] = hit
        return hit[1]


class GammaShapeFamily(_PointFamily):
    """u = [a, log Gamma(a)] (GammaPriorMoments, gamma.py:33-58)."""

    def initial_moments(self):
        return self.fixed_moments(1.0)              # gamma.py:301

    def fixed_moments(self, x):
        a = _arr(np.asarray(x, dtype=np.float64))
        return [a, fuse(lambda v: da.gammaln(v), a)]

    def ml_update(self, msgs):
        rt = get_runtime()
        node = self.node
        pl = tuple(node.plates)
        m0, m1 = _dense(msgs[0], pl), _dense(msgs[1], pl)
        r0 = self._own('m0', node._m0, pl)
        r1 = self._own('m1', node._m1, pl)
        a, lga = DArray.empty(pl), DArray.empty(pl)
        n = int(np.prod(pl)) if pl else 1
        rt.sync_stream()
        rt.note_reads([m0, m1, r0, r1])
        rt.check(rt.lib.vmp_ml_gamma_shape(rt.ctx, n, _vp(m0), _vp(m1), _vp(r0), _vp(r1), _vp(a),
                                           _vp(lga)))
        return [a, lga]

    def bound_term(self, u):
        return None                                  # gamma.py:333-334


class ConcentrationFamily(_PointFamily):
    """u = [alpha, log Gamma(sum alpha) - sum log Gamma(alpha)] (ConcentrationMoments,
    dirichlet.py:25-51)."""

    # the reference loops until convergence; a kernel must not spin forever.  A concentration that
    # grows into the thousands from a = 1 takes tens of thousands of steps (the mixture of
    # tests/ml_models.py: up to ~50 000 per update), so the cap sits four times above that.  A launch
    # that reaches it runs cap x the time of one iteration (3 us at one row of 4,
    # 0.36 ms at 4096 rows of 4)
    max_iter = 200000

    def initial_moments(self):
        return self.fixed_moments(np.ones(self.node.D))       # dirichlet.py:256

    def fixed_moments(self, x):
        a = _arr(np.asarray(x, dtype=np.float64))
        lg = misc.sum_multiply(fuse(lambda v: da.gammaln(v), a), axis=-1)
        s = misc.sum_multiply(a, axis=-1)
        return [a, fuse(lambda t, l: da.gammaln(t) - l, s, lg)]

    def _reg(self):
        node = self.node
        pl, K = tuple(node.plates), node.D
        reg = node.regularization
        return self._own('r0', reg[0], pl + (K,)), self._own('r1', reg[1], pl)

    def ml_update(self, msgs):
        rt = get_runtime()
        node = self.node
        pl, K = tuple(node.plates), node.D
        m0, m1 = _dense(msgs[0], pl + (K,)), _dense(msgs[1], pl)
        r0, r1 = self._reg()
        alpha, work, z = DArray.empty(pl + (K,)), DArray.empty(pl + (K,)), DArray.empty(pl)
        status = rt.torch.empty(3, dtype=rt.torch.int32, device=rt.device)
        rows = int(np.prod(pl)) if pl else 1
        rt.sync_stream()
        rt.note_reads([m0, m1, r0, r1])
        rt.check(rt.lib.vmp_ml_concentration(rt.ctx, rows, K, _vp(m0), _vp(m1), _vp(r0), _vp(r1),
                                             int(self.max_iter), _vp(alpha), _vp(work), _vp(z),
                                             ctypes.c_void_p(status.data_ptr())))
        # [infinite mean_logp, iteration cap reached, iterations]: read with the other validity
        # flags of the operation (inside a recorded sweep: outputs of the graph)
        self.status = status
        rt.defer_check(status[0:1], ValueError, _ERR_INF)
        rt.defer_check(status[1:2], RuntimeError,
                       'The fixed point of %s did not converge in %d iterations'
                       % (node.name, int(self.max_iter)))
        return [alpha, z]

    def bound_term(self, u):
        """sum over the plates of <alpha> . reg0 + z reg1 (dirichlet.py:323-327)."""
        node = self.node
        pl = tuple(node.plates)
        r0, r1 = self._reg()
        t = fuse(lambda a, z, r: a + z * r, misc.sum_multiply(_arr(u[0]), r0, axis=-1),
                 _arr(u[1]), r1)
        return misc.sum_multiply_to_plates(t, to_plates=(), from_plates=pl, ndim=0).reshape(())
