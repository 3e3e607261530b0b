"""
Maximum-likelihood hyperparameter nodes (reference: ``GammaShape`` gamma.py:273-334,
``Concentration`` dirichlet.py:234-330).

They hold a point estimate instead of a distribution: no natural parameters, no log-normaliser.
An update sums the children's messages to the node's plates and solves for the maximum-likelihood
value on the device (csrc/vmp_ml.hip):

* ``GammaShape``: the shape ``a`` of Gamma children, psi(a) = -m0 / m1; moments [a, log Gamma(a)]
  (the moments a numeric shape has, gamma.py:33-58);
* ``Concentration``: the concentration vector of Dirichlet / Beta children by the reference's
  fixed point; moments [alpha, log Gamma(sum alpha) - sum log Gamma(alpha)] (dirichlet.py:25-51).
"""
import numpy as np

from .node import Stochastic
from ..utils.shapes import is_shape_subset


class _PointEstimate(Stochastic):
    """A Stochastic node without parents whose q is a point (``initialize=False`` nodes of the
    reference, stochastic.py:83-120)."""

    def __init__(self, dims, plates=None, name=None):
        super().__init__(plates=() if plates is None else tuple(plates), dims=dims, name=name)

    def observe(self, x, mask=True):
        raise NotImplementedError('%s is a maximum-likelihood estimate: it cannot be observed'
                                  % type(self).__name__)

    def initialize_from_random(self):
        raise NotImplementedError('%s is a maximum-likelihood estimate: it has no distribution to '
                                  'draw from' % type(self).__name__)

    def initialize_from_parameters(self, *args):
        raise NotImplementedError('%s is a maximum-likelihood estimate: it has no parameters'
                                  % type(self).__name__)

    def random(self):
        raise NotImplementedError('%s is a maximum-likelihood estimate: it has no distribution to '
                                  'draw from' % type(self).__name__)


class GammaShape(_PointEstimate):
    """``GammaShape(m0=0, m1=0, plates=(), name=...)``: ML estimate of the shape of Gamma children;
    ``m0``, ``m1`` add to the children's messages (gamma.py:273-334)."""

    def __init__(self, m0=0, m1=0, plates=None, name=None):
        super().__init__(dims=((), ()), plates=plates, name=name)
        self._m0 = m0
        self._m1 = m1

    def _check_value_shape(self, x):
        a = np.asarray(x, dtype=np.float64)
        if np.any(a <= 0):
            raise ValueError("Shape parameter must be positive")
        super()._check_value_shape(a)


class Concentration(_PointEstimate):
    """``Concentration(D, regularization=True, plates=(), name=...)``: ML estimate of the
    concentration of Dirichlet / Beta children with D categories (dirichlet.py:234-330).
    ``regularization``: "prior" log-probability and "prior" sample number; ``True`` means
    ``[log(1/D), 1]``, ``None`` / ``False`` means ``[0, 0]``."""

    def __init__(self, D, regularization=True, plates=None, name=None):
        self.D = D
        super().__init__(dims=((D,), ()), plates=plates, name=name)
        if regularization is None or regularization is False:
            regularization = [0, 0]
        elif regularization is True:
            regularization = [np.log(1 / D), 1]
        self.regularization = regularization

    @property
    def regularization(self):
        return self._regularization

    @regularization.setter
    def regularization(self, regularization):
        if len(regularization) != 2:
            raise ValueError("Regularization must 2-tuple")
        if not is_shape_subset(np.shape(regularization[0]), self.get_shape(0)):
            raise ValueError("Wrong shape")
        if not is_shape_subset(np.shape(regularization[1]), self.get_shape(1)):
            raise ValueError("Wrong shape")
        self._regularization = regularization
        if self._plan is not None:
            # the estimate stays what it is, as in the reference; the next update and bound term
            # read the new regularization (a recorded sweep holding the old one is dropped)
            self._plan.invalidate(self, keep_state=True)

    def _check_value_shape(self, x):
        a = np.asarray(x, dtype=np.float64)
        if np.ndim(a) < 1:
            raise ValueError("The prior sample sizes must be a vector")
        if np.any(a < 0):
            raise ValueError("The prior sample sizes must be non-negative")
        super()._check_value_shape(a)


DirichletConcentration = Concentration


def BetaConcentration(**kwargs):
    """``Concentration(2)`` for Beta children (dirichlet.py: ``BetaConcentration``)."""
    return Concentration(2, **kwargs)
