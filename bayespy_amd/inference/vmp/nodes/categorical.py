"""Import-path mirror of ``bayespy.inference.vmp.nodes.categorical``."""
from ....nodes.categorical import Categorical, CategoricalMoments      # noqa: F401
