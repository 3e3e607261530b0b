"""``bayespy_amd.inference.vmp.nodes`` -- import-path mirror of ``bayespy.inference.vmp.nodes``:
the node classes of :mod:`bayespy_amd.nodes` under the reference's long module path, for scripts
that import helper classes from there (doc/source/examples/lda.rst:100 imports
``CategoricalMoments`` from ``...vmp.nodes.categorical``)."""
from ....nodes import *                 # noqa: F401,F403
from ....nodes import __all__           # noqa: F401
