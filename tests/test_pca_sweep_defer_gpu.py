"""
The one-launch sweep forms <log tau>, <log alpha>, the bound, the ring slot and the stop rule in one
wavefront beside the next head's first inverse.  Against three launches per sweep, bitwise.

The scenarios are those of test_pca_sweep_one_launch_gpu.py, which holds their code and shares its
reference runs; the tests here are the ones of this file whose names and parameters are still true of
what they compare (the cases against a one-launch form that computed the bound in its tail went with
that form).  They stay only until they may be removed too.
"""
import pytest

import test_pca_sweep_one_launch_gpu as one
from test_pca_sweep_one_launch_gpu import (  # noqa: F401  (collected here under their own names)
    _restore_switches, test_early_stop_inside_a_chunk, test_stamps_of_the_side_wavefront,
    test_two_plans_with_different_priors_updated_alternately)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('ref', [one.THREE])
@pytest.mark.parametrize('D,K', one.DKS)
def test_update_of_12_equals(D, K, ref):
    assert ref == one.THREE                     # the reference of update_of_12
    one.update_of_12(D, K)


@pytest.mark.parametrize('D,K', [(128, 32), (40, 9)])
def test_two_calls_on_one_plan_in_chunks_of_5(D, K):
    one.two_calls_in_chunks_of_5(D, K)


def test_checkpoint_saved_and_loaded_is_identical(tmp_path):
    one.checkpoint_saved_and_loaded(tmp_path, 96, 20)
