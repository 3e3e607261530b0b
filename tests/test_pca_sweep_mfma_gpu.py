"""
The one-launch sweep runs the chains of sum y<x>^T and the partials of sum <x><x>^T on the matrix
cores (test_mfma_order_gpu.py pins the order in which they add).  Against three launches per sweep,
which is scalar code, bitwise.

The scenarios are those of test_pca_sweep_one_launch_gpu.py, which holds their code and shares its
reference runs; the tests here are the ones of this file whose names and parameters are still true of
what they compare (the cases against scalar chains inside the one launch, and phase A against forms
of vmp_pca_gram_stats_form that are gone, went with those forms).  They stay only until they may be
removed too.
"""
import pytest

import test_pca_sweep_one_launch_gpu as one
from test_pca_sweep_one_launch_gpu import (  # noqa: F401  (collected here under their own names)
    _restore_switches, test_early_stop_inside_a_chunk)

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


def test_stamped_build():
    """"pca_sweep_stamps" = 2: every row holds the 18 stamps of the workgroup that ran phase B in
    ascending order."""
    one.rows_hold_18_stamps_ascending(2)
