"""
The one-launch sweep forms sum <x><x>^T in the workgroup that runs phase B, from the A and the rows
of sum y<x>^T it holds in LDS, and its kernels put the ticket words back to zero.  Against three
launches per sweep, bitwise.

The scenarios are those of test_pca_sweep_one_launch_gpu.py, which holds their code and shares its
reference runs; the tests here are the ones of this file whose names and parameters are still true of
what they compare (the cases against one-launch forms that stored partial blocks or ran the bodies
of the three-launch sweep went with those forms).  They stay only until they may be removed too.
"""
import pytest

import test_pca_sweep_one_launch_gpu as one
from test_pca_sweep_one_launch_gpu import (  # noqa: F401  (collected here under their own names)
    _restore_switches, test_early_stop_inside_a_chunk,
    test_two_calls_reuse_ticket_words_cleared_by_the_kernels)

pytestmark = pytest.mark.gpu

test_stamped_build_is_the_same_code_with_a_stamp_at_pxx_formed = \
    one.test_stamp_at_pxx_formed_and_none_at_partials_summed


@pytest.mark.parametrize('ref', [one.THREE])
@pytest.mark.parametrize('D,K', one.DKS)
def test_update_of_12_equals(D, K, ref):
    assert ref == one.THREE                     # the reference of update_of_12
    one.update_of_12(D, K)


def test_checkpoint_saved_and_loaded_is_identical(tmp_path):
    one.checkpoint_saved_and_loaded(tmp_path, 96, 20)
