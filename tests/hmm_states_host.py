"""TEST INFRASTRUCTURE of tests/test_hmm_states_gpu.py: the inputs.  The long-double restatement
and the allowance rule are ``hmm_mult_host.restate`` / ``compare``, as they are."""
import numpy as np

from hmm_mult_host import ALL, SUMS, compare  # noqa: F401
import hmm_mult_host as mult


def pass_inputs(B, T, M, K, band=False):
    """(x, Pt, la0, lA) of ``hmm_mult_host.pass_inputs`` (Dirichlet digamma tables); ``band``: a
    left-to-right chain, -inf in <log A> outside i <= j <= i + 3 and in <log a0> past state 3."""
    x, Pt, la0, lA = mult.pass_inputs(B, T, M, K)
    if band:
        i, j = np.indices((K, K))
        lA = np.where((j >= i) & (j <= i + 3), lA, -np.inf)
        lA[K - 1, K - 1] = 0.0      # the last state absorbs
        la0 = np.where(np.arange(K) < 4, la0, -np.inf)
    return x, Pt, la0, lA
