#!/usr/bin/env python
"""
Fixture of the wide-emission hidden-Markov-model scripts from the LIVE reference:
tests/golden/hmm_wide.npz.  Runs tests/hmm_wide_models.py on the reference, imported the way
oracle/make_golden.py imports it, and stores the inputs (in_*; NaN at every masked position of y),
the bound after every sweep and the final moments of Z, A and a0 (form (b): mu and Lambda too).

    python tools/make_golden_hmm_wide.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    from oracle.make_golden import _import_reference, OUT
    _import_reference()
    import bayespy.nodes
    from bayespy.inference import VB
    import hmm_wide_models
    g = hmm_wide_models.make_inputs(np.random.RandomState(4117))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = hmm_wide_models.run_cases(dict(nodes=bayespy.nodes, VB=VB), g)
    out = {'in_' + k: v for k, v in g.items()}
    out.update({k: np.array(v) for k, v in res.items() if not k.endswith('_plan')})
    fn = os.path.join(OUT, 'hmm_wide.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])


if __name__ == '__main__':
    main()
