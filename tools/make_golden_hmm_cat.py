#!/usr/bin/env python
"""
Fixtures of the discrete hidden-Markov-model scripts from the LIVE reference:
tests/golden/hmm_cat.npz.  Runs the model scripts of tests/hmm_cat_models.py on the reference,
imported the way oracle/make_golden.py imports it, and stores the inputs (in_*; a valid word, 0,
at every masked position of y: the reference checks the words whatever the mask says), the bound
after every sweep, every per-node bound term, the final moments of Z and of the learned roles
among P, A and a0 and, with a mask, the masks of Z and Y.

    python tools/make_golden_hmm_cat.py
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
    import hmm_cat_models
    g = hmm_cat_models.make_inputs(np.random.RandomState(4117))
    mods = dict(nodes=bayespy.nodes, VB=VB)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = hmm_cat_models.run_cases(mods, g)
    out = {'in_' + k: v for k, v in g.items()}
    for k, v in res.items():
        if not k.endswith('_plan') and not k.endswith('_model'):
            out[k] = np.array(v)
    fn = os.path.join(OUT, 'hmm_cat.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L') or k.endswith('_Z_mask'):
            print(k, out[k])


if __name__ == '__main__':
    main()
