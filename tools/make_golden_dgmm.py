#!/usr/bin/env python
"""
Fixtures of the diagonal-Gaussian-mixture scripts from the LIVE reference:
tests/golden/dgmm.npz.  Runs the model scripts of tests/dgmm_models.py on the reference, imported
the way oracle/make_golden.py imports it, and stores the inputs (in_*), the bound after every sweep,
every per-node bound term and the final moments of alpha, Z, mu and tau.

    python tools/make_golden_dgmm.py
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
    import dgmm_models
    g = dgmm_models.make_inputs(np.random.RandomState(4117))
    mods = dict(nodes=bayespy.nodes, VB=VB)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = dgmm_models.run_cases(mods, g)
    out = {'in_' + k: v for k, v in g.items()}
    for k, v in res.items():
        if not k.endswith('_plan'):
            out[k] = np.array(v)
    fn = os.path.join(OUT, 'dgmm.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])


if __name__ == '__main__':
    main()
