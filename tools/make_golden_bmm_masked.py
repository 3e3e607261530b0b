#!/usr/bin/env python
"""
Fixtures of the Bernoulli-mixture models with missing observations from the LIVE reference:
tests/golden/bmm_masked.npz.  Runs the model scripts of tests/bmm_masked_models.py on the
reference, imported the way oracle/make_golden.py imports it, and stores the inputs (in_*, x with
NaN at the hidden positions), the bound after every sweep, every per-node bound term, the final
moments of R, P and Z and ``Z.mask``.  Case (d), a mask of ones, uses the data of case a of
tests/golden/bmm_fused.npz.

    python tools/make_golden_bmm_masked.py
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
    import bmm_masked_models as models
    fused = np.load(os.path.join(OUT, 'bmm_fused.npz'))
    g = models.make_masked_inputs(np.random.RandomState(7311),
                                  {k[3:]: fused[k] for k in fused.files if k.startswith('in_')})
    mods = dict(nodes=bayespy.nodes, VB=VB)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = models.run_masked_cases(mods, g)
    out = {'in_' + k: v for k, v in g.items()}
    for k, v in res.items():
        if not k.endswith('_plan'):
            out[k] = np.array(v)
    fn = os.path.join(OUT, 'bmm_masked.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])
    for tag in models.CASES:
        Q = res[tag + '_plan']
        print(tag, 'masks: Z', out[tag + '_Z_mask'].shape, int(out[tag + '_Z_mask'].sum()),
              'P', np.shape(Q['P'].mask), 'R', np.shape(Q['R'].mask), np.all(Q['R'].mask))
    np.testing.assert_allclose(out['d_L'][:4], fused['a_L'], rtol=1e-12)


if __name__ == '__main__':
    main()
