#!/usr/bin/env python
"""
Fixtures of the diagonal-Gaussian-mixture models with missing observations from the LIVE
reference: tests/golden/dgmm_masked.npz.  Runs the model scripts of tests/dgmm_masked_models.py on
the reference, imported the way oracle/make_golden.py imports it, and stores the inputs (in_*, y
with NaN at the hidden positions), the bound after every sweep, every per-node bound term, the
final moments of alpha, Z, mu and tau and the masks of Z and mu.  The data come from
tests/golden/dgmm.npz; case (d), a mask of ones, must reproduce its case a.

    python tools/make_golden_dgmm_masked.py
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
    import dgmm_masked_models as models
    plain = np.load(os.path.join(OUT, 'dgmm.npz'))
    g = models.make_masked_inputs(np.random.RandomState(4118),
                                  {k[3:]: plain[k] for k in plain.files if k.startswith('in_')})
    mods = dict(nodes=bayespy.nodes, VB=VB)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = models.run_masked_cases(mods, g)
    out = {'in_' + k: v for k, v in g.items()}
    for k, v in res.items():
        if not k.endswith('_plan'):
            out[k] = np.array(v)
    np.testing.assert_allclose(out['d_L'], plain['a_L'], rtol=1e-12)
    fn = os.path.join(OUT, 'dgmm_masked.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])
    for tag in models.CASES:
        Q = res[tag + '_plan']
        print(tag, 'masks: Z', out[tag + '_Z_mask'].shape, int(out[tag + '_Z_mask'].sum()),
              'mu', out[tag + '_mu_mask'].shape, int(out[tag + '_mu_mask'].sum()),
              'tau', np.shape(Q['tau'].mask), 'alpha', np.shape(Q['alpha'].mask))


if __name__ == '__main__':
    main()
