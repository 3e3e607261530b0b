#!/usr/bin/env python
"""
Fixtures of the maximum-likelihood nodes (GammaShape, Concentration) from the LIVE reference:
tests/golden/ml_nodes.npz.  Runs the model scripts of tests/ml_models.py on the reference, imported
the way oracle/make_golden.py imports it, and stores the inputs (in_*), the bound after every sweep
and the final moments.

    python tools/make_golden_ml.py
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
    import ml_models
    g = ml_models.make_ml_inputs(np.random.RandomState(5150))
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = ml_models.run_ml_cases(bayespy.nodes, VB, g)
    out = {'in_' + k: v for k, v in g.items()}
    for k, v in res.items():
        if isinstance(v, list):
            for i, vi in enumerate(v):
                out['%s_%d' % (k, i)] = np.array(vi)
        else:
            out[k] = np.array(v)
    fn = os.path.join(OUT, 'ml_nodes.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k][:3], '...', out[k][-1])
    print('gamma-shape demo: a = %.4f, b = %.4f' % (out['gs_a_u_0'], out['gs_b_u_0']))


if __name__ == '__main__':
    main()
