#!/usr/bin/env python
"""
Fixtures of the multinomial-mixture (count-vector clustering) models from the LIVE reference:
tests/golden/mmm.npz.  Runs the model scripts of tests/mmm_models.py on the reference, imported the
way oracle/make_golden.py imports it, and stores the inputs (in_*), the bound after every sweep,
every per-node bound term and the final moments of R, P and Z.

    python tools/make_golden_mmm.py
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
    import mmm_models
    g = mmm_models.make_mmm_inputs(np.random.RandomState(5231))
    assert g['e_x'].max() > 3000 and g['e_x'].max() <= 65534
    mods = dict(nodes=bayespy.nodes, VB=VB)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = mmm_models.run_mmm_cases(mods, g)
    Q = res['a_plan']
    assert Q['X'].plates == (300,) and Q['Z'].plates == (300,) and Q['P'].plates == (3,)
    assert [type(p).__name__ for p in Q['X'].parents] == ['Categorical', 'Dirichlet']
    assert res['a_P_u0'].shape == (3, 7) and res['a_Z_u0'].shape == (300, 3)
    out = {'in_' + k: (v.astype(np.int32) if k.endswith('_x') else v) for k, v in g.items()}
    for k, v in res.items():
        if not k.endswith('_plan'):
            out[k] = np.array(v)
    fn = os.path.join(OUT, 'mmm.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])


if __name__ == '__main__':
    main()
