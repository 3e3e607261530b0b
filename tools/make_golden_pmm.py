#!/usr/bin/env python
"""
Fixtures of the Poisson-mixture (count clustering) models from the LIVE reference:
tests/golden/pmm.npz.  Runs the model scripts of tests/pmm_models.py on the reference, imported the
way oracle/make_golden.py imports it, and stores the inputs (in_*), the bound after every sweep,
every per-node bound term, the final moments of R, lam and Z and the masks of Z and lam.  Case (g),
a mask of ones, must reproduce case (a).

    python tools/make_golden_pmm.py
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
    import pmm_models
    g = pmm_models.make_pmm_inputs(np.random.RandomState(4119))
    assert g['e_x'].max() > 3000 and g['e_x'].max() <= 65534
    mods = dict(nodes=bayespy.nodes, VB=VB)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = pmm_models.run_pmm_cases(mods, g)
    X = res['a_plan']['X']
    assert X.plates == (300, 7) and res['a_lam_u0'].shape == (7, 3)
    assert res['f_Z_mask'].shape == (300, 1) and res['f_lam_mask'].shape == (7, 1)
    for k in res:
        if k.startswith('g_') and not k.endswith(('_plan', '_mask')):
            np.testing.assert_allclose(res[k], res['a_' + k[2:]], rtol=1e-12, atol=1e-12, err_msg=k)
    out = {'in_' + k: (v.astype(np.int32) if k.endswith('_x') else v) for k, v in g.items()}
    for k, v in res.items():
        if not k.endswith('_plan'):
            out[k] = np.array(v)
    fn = os.path.join(OUT, 'pmm.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])


if __name__ == '__main__':
    main()
