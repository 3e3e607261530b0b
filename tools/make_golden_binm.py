#!/usr/bin/env python
"""
Fixtures of the binomial-mixture (successes out of trials) models from the LIVE reference:
tests/golden/binm.npz.  Runs the model scripts of tests/binm_models.py on the reference, imported the
way oracle/make_golden.py imports it, and stores the inputs (in_*), the bound after every sweep,
every per-node bound term, the final moments of R, P and Z and the masks of Z and P.  Cases (g) and
(h), a mask of ones and the scalar mask True, must reproduce case (a).

    python tools/make_golden_binm.py
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
    import binm_models
    g = binm_models.make_binm_inputs(np.random.RandomState(5227))
    assert (g['d_n'] == 0).any() and g['e_n'].max() > 2000
    mods = dict(nodes=bayespy.nodes, VB=VB)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        res = binm_models.run_binm_cases(mods, g)
    X = res['a_plan']['X']
    assert X.plates == (300, 7) and res['a_P_u0'].shape == (7, 3, 2)
    assert res['f_Z_mask'].shape == (60, 1) and res['f_P_mask'].shape == (4, 1)
    for tag in 'gh':
        for k in res:
            if k.startswith(tag + '_') and not k.endswith(('_plan', '_mask')):
                np.testing.assert_allclose(res[k], res['a_' + k[2:]], rtol=1e-12, atol=1e-12,
                                           err_msg=k)
    for tag in binm_models.CASES:       # no case sits at the symmetric fixed point
        r = res[tag + '_Z_u0'].reshape(-1, res[tag + '_Z_u0'].shape[-1])
        assert r.shape[1] == 1 or np.ptp(r.mean(axis=0)) > 1e-3, tag
    out = {'in_' + k: (v.astype(np.int32) if k.endswith(('_x', '_n')) else v)
           for k, v in g.items()}
    for k, v in res.items():
        if not k.endswith('_plan'):
            out[k] = np.array(v)
    fn = os.path.join(OUT, 'binm.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])


if __name__ == '__main__':
    main()
