#!/usr/bin/env python
"""
Fixture of the diagonal-Gaussian mixture under stochastic variational inference from the LIVE
reference: tests/golden/dgmm_svi.npz.  Runs the cases of tests/dgmm_svi_models.py on the reference,
imported the way oracle/make_golden.py imports it, and stores the inputs (data, the mini-batch index
sequences, the masks, the initial parameters) and, after every step, the bound, the five per-node
bound terms and the moments of mu, tau and the weights; Z.u[0] of the last mini-batch.

    python tools/make_golden_dgmm_svi.py
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
    import dgmm_svi_models as M
    g = M.make_inputs(np.random.RandomState(9127))
    mods = dict(nodes=bayespy.nodes, VB=VB)
    out = dict(g)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for tag in M.CASES:
            for k, v in M.run_case(mods, g, tag).items():
                if not k.endswith('_plan'):
                    out[k] = np.array(v)
    fn = os.path.join(OUT, 'dgmm_svi.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for tag in M.CASES:
        print(tag, out[tag + '_L'])
        print(tag, 'terms of the last step', out[tag + '_terms'][-1])
        assert all(np.all(np.isfinite(out[tag + '_' + k])) for k in ('L', 'terms') + M.MOMENTS)


if __name__ == '__main__':
    main()
