#!/usr/bin/env python
"""
Fixture of the count-mixture models under stochastic variational inference from the LIVE reference:
tests/golden/mix_svi.npz.  Runs the model scripts of tests/mix_svi_models.py on the reference,
imported the way oracle/make_golden.py imports it, and stores the inputs (data, the mini-batch index
sequences, the masks, the trials, the initial parameters) and, after every step, the bound, the
per-node bound terms and the moments of the parameter node and the weights; Z.u[0] of the last
mini-batch.

    python tools/make_golden_mix_svi.py
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
    import mix_svi_models as M
    g = M.make_inputs(np.random.RandomState(7411))
    mods = dict(nodes=bayespy.nodes, VB=VB)
    out = dict(g)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for tag in M.CASES:
            for k, v in M.run_case(mods, g, tag).items():
                if not k.endswith('_plan'):
                    out[k] = np.array(v)
    fn = os.path.join(OUT, 'mix_svi.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for tag in M.CASES:
        print(tag, out[tag + '_L'])


if __name__ == '__main__':
    main()
