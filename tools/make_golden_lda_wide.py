#!/usr/bin/env python
"""
Fixtures of the latent-Dirichlet-allocation model with more than 64 topics from the LIVE reference:
tests/golden/lda_wide.npz.  Runs the model script of tests/lda_wide_models.py on the reference,
imported the way oracle/make_golden.py imports it, and stores the inputs and initial moments
(in_*), and after every sweep the bound, every per-node bound term and the parameters of both
Dirichlet nodes.  Data only.

    python tools/make_golden_lda_wide.py
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
    from bayespy.inference.vmp.nodes.categorical import CategoricalMoments
    import lda_wide_models as wm
    g = wm.make_wide_inputs(np.random.RandomState(1311))
    mods = dict(nodes=bayespy.nodes, VB=VB, CategoricalMoments=CategoricalMoments,
                params=lambda Q, m: (m['p_topic'].phi[0], m['p_word'].phi[0]))
    out = {'in_' + k: v for k, v in g.items()}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for tag in wm.WIDE_CASES:
            for k, v in wm.run_wide_case(mods, g, tag).items():
                if not k.endswith(('_plan', '_model')):
                    out[k] = np.array(v)
    fn = os.path.join(OUT, 'lda_wide.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])


if __name__ == '__main__':
    main()
