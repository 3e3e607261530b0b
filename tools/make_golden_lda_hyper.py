#!/usr/bin/env python
"""
Fixtures of the latent-Dirichlet-allocation model with learnt concentrations from the LIVE
reference: tests/golden/lda_hyper.npz.  Runs the model script of tests/lda_hyper_models.py on the
reference, imported the way oracle/make_golden.py imports it, and stores the inputs and initial
moments (in_*), the initial moments of every concentration node, and after every sweep the bound,
every per-node bound term, the parameters of both Dirichlet nodes and the moments of every
concentration.  Data only.

The fixed point of a concentration stops when no element moved by more than 1e-5 relative; a last-bit
difference in the children's message can move the stopping iteration by one only if a movement lies
at the threshold.  For every concentration update the generator repeats the reference's iteration on
the very messages the node received and prints the largest relative movement of the step that
stopped it and of the step before.  The iteration converges linearly (each movement is 0.75 to 0.99
of the one before), so the two figures always straddle 1e-5 within that ratio and no case can keep
both a factor of 10 away; what a case must keep is a relative distance of MARGIN = 1e-3 from 1e-5 on
either side.  A last-bit difference in the message moves a movement by about 1e-13 relative, ten
orders of magnitude less; a case that comes closer is refused.

    python tools/make_golden_lda_hyper.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

THRESHOLD, MARGIN = 1e-5, 1e-3


def _movements(node, m):
    """(movement of the stopping step, movement of the step before, steps) of the node's fixed point
    on the messages ``m``: the restatement of tests/ml_host.py stopped at its last three steps."""
    from ml_host import concentration_fixed_point
    r0, r1 = np.asarray(node.regularization[0], dtype=float), np.asarray(node.regularization[1],
                                                                         dtype=float)
    m0, m1 = np.asarray(m[0], dtype=float), np.asarray(m[1], dtype=float)
    _, n, capped = concentration_fixed_point(m0, m1, r0, r1, max_iter=10 ** 6)
    assert not capped and n >= 2
    a = [concentration_fixed_point(m0, m1, r0, r1, max_iter=k)[0] for k in (n - 2, n - 1, n)]
    move = [float(np.max(np.abs((y - x) / y))) for x, y in zip(a[:-1], a[1:])]
    return move[1], move[0], n


def main():
    from oracle.make_golden import _import_reference, OUT
    _import_reference()
    import bayespy.nodes
    from bayespy.inference import VB
    from bayespy.inference.vmp.nodes.categorical import CategoricalMoments
    from bayespy.inference.vmp.nodes.dirichlet import Concentration
    import lda_hyper_models as hm

    figures = []
    inner = Concentration._update_distribution_and_lowerbound

    def recording(self, m):
        figures.append((self.name,) + _movements(self, m))
        return inner(self, m)
    Concentration._update_distribution_and_lowerbound = recording

    g = hm.make_hyper_inputs(np.random.RandomState(1413))
    mods = dict(nodes=bayespy.nodes, VB=VB, CategoricalMoments=CategoricalMoments,
                params=lambda Q, m: (m['p_topic'].phi[0], m['p_word'].phi[0]))
    out = {'in_' + k: v for k, v in g.items()}
    refused = []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for tag in hm.HYPER_CASES:
            del figures[:]
            res = hm.run_hyper_case(mods, g, tag)
            for name, last, before, its in figures:
                ok = last < THRESHOLD * (1 - MARGIN) and before > THRESHOLD * (1 + MARGIN)
                print('%-6s %-10s %6d steps  stopping movement %.3e  the one before %.3e  %s'
                      % (tag, name, its, last, before, 'ok' if ok else 'REFUSED'))
                if not ok:
                    refused.append((tag, name, last, before))
            for k, v in res.items():
                if not k.endswith(('_plan', '_model')):
                    out[k] = np.array(v)
    if refused:
        raise SystemExit('refused: a movement within a relative %g of %g: %s'
                         % (MARGIN, THRESHOLD, refused))
    fn = os.path.join(OUT, 'lda_hyper.npz')
    np.savez_compressed(fn, **out)
    print(fn, os.path.getsize(fn), 'bytes')
    for k in sorted(out):
        if k.endswith('_L'):
            print(k, out[k])


if __name__ == '__main__':
    main()
