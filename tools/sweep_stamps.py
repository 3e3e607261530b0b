#!/usr/bin/env python
"""Where the time goes inside one launch of pca_sweep_mid_kernel: per-phase medians from the
wall_clock64 stamps of the stamped build (tune key "pca_sweep_stamps").

    python tools/sweep_stamps.py [--D 128] [--K 32] [--N 4096] [--chunks 5]

Runs chunks of 32 sweeps (31 mid launches each) of the PCA demo model at the headline's (D, K) with a
small N, reads the stamps of each chunk and prints the median over all launches of every phase, in
microseconds.  wall_clock64 counts a constant 100 MHz clock, so one tick is 10 ns and a phase of a
few microseconds is resolved to a few per cent.  A stamp is one clock read and one store to LDS by
one lane; that this costs well under a tick is assumed, not measured (the stamped kernel's own
duration has not been set against the default kernel's).
The rows are those of enum SP_*, which keeps the boundaries of forms the kernel no longer has so that
earlier records stay comparable: the tail forms sum <x><x>^T from LDS after its loads have landed
('tail: Pxx formed') and adds no stored partial blocks, so 'tail: partials summed' is not passed and
prints '-'; 'A: Pxx stored' is the end of phase A.  The tail hands over to the head once the means of
tau and alpha are ready: the three boundaries behind 'tail: block sums done' are stamped together
there.  The stamped build runs at "pca_sweep_stamps" = 2, where the side wavefront -- which forms the
bound, the ring slot and the stop word beside the head's first inverse -- stamps too.  Its two
boundaries are printed since kernel entry, with whether the side work ends before 'head: inverse 1
done'.  The last column is the least and the greatest length of each phase over the launches.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TICK_US = 1.0 / 100.0            # 100 MHz
# (name of the boundary, in the order of enum SP_* in csrc/vmp_pca_small.hip)
NAMES = ['kernel entry', 'A: LDS filled', 'A: Syx done', 'A: Pxx stored', 'ticket drawn', 'acquire done',
         'tail: partials summed', 'tail: loads landed', 'tail: Pxx formed', 'tail: block sums done',
         'tail: tau/alpha done',
         'tail: bound done', 'tail: ring written',
         'head: Lambda_W built', 'head: inverse 1 done', 'head: W done', 'head: Sww done',
         'head: inverse 2 done', 'head: A stored']
SIDE = ['side: tau/alpha state stored', 'side: ring and stop written']      # words 19 and 20 of a row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--D', type=int, default=128)
    ap.add_argument('--K', type=int, default=32)
    ap.add_argument('--N', type=int, default=4096)
    ap.add_argument('--chunks', type=int, default=5)
    a = ap.parse_args()
    from bayespy_amd import nodes
    from bayespy_amd.device import get_runtime
    from bayespy_amd.inference import VB
    rt = get_runtime()
    rt.check(rt.lib.vmp_tune_set(b'pca_sweep_stamps', 2))
    rng = np.random.default_rng(0)
    y = rng.standard_normal((a.D, a.K)) @ rng.standard_normal((a.K, a.N)) \
        + 0.1 * rng.standard_normal((a.D, a.N))
    alpha = nodes.Gamma(1e-2, 1e-2, plates=(a.K,), name='alpha')
    W = nodes.GaussianARD(0, alpha, shape=(a.K,), plates=(a.D, 1), name='W')
    X = nodes.GaussianARD(0, 1, shape=(a.K,), plates=(1, a.N), name='X')
    F = nodes.SumMultiply('i,i', W, X, name='F')
    tau = nodes.Gamma(1e-2, 1e-2, name='tau')
    Y = nodes.GaussianARD(F, tau, name='Y')
    X.initialize_from_value(rng.standard_normal((1, a.N, a.K)))
    Y.observe(y)
    Q = VB(Y, F, W, X, tau, alpha)
    Q.ignore_bound_checks = True
    plan = Q.plans[0]
    plan.sweep_chunk = 32
    Q.update(repeat=1, verbose=False)                  # the first sweep runs node by node
    rows = []
    for _ in range(a.chunks + 1):
        Q.update(repeat=32, verbose=False)
        r, allocated = plan.kernels.sweep_stamps()
        assert allocated and r.shape[0] == 31, r.shape
        rows.append(r[:, :len(NAMES) + len(SIDE)].astype(np.int64))
    t = np.concatenate(rows[1:])                       # (the first chunk warms up)
    print('pca_sweep_mid_kernel stamps: D=%d K=%d N=%d, %d launches' % (a.D, a.K, a.N, t.shape[0]))
    print('wall_clock64 at a constant 100 MHz: 1 tick = 0.01 us; medians over the launches')
    print('%-28s %10s %12s %14s' % ('boundary', 'phase_us', 'since_entry', 'phase min-max'))
    prev = t[:, 0]
    ix = {name: i for i, name in enumerate(NAMES)}
    for i, name in enumerate(NAMES):
        have = t[:, i] != 0
        if not have.all():
            print('%-28s %10s %12s' % (name, '-', '-'))
            continue
        print('%-28s %10.2f %12.2f %7.2f-%.2f' % (name, np.median(t[:, i] - prev) * TICK_US,
                                                  np.median(t[:, i] - t[:, 0]) * TICK_US,
                                                  (t[:, i] - prev).min() * TICK_US,
                                                  (t[:, i] - prev).max() * TICK_US))
        prev = t[:, i]
    print('phase A (entry -> ticket) %.2f | tail (acquire -> ring) %.2f | head (ring -> A stored) %.2f us'
          % tuple(np.median(x) * TICK_US for x in
                  (t[:, ix['ticket drawn']] - t[:, 0],
                   t[:, ix['tail: ring written']] - t[:, ix['acquire done']],
                   t[:, ix['head: A stored']] - t[:, ix['tail: ring written']])))
    total = (t[:, ix['head: A stored']] - t[:, 0]) * TICK_US
    print('entry -> A stored %.2f us (min %.2f, max %.2f)' % (np.median(total), total.min(), total.max()))
    inv1 = t[:, ix['head: inverse 1 done']]
    for i, name in enumerate(SIDE):
        print('%-28s %10s %12.2f' % (name, '', np.median(t[:, len(NAMES) + i] - t[:, 0]) * TICK_US))
    slack = inv1 - t[:, len(NAMES) + 1]
    print("side work ends before 'head: inverse 1 done' in %d of %d launches; slack median %.2f, "
          'min %.2f us' % (int((slack >= 0).sum()), slack.size, np.median(slack) * TICK_US,
                           slack.min() * TICK_US))


if __name__ == '__main__':
    main()
