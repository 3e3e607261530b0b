#!/usr/bin/env python
"""Chain summary of one rocprofv3 kernel trace (rocpd sqlite) of `bench.py --steps N`: per-kernel
calls / mean / min of the replicated-node chain over the timed region, launches per sweep, and the
gap from one sweep's end to the next one's start.

    python tools/chain_summary.py <results.db> <steps> [<below_us>]

With <below_us> (the other build's shortest one-launch sweep) the distribution of the one-launch sweeps
is printed as well: deciles and how many launches are shorter than that.
"""
import re
import sqlite3
import sys
from collections import defaultdict


def short(name):
    name = re.sub(r'\(anonymous namespace\)::', '', name)
    name = re.sub(r'^void ', '', name)
    m = re.match(r'([A-Za-z0-9_:]+(<[0-9a-z, ]+>)?)', name)
    return (m.group(1) if m else name)[:60]


ENDERS = ('pca_tail_sweep_kernel', 'pca_sweep_mid_kernel')      # the kernel that ends a sweep
PASSES = ('pca_xpass', 'pca_pass')


def main(db, steps, below=None):
    """The window is the timed region of `bench.py --steps <steps>`: every pca_* launch that starts
    after the end of the last sweep BEFORE the final `steps` sweeps (the last warm-up sweep), so
    set-up and warm-up launches are left out and parent and change are cut the same way."""
    con = sqlite3.connect(db)
    cols = [r[1] for r in con.execute("pragma table_info('kernels')").fetchall()]
    if 'end' in cols:
        rows = con.execute('select name, start, "end" from kernels order by start').fetchall()
    else:
        rows = [(n, s, s + d) for n, s, d in
                con.execute('select name, start, duration from kernels order by start').fetchall()]
    chain = [(short(n), s, e) for n, s, e in rows if short(n).startswith('pca_')]
    ends = [e for n, s, e in chain if n.startswith(ENDERS)]
    if len(ends) <= steps:
        raise SystemExit('only %d sweeps in the trace, %d asked for' % (len(ends), steps))
    t_begin = ends[-steps - 1]
    win = [r for r in chain if r[1] >= t_begin]
    agg = defaultdict(list)
    for n, s, e in win:
        agg[n].append((e - s) / 1e3)
    print('timed region: the last %d sweeps, %d pca_* launches' % (steps, len(win)))
    print('%-52s %6s %10s %10s %10s' % ('kernel', 'calls', 'mean_us', 'min_us', 'max_us'))
    for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        print('%-52s %6d %10.2f %10.2f %10.2f' % (k, len(v), sum(v) / len(v), min(v), max(v)))
    mid = sorted(d for k, v in agg.items() if k.startswith('pca_sweep_mid_kernel') for d in v)
    if mid:
        q = lambda f: mid[min(len(mid) - 1, int(f * len(mid)))]
        print('pca_sweep_mid_kernel durations: p10 %.2f median %.2f p90 %.2f us'
              % (q(0.1), q(0.5), q(0.9)))
        if below is not None:
            print('pca_sweep_mid_kernel launches shorter than %.2f us: %d of %d'
                  % (below, sum(1 for d in mid if d < below), len(mid)))
    small = [r for r in win if not r[0].startswith(PASSES)]
    # gap: the end of a sweep to the start of the next small kernel; period: sweep end to sweep end
    gaps, periods, prev_end = [], [], t_begin
    for i, (n, s, e) in enumerate(small):
        if n.startswith(ENDERS):
            periods.append((e - prev_end) / 1e3)
            prev_end = e
            if i + 1 < len(small):
                gaps.append((small[i + 1][1] - e) / 1e3)
    for name, v in (('gap, sweep end -> next chain kernel start', gaps),
                    ('sweep period (end to end)', periods)):
        v = sorted(v)
        print('%s: n=%d median %.2f us min %.2f us max %.2f us'
              % (name, len(v), v[len(v) // 2], v[0], v[-1]))
    print('launches per sweep (head, Gram statistics, tail and mid launches / sweeps): %d / %d = %.2f'
          % (len(small), steps, len(small) / steps))
    print('first 24 launches of the region (name, start_us, dur_us):')
    for n, s, e in win[:24]:
        print('  %-52s %10.1f %8.2f' % (n, (s - t_begin) / 1e3, (e - s) / 1e3))


if __name__ == '__main__':
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 200,
         float(sys.argv[3]) if len(sys.argv) > 3 else None)
