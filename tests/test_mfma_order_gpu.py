"""
In which order do the two fp64 matrix instructions add the four products of an output?

v_mfma_f64_16x16x4_f64 and v_mfma_f64_4x4x4_4b_f64 compute d = a0 b0 + a1 b1 + a2 b2 + a3 b3 + c per
output.  The kernels that must keep bits when a scalar chain of fused multiply-adds moves onto the
matrix cores (csrc/vmp_pca_small.hip) need to know HOW: this test runs single instructions through
vmp_mfma_order_probe on tiles chosen on the host and compares the bits with every candidate,
evaluated exactly on the CPU (rational arithmetic, one correct rounding per operation):

    chain from C, slots p        fma(a_p3, b_p3, fma(a_p2, b_p2, fma(a_p1, b_p1, fma(a_p0, b_p0, c))))
                                 for all 24 orders p of the four k-slots
    chain from 0, slots p, + C   the same chain started at +0.0, c added last (24 orders)
    unfused from C, slots p      rounded products, added to c one at a time (24 orders)
    pairwise tree, fused         (fma(a0, b0, rn(a1 b1)) + fma(a2, b2, rn(a3 b3))) + c
    pairwise tree, unfused       ((rn(a0 b0) + rn(a1 b1)) + (rn(a2 b2) + rn(a3 b3))) + c
    exact                        the exact sum, rounded once

Before any GPU run the test asserts that these 75 candidates are pairwise distinct on the chosen
inputs: for every two of them there is an output on which they differ, so at most one candidate can
match the hardware on all outputs.  (On an output with c = +0.0 a chain from C and the chain from 0 of
the same order are the same expression; those outputs are there because the sweeps start their
chains at 0.0, and they take part in the match, not in telling these two families apart.)  The test
fails unless exactly one candidate matches every output, and names it.

Inputs per form: tiles of full random mantissas with exponents a few binades apart (every addition
rounds), tiles with exponents up to 2^+-30 apart (absorption), and adversarial tiles in which the
first two products cancel to 40 bits, with c = +0.0 on half of the outputs, and tiles at the bottom
of the range -- subnormal operands, products of normal operands that are subnormal, subnormal c and
results, where a flush to zero anywhere in the instruction would show: 1280 and 1024 outputs.

FINDING (MI355X): both instructions are the chain from C over the k-slots in ascending order,
every step fused: EXPECT below.
"""
import functools
import itertools
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXPECT = 'chain from C, slots 0123'


def _fma(x, y, z):
    return float(Fraction(x) * Fraction(y) + Fraction(z))


def _add(x, y):
    return float(Fraction(x) + Fraction(y))


def _mul(x, y):
    return float(Fraction(x) * Fraction(y))


PERMS = list(itertools.permutations(range(4)))


def candidates(a, b, c):
    """name -> value for one output: a, b four floats each, c a float"""
    out = {}
    p = [_mul(a[k], b[k]) for k in range(4)]
    for perm in PERMS:
        tag = ''.join(map(str, perm))
        s = c
        z = 0.0
        u = c
        for k in perm:
            s = _fma(a[k], b[k], s)
            z = _fma(a[k], b[k], z)
            u = _add(u, p[k])
        out['chain from C, slots ' + tag] = s
        out['chain from 0, slots %s, + C' % tag] = _add(z, c)
        out['unfused from C, slots ' + tag] = u
    out['pairwise tree, fused'] = _add(_add(_fma(a[0], b[0], p[1]), _fma(a[2], b[2], p[3])), c)
    out['pairwise tree, unfused'] = _add(_add(_add(p[0], p[1]), _add(p[2], p[3])), c)
    out['exact'] = float(sum((Fraction(a[k]) * Fraction(b[k]) for k in range(4)), Fraction(c)))
    return out


def _rand(rng, shape, spread, base=0):
    m = 1.0 + rng.random(shape)
    e = base + rng.integers(-spread, spread + 1, shape)
    s = rng.choice([-1.0, 1.0], shape)
    return s * np.ldexp(m, e)


def _tiles(form, seed):
    """A (T, M, 4), B (T, 4, Nn), C (T, M, Nn) with M = Nn = 16 (form 0: five tiles, one of each
    kind) or T counting blocks of M = Nn = 4 (form 1: 64 blocks, 16 of each of the first three kinds
    and 8 of each of the last two)"""
    rng = np.random.default_rng(seed)
    M = 16 if form == 0 else 4
    kinds = [0, 1, 2, 3, 4] if form == 0 else [0] * 16 + [1] * 16 + [2] * 16 + [3] * 8 + [4] * 8
    T = len(kinds)
    A = np.empty((T, M, 4))
    B = np.empty((T, 4, M))
    C = np.empty((T, M, M))
    for t, kind in enumerate(kinds):
        if kind == 0:                       # every addition rounds
            A[t], B[t], C[t] = _rand(rng, (M, 4), 2), _rand(rng, (4, M), 2), _rand(rng, (M, M), 3)
        elif kind == 1:                     # absorption
            A[t], B[t], C[t] = _rand(rng, (M, 4), 15), _rand(rng, (4, M), 15), _rand(rng, (M, M), 30)
        elif kind == 3:
            # subnormal operands in A (2^-1040: 34 bits left), subnormal products, sums and C
            A[t], B[t] = _rand(rng, (M, 4), 2, -1040), _rand(rng, (4, M), 3, 8)
            C[t] = _rand(rng, (M, M), 4, -1032)
        elif kind == 4:
            # normal operands whose products (106 bits at 2^-1030) and sums are subnormal
            A[t], B[t] = _rand(rng, (M, 4), 2, -515), _rand(rng, (4, M), 2, -515)
            C[t] = _rand(rng, (M, M), 4, -1030)
        else:                               # products 0 and 1 of opposite sign, equal to 40 bits
            A[t], B[t] = _rand(rng, (M, 4), 1), _rand(rng, (4, M), 1)
            A[t][:, 1] = -A[t][:, 0] * (1.0 + np.ldexp(1.0 + rng.random(M), -40))
            B[t][1, :] = B[t][0, :]
            # the other two products a few binades below the first two
            A[t][:, 2:] *= 2.0 ** -3
            C[t] = _rand(rng, (M, M), 2) * 2.0 ** -6
            C[t][rng.random((M, M)) < 0.5] = 0.0       # +0.0
    return A, B, C


@functools.lru_cache(maxsize=None)
def _cpu(form):
    """(A, B, C, names, table): table[i] the candidates' values on all outputs, in the order of C.ravel()"""
    A, B, C = _tiles(form, 20240 + form)
    T, M, _ = A.shape
    rows = []
    for t in range(T):
        for i in range(M):
            for j in range(M):
                rows.append(candidates([float(x) for x in A[t, i, :]], [float(x) for x in B[t, :, j]],
                                       float(C[t, i, j])))
    names = list(rows[0])
    table = np.array([[r[n] for r in rows] for n in names])
    return A, B, C, names, table


def _probe(form, A, B, C):
    """one instruction per tile; form 1 packs four blocks into a tile"""
    from bayespy_amd.device import get_runtime, ptr
    rt = get_runtime()
    torch = rt.torch
    dev = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64).ravel().copy()).to(rt.device)
           for x in (A, B, C)]
    out = rt.zeros(C.size)
    out.fill_(float('nan'))
    ntiles = C.size // (256 if form == 0 else 64)
    assert ntiles * (256 if form == 0 else 64) == C.size
    rt.sync_stream()
    rt.check(rt.lib.vmp_mfma_order_probe(rt.ctx, form, ntiles, ptr(dev[0]), ptr(dev[1]), ptr(dev[2]),
                                         ptr(out)))
    rt.sync_stream()
    return out.cpu().numpy().reshape(C.shape)


@pytest.mark.parametrize('form', [0, 1], ids=['16x16x4', '4x4x4_4b'])
def test_order_of_accumulation(form):
    A, B, C, names, table = _cpu(form)
    assert table.shape[1] >= 1024 and len(names) == 75
    # --- CPU: the candidates are pairwise distinct on these inputs ------------------------------
    bits = table.view(np.uint64)
    least = None
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            n = int(np.count_nonzero(bits[i] != bits[j]))
            assert n > 0, 'candidates %r and %r agree on every output' % (names[i], names[j])
            least = n if least is None else min(least, n)
    print('form %d: %d outputs, %d candidates, every pair differs on at least %d outputs'
          % (form, table.shape[1], len(names), least))
    tiny = np.finfo(np.float64).tiny
    assert np.count_nonzero((A != 0.0) & (np.abs(A) < tiny)) >= 32           # subnormal operands,
    assert np.count_nonzero((C != 0.0) & (np.abs(C) < tiny)) >= 100          # subnormal C
    want = table[names.index(EXPECT)]
    assert np.count_nonzero((want != 0.0) & (np.abs(want) < tiny)) >= 100    # and subnormal results
    zero_c = np.count_nonzero(C == 0.0)
    assert zero_c > 50 and not np.signbit(C[C == 0.0]).any()
    # --- GPU: the lane layout, with small integers (exact in any order) -------------------------
    rng = np.random.default_rng(5 + form)
    Ai = rng.integers(-9, 10, A.shape).astype(np.float64)
    Bi = rng.integers(-9, 10, B.shape).astype(np.float64)
    Ci = rng.integers(-99, 100, C.shape).astype(np.float64)
    assert np.array_equal(_probe(form, Ai, Bi, Ci), Ai @ Bi + Ci), 'operand / result layout'
    # --- GPU: the order -------------------------------------------------------------------------
    got = _probe(form, A, B, C).ravel().view(np.uint64)
    match = [n for n, row in zip(names, bits) if np.array_equal(row, got)]
    near = sorted(((int(np.count_nonzero(row != got)), n) for n, row in zip(names, bits)))[:3]
    print('form %d: matches %s; nearest (outputs that differ, candidate): %s' % (form, match, near))
    assert len(match) == 1, 'no single candidate matches all outputs: %s, nearest %s' % (match, near)
    assert match[0] == EXPECT
