"""
The discrete hidden-Markov-model block (plans/hmm_cat.py) with multinomial emissions: every time
step carries a vector of counts over M categories (word histograms of a text window, event-type
counts per interval, k-mer counts per genomic bin)

    Z = CategoricalMarkovChain(a0, A, states=T)             plates () or (B,)
    Y = Mixture(Z, Multinomial, n, P);  Y.observe(x)        plates (T,) or (B, T), x (..., M)

with ``n`` a constant number of trials -- a scalar, or an array that broadcasts to the plates of
``Y`` + (1,), beside the cluster axis --, ``P`` a strictly positive constant (K, M) or
``Dirichlet(const, plates=(K,))`` and ``a0`` / ``A`` as in plans/hmm_cat.py.  T >= 2, K <= 64,
M <= 1024, counts of at most 65534 (``vmp_hmm_mult_limits``).

``MultinomialHMMPlan`` is ``CategoricalHMMPlan`` -- the chain-side bookkeeping, the word-major
<log P> table (M, K), the count table S (M, K), the Dirichlet rows of ``P``, masks, labels and
``save`` / ``load`` are inherited -- with counts for words: ``x`` is kept as one uint16 per entry
(one ``vmp_mmm_pack`` call over the B T rows, which checks the row sums against ``n`` and adds the
multinomial coefficients), and the pass is ``vmp_hmm_mult_pass`` (csrc/vmp_hmm_mult.hip):
E = X <log P>^T and S = X^T Gamma over the whole (b, t) plate on the fp64 matrix cores, the chain
kernel of the wide-emission pass between them.  Nothing of size (B, T, K, M) exists.

    <log p(Y)> = sum S . <log P> + sum over the observed rows [lgamma(n + 1) - sum_m lgamma(x_m + 1)]

A masked step gets zeros and zero trials before the pack, so that anything (NaN, -1, 1e300) may
stand there; it adds nothing to S, to the coefficients or to any other sum.

Opt-in: ``VB(..., engine='fused+counts')``, which is ``engine='fused'`` with the forms of
``plans.OPT_IN_COUNT_EMISSIONS`` tried right after their block.  Every other engine value keeps its
answer and never keeps such a plan on reuse.
"""
import ctypes

import numpy as np

from .hmm_cat import CatHMMKernels, CategoricalHMMPlan, _match
from .mmm import _DTYPES, row_trials

from ... import _lib
from ...device import ptr
from ...nodes.multinomial import Multinomial

LABEL = 'fused hidden-Markov-model block (multinomial emissions)'
_LIMITS = []


def hmm_mult_limits():
    """(max K, max M, largest count) of the built pass: host-only ``vmp_hmm_mult_limits``."""
    if not _LIMITS:
        v = [ctypes.c_int32() for _ in range(3)]
        _lib.raise_for_status(_lib.load().vmp_hmm_mult_limits(*[ctypes.byref(a) for a in v]))
        _LIMITS.append(tuple(a.value for a in v))
    return _LIMITS[0]


def _trials_reason(Y):
    if row_trials(Y) is None:
        return ('the number of trials n has shape %s: the block needs a constant integer array '
                'that broadcasts to the plates of Y + (1,), the same for every state'
                % (np.shape(Y._proto.trials),))
    return None


class MultHMMKernels(CatHMMKernels):

    def plan(self, B, T, M, K):
        """(chains of a workgroup, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_hmm_mult_plan(B, T, M, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the %s supports T >= 2, K <= %d, M <= %d and counts of at '
                                      'most %d' % ((LABEL,) + hmm_mult_limits()))
        return c.value, w.value

    def pack(self, N, M, dtype, x, trials, xp, flags, lcoef, ws):
        self.rt.check(self.lib.vmp_mmm_pack(self.ctx, N, M, dtype, ptr(x), ptr(trials), ptr(xp),
                                            ptr(flags), ptr(lcoef), ptr(ws)))

    def pass_(self, B, T, M, K, xp, elogPt, elog_a0, elog_A, labels, mask, ws, z0sum, xisum, S,
              scal, gamma=None, z0=None, zz=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_hmm_mult_pass(
            self.ctx, B, T, M, K, p(xp), p(elogPt), p(elog_a0), p(elog_A), p(labels), p(mask),
            p(ws), p(z0sum), p(xisum), p(S), p(scal), p(gamma), p(z0), p(zz)))


class MultinomialHMMPlan(CategoricalHMMPlan):
    """``CategoricalHMMPlan`` with count vectors for words.  Opt-in:
    ``VB(..., engine='fused+counts')``, tried right after the discrete HMM block."""

    _KIND, _EMISSIONS = 'hmm_mult', 'multinomial'

    @staticmethod
    def describe():
        return ("Mixture(CategoricalMarkovChain(a0, A, states=T), Multinomial, n, P) with each of "
                "a0, A, P a Dirichlet(const) node or a strictly positive constant and n a constant "
                "number of trials (a scalar or one per step), plates (T,) or (B, T), observed with "
                "count vectors that add up to n, without a mask or with a boolean mask of exactly "
                "that shape, T >= 2, K <= %d, M <= %d, counts of at most %d" % hmm_mult_limits())

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, label=LABEL, limits=lambda: hmm_mult_limits()[:2],
                      family=Multinomial, extra=_trials_reason)

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = MultHMMKernels(self.rt)
        return self._kernels

    # -- set-up ------------------------------------------------------------------------------------
    def _upload_y(self):
        """``x`` as uint16 (B T, M), the mask and the sum of the multinomial coefficients: one
        ``vmp_mmm_pack`` over the rows, a masked row as zeros with zero trials.  Counts that are
        negative, no integers or do not add up to ``n`` are the reference's ValueError
        (multinomial.py), one above the cap NotImplementedError."""
        rt, torch = self.rt, self.rt.torch
        R, M = self.B * self.T, self.M
        x = self.Y._data
        if x is None:
            raise ValueError('Node %s has not been observed' % self.Y.name)
        trials = row_trials(self.Y)
        if trials is None:
            raise ValueError('the number of trials of %s does not broadcast to its rows'
                             % self.Y.name)
        self._upload_mask()
        if isinstance(x, torch.Tensor):
            t = x.to(rt.device)
        else:
            a = np.asarray(x)
            if a.dtype == bool:
                a = a.astype(np.uint8)
            if a.dtype.name not in _DTYPES:
                a = a.astype(np.float64)
            t = torch.from_numpy(np.array(np.broadcast_to(a, self.Y.plates + (M,)), order='C'))
            t = t.to(rt.device)
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        if str(t.dtype).replace('torch.', '') not in _DTYPES:
            t = t.to(torch.float64)
        t = t.expand(self.Y.plates + (M,)).reshape(R, M)
        nd = torch.from_numpy(trials.reshape(-1) if R else np.zeros(1, dtype=np.int64)).to(rt.device)
        if self.maskd is not None and R:    # what stands at a masked step is never used
            seen = self.maskd.reshape(R) != 0
            t = torch.where(seen[:, None], t, torch.zeros_like(t))
            nd = torch.where(seen, nd, torch.zeros_like(nd))
        t = t.contiguous()
        self.xp = torch.zeros(max(R * M, 4), dtype=torch.int16, device=rt.device)
        self.lcoef = rt.zeros(1)
        flags = torch.zeros(4, dtype=torch.int32, device=rt.device)
        self.kernels.pack(R, M, _DTYPES[str(t.dtype).replace('torch.', '')], t, nd, self.xp, flags,
                          self.lcoef, rt.empty(1024))
        f = flags.cpu().numpy()
        if f[0]:
            raise ValueError("Counts must be integers" if f[2] else "Counts must be non-negative")
        if f[1]:
            raise NotImplementedError('%s: an observed count exceeds %d; the generic engine takes '
                                      'such data' % (LABEL, hmm_mult_limits()[2]))
        if f[3]:
            raise ValueError("Counts must sum to the number of trials")
        self._y_stale = False

    def _launch_pass(self, gamma, z0, zz):
        table = self.used_Pt if self._with_emissions else None
        self.kernels.pass_(self.B, self.T, self.M, self.K, self.xp, table, self.used_a0,
                           self.used_A, self.labels, self.maskd, self.ws, self.z0sum, self.xisum,
                           self.S, self.scal, gamma, z0, zz)

    # -- operations ----------------------------------------------------------------------------------
    def _y_term(self, s):
        """<log p(Y)>: S . <log P> and the multinomial coefficients of the observed rows."""
        return float(s[4]) + float(self.lcoef.cpu().numpy()[0])

    def get_moments(self, node):
        if node is self.Y:
            self._materialize()
            n = self.B * self.T * self.M
            xp = self.xp.cpu().numpy()[:n].view(np.uint16)
            return [xp.reshape(self.Y.plates + (self.M,)).astype(np.float64)]
        return super().get_moments(node)
