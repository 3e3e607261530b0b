"""
Execution plan of the hidden-Markov-model block with categorical emissions (the discrete HMM of
doc/source/examples/hmm.rst, first half)

    Z = CategoricalMarkovChain(a0, A, states=T)            plates () or (B,)
    Y = Mixture(Z, Categorical, P);  Y.observe(y)          plates (T,) or (B, T), y in [0, M)

with ``P`` a strictly positive constant (K, M) or ``Dirichlet(const, plates=(K,))`` over M
categories, and ``a0`` / ``A`` each a ``Dirichlet`` node under the conditions of plans/hmm.py or a
strictly positive constant (K,) / (K, K) -- hmm.rst's first model has three constants, and
``VB(Y, Z)`` is then the whole model.  T >= 2, K <= 64, M <= 128 (``vmp_hmm_fused_cat_limits``).
Opt-in: ``VB(..., engine='fused')``; the default engine runs this model on the generic engine.

``CategoricalHMMPlan`` is ``HMMPlan`` with another emission side: the chain-side bookkeeping (labels,
the tables of ``a0`` and ``A`` and their Dirichlet calls, the version logic of the pass, the formula
of L_Z, the mask and its checks, ``get_mask``) is inherited.  Its own state in HBM: ``y`` as int32
(B, T); <log P> WORD-MAJOR (M, K), so that the K lanes of a chain read one contiguous row per step;
``alpha_P``, ``prior_P`` and the table the last ``Z`` update used in the same layout for a Dirichlet
``P``; the count table
S (M, K) = sum over the observed (b, t) of gamma_{b,t,k} [y_{b,t} = m].

    update(Z)   one ``vmp_hmm_fused_pass_categorical``
    update(P)   ``vmp_lda_dirichlet`` on K rows of M columns with row stride 1 and column stride K
    <log p(Y)>  = sum S . <log P>   (``vmp_lda_dot``, with the present table)

Masks are those of plans/hmm.py, word for word: a masked step sends a zero message but stays a step
of the chain, contributes nothing to S, sum gamma . e or <log p(Y)>, and its word is never used --
any integer, -1 included, may stand there.  Every observed word is checked to be an integer in
[0, M) before it is uploaded (host arrays on the host, device tensors with one min / max over the
observed positions); the kernel treats a word outside the range as a masked step, so that a bad
word can never become an address, but the check here is what reports it.
"""
import ctypes

import numpy as np

from ._dirichlet import DirichletKernels, prior_table
from .hmm import HMMPlan, _takes_mask, _mask_shape

from ... import _lib
from ...device import ptr
from ...nodes.node import Constant
from ...nodes.dirichlet import Dirichlet
from ...nodes.categorical import Categorical
from ...nodes.categorical_markov_chain import (CategoricalMarkovChain,
                                               CategoricalMarkovChainToCategorical)
from ...nodes.mixture import Mixture

_LIMITS = []


def hmm_cat_limits():
    """(max K, max M) of the built pass: host-only ``vmp_hmm_fused_cat_limits``."""
    if not _LIMITS:
        k, m = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_hmm_fused_cat_limits(ctypes.byref(k),
                                                                   ctypes.byref(m)))
        _LIMITS.append((k.value, m.value))
    return _LIMITS[0]


class CatHMMKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def plan(self, B, T, M, K):
        """(chains of a workgroup, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_hmm_fused_cat_plan(B, T, M, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused hidden-Markov-model block with categorical '
                                      'emissions supports T >= 2, K <= %d and M <= %d'
                                  % hmm_cat_limits())
        return c.value, w.value

    def pass_(self, B, T, M, K, y, elogPt, elog_a0, elog_A, labels, mask, ws, z0sum, xisum, S, scal,
              gamma=None, z0=None, zz=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_hmm_fused_pass_categorical(
            self.ctx, B, T, M, K, p(y), p(elogPt), p(elog_a0), p(elog_A), p(labels), p(mask),
            p(ws), p(z0sum), p(xisum), p(S), p(scal), p(gamma), p(z0), p(zz)))


def _positive_constant(node, shape):
    return isinstance(node, Constant) and node.value.shape == shape and bool(np.all(node.value > 0))


def _match(nodes, why):
    for Y in nodes:
        if not isinstance(Y, Mixture) or not isinstance(Y.parents[0],
                                                        CategoricalMarkovChainToCategorical):
            continue
        if Y.node_class is not Categorical:
            continue            # another emission family: plans/hmm.py gives its reason

        def no(msg, Y=Y):
            if why is not None:
                why.append('fused hidden-Markov-model block with categorical emissions, observed '
                           'node %s: %s' % (Y.name or '<unnamed>', msg))
        Zc = Y.parents[0]
        Z = Zc.parents[0]
        if type(Z) is not CategoricalMarkovChain or len(Y.parents) != 2:
            no('its parents are not (CategoricalMarkovChain, P)')
            continue
        a0, A = Z.parents
        P = Y.parents[1]
        K, T = Z.categories, Z.states
        M = Y.dims[0][0]
        bad = [(n, nm) for n, nm in ((a0, 'a0'), (A, 'A'), (P, 'P'))
               if type(n) is not Dirichlet and not isinstance(n, Constant)]
        if bad:
            no('%s is %s: the block takes a Dirichlet node or a constant'
               % (bad[0][1], type(bad[0][0]).__name__))
            continue
        learned = [n for n in (a0, A, P) if type(n) is Dirichlet]
        if not all(any(n is m for m in nodes) for n in [Y, Z] + learned):
            continue
        chain = [Y, Zc, Z] + learned
        if any(any(m != 1 for m in n.plates_multiplier) for n in chain):
            no('plates_multiplier (mini-batches) goes through the generic engine')
            continue
        if any(getattr(n, '_shard_axis', None) is not None for n in chain):
            no('a plate is sharded over ranks')
            continue
        if not _takes_mask(Y):
            no('it has a mask of shape %s: the block takes no mask or a mask of the full shape of '
               'the plates of Y, here %s ((T,) for one chain, (B, T) for a batch); a scalar mask '
               'or one that broadcasts over a plate goes through the generic engine'
               % (_mask_shape(Y._mask), tuple(Y.plates)))
            continue
        bad = [n for n in learned if not isinstance(n.parents[0], Constant)]
        if bad:
            no('the concentration of %s is a node (%s), not a constant'
               % (bad[0].name, type(bad[0].parents[0]).__name__))
            continue
        if isinstance(P, Constant):
            if P.value.shape != (K, M):
                no('P has shape %s, not (K, M) = %s' % (P.value.shape, (K, M)))
                continue
            if not np.all(P.value > 0):
                no('the constant P has an entry that is not positive: 0 log 0 would put NaN into '
                   'the lower bound')
                continue
        elif P.plates != (K,):
            no('P has plates %s, not (K,)' % (P.plates,))
            continue
        if isinstance(a0, Constant) and not _positive_constant(a0, (K,)):
            no('the constant a0 is not a strictly positive vector of shape (K,)')
            continue
        if isinstance(A, Constant) and not _positive_constant(A, (K, K)):
            no('the constant A is not a strictly positive matrix of shape (K, K): a time plate or '
               'chain plates on the transition probabilities go through the generic engine')
            continue
        if type(A) is Dirichlet and A.plates != (K,):
            no('A has plates %s, not (K,): a time plate or chain plates on the transition '
               'probabilities go through the generic engine' % (A.plates,))
            continue
        if type(a0) is Dirichlet and any(p != 1 for p in a0.plates):
            no('a0 has plates %s' % (a0.plates,))
            continue
        if T < 2:
            no('the chain has T = %d < 2 time instances' % T)
            continue
        if len(Z.plates) > 1 or Y.plates != Z.plates + (T,) or Y.cluster_plate != -1:
            no('it needs plates (T,) or (B, T), Y has plates %s and Z has plates %s'
               % (Y.plates, Z.plates))
            continue
        max_K, max_M = hmm_cat_limits()
        if K > max_K or M > max_M:
            no('M = %d, K = %d exceed the limits of the block (M <= %d, K <= %d)'
               % (M, K, max_M, max_K))
            continue
        kids = [(Z, [Zc]), (Zc, [Y]), (Y, [])] \
            + [(n, [Z]) for n in (a0, A) if type(n) is Dirichlet] \
            + [(n, [Y]) for n in (P,) if type(n) is Dirichlet]
        if any([c for c, _ in n.children] != want for n, want in kids):
            no('one of its roles has other children as well')
            continue
        if any(n.observed for n in learned):
            no('a0, A or P is observed')
            continue
        bad = [n for n in learned if n._init is not None]
        if bad:
            no('%s is initialised by %s' % (bad[0].name, bad[0]._init[0]))
            continue
        roles = dict(Y=Y, Z=Z, Zc=Zc)
        for key, n in (('A', A), ('a0', a0), ('P', P)):
            if type(n) is Dirichlet:
                roles[key] = n
        return roles
    return None


class CategoricalHMMPlan(HMMPlan):

    @staticmethod
    def describe():
        return ("Mixture(CategoricalMarkovChain(a0, A, states=T), Categorical, P) with each of a0, "
                "A, P a Dirichlet(const) node (plates (), (K,), (K,)) or a strictly positive "
                "constant, plates (T,) or (B, T), observed with integers in [0, M) without a mask "
                "or with a boolean mask of exactly that shape, T >= 2, M <= %d, K <= %d"
                % (hmm_cat_limits()[1], hmm_cat_limits()[0]))

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why)

    def __init__(self, roles, runtime=None, kernels=None):
        super().__init__(roles, runtime, kernels)
        self.M = self.Y.dims[0][0]
        self.P = self.Y.parents[1]
        self.learnedP = 'P' in roles

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = CatHMMKernels(self.rt)
        return self._kernels

    # -- set-up ------------------------------------------------------------------------------------
    def _upload_y(self):
        """``y`` as int32 (B, T) and the mask; every observed word is an integer in [0, M)."""
        rt, torch = self.rt, self.rt.torch
        y = self.Y._data
        if y is None:
            raise ValueError('Node %s has not been observed' % self.Y.name)
        self._upload_mask()
        if isinstance(y, torch.Tensor):
            t = y.to(rt.device).expand(self.Y.plates).reshape(self.B, self.T)
            if t.dtype.is_floating_point and bool(torch.any(t != torch.round(t))):
                raise ValueError("Values must be integers")
            t = t.to(torch.int64)
            seen = t if self.maskd is None else t[self.maskd != 0]
            if seen.numel() and (int(seen.min()) < 0 or int(seen.max()) >= self.M):
                raise ValueError("Invalid category index")
            if self.maskd is not None:          # what stands at a masked position is never used
                t = torch.where(self.maskd != 0, t, torch.full_like(t, -1))
            self.yd = t.to(torch.int32).contiguous()
        else:
            a = np.asarray(y)
            m = self._host_mask()
            m = np.ones(self.Y.plates, dtype=bool) if m is None else m
            a = np.broadcast_to(a, self.Y.plates)
            seen = a[m]
            if a.dtype.kind == 'f':
                if np.any(seen != np.round(seen)):
                    raise ValueError("Values must be integers")
            elif a.dtype.kind not in 'iub':
                raise ValueError("Values must be integers")
            if seen.size and (seen.min() < 0 or seen.max() >= self.M):
                raise ValueError("Invalid category index")
            a = np.where(m, a, -1).astype(np.int32)
            self.yd = torch.from_numpy(np.ascontiguousarray(a.reshape(self.B, self.T))).to(rt.device)
        self._y_stale = False

    def _materialize(self):
        if self._ready:
            if self._y_stale:
                self._upload_y()
                self._run_pass(refresh=False)
            return
        from . import _delta
        self._delta = _delta.delta_roles(self.roles)
        rt, k = self.rt, self.kernels
        torch = rt.torch
        B, T, M, K = self.B, self.T, self.M, self.K
        rt.sync_stream()
        self.chains_per_wg, wsd = k.plan(B, T, M, K)
        self._upload_y()
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(rt.device)  # noqa: E731
        self.ws = rt.empty(int(wsd))
        self.S = rt.zeros(M, K)
        self.bndP = rt.zeros(1)
        self._init_chain_state()
        if self.learnedP:
            # K Dirichlet rows of M columns in the word-major table: element (k, m) at k + m K
            self.prior_P = up(prior_table(self.P, (K, M)).T)
            self.alpha_P, self.elogPt = rt.empty(M, K), rt.empty(M, K)
            self.used_Pt = rt.empty(M, K)           # the table of the last Z update, as used_A
            k.dirichlet(K, M, 1, K, self.prior_P, None, self.alpha_P, self.elogPt, self.ws_small,
                        self.bndP)
        else:
            self.elogPt = self.used_Pt = up(np.log(np.asarray(self.P.value, dtype=np.float64)).T)
        self._with_emissions = False
        self._ready = True
        self._run_pass()

    def _refresh_tables(self):
        super()._refresh_tables()
        if self.learnedP:
            self.used_Pt.copy_(self.elogPt)

    def _launch_pass(self, gamma, z0, zz):
        table = self.used_Pt if self._with_emissions else None
        self.kernels.pass_(self.B, self.T, self.M, self.K, self.yd, table, self.used_a0,
                           self.used_A, self.labels, self.maskd, self.ws, self.z0sum, self.xisum,
                           self.S, self.scal, gamma, z0, zz)

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        if self.learnedP and node is self.P:
            from . import _delta
            self._materialize()
            _delta.updated(self._delta, self.roles, node)
            self.rt.sync_stream()
            self.kernels.dirichlet(self.K, self.M, 1, self.K, self.prior_P, self.S, self.alpha_P,
                                   self.elogPt, self.ws_small, self.bndP)
            self._version += 1
        else:
            super().update(node)

    def _lower_bound_terms(self):
        from . import _delta
        self._materialize()
        if self._L_version != self._version:
            self.rt.sync_stream()
            self.kernels.dot(self.M * self.K, self.S, self.elogPt, self.ws_small, self.scal[4:5])
            s, chain = self._chain_terms()
            t = dict(Y=float(s[4]), **chain)
            if self.learnedP:
                t['P'] = float(self.bndP.cpu().numpy()[0])
            t['total'] = sum(t.values())
            self._L = t
            self._L_version = self._version
        return _delta.bound_terms(self._L, self._delta)

    def get_moments(self, node):
        self._materialize()
        if self.learnedP and node is self.P:
            return [self.elogPt.cpu().numpy().T.copy()]
        if node is self.Y:
            y = self.yd.cpu().numpy().reshape(self.Y.plates)
            return [(y[..., None] == np.arange(self.M)).astype(np.float64)]
        return super().get_moments(node)

    # -- persistence -----------------------------------------------------------------------------------
    _KIND, _EMISSIONS = 'hmm_cat', 'categorical'
    _DIMS = '(B, T, M, K, learned P, constant a0, constant A)'

    def _dims(self):
        return (self.B, self.T, self.M, self.K, int(self.learnedP),
                int(isinstance(self.a0, Constant)), int(isinstance(self.A, Constant)))

    @property
    def _SAVED(self):
        return self._SAVED_BOTH + ('S', 'elogPt') + (('alpha_P', 'used_Pt', 'bndP') if self.learnedP else ())
