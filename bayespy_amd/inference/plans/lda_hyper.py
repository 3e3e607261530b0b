"""
The latent-Dirichlet-allocation block (plans/lda.py, plans/lda_wide.py) with learnt concentrations

    a = DirichletConcentration(K);  p_topic = Dirichlet(a, plates=(D,))
    b = DirichletConcentration(V);  p_word  = Dirichlet(b, plates=(K,))

Either Dirichlet, or both, may have a ``Concentration`` parent (nodes/ml.py) in place of a constant.
``HyperLDAPlan`` and ``WideHyperLDAPlan`` are the two forms of the block with three additions, all
of them the size of a table or smaller:

* ``vmp_lda_concentration_stats`` (csrc/vmp_lda_hyper.hip): one pass over the parameters and <log>
  moments of a Dirichlet leaves S = sum_rows <log p> -- the children's message m0 to the
  concentration, m1 is the number of rows -- and qterm, the part of the Dirichlet's bound term that
  does not depend on the prior.  It runs at most once per state of a table (a version stamp).
* ``update(concentration)``: that pass, ``vmp_ml_concentration`` on one row of ``cols`` elements
  (the fixed point of the generic engine) and ``vmp_lda_prior_fill``, which writes
  the new vector into every row of the block's prior table.  The Dirichlet kernels keep reading a
  full prior table and are untouched.
* the bound: the term of a Dirichlet is rows z(a) + sum_c (a_c - 1) S_c - qterm with z(a) =
  lgamma(sum a) - sum lgamma(a) from ``vmp_ml_concentration``, right after a Dirichlet update and
  after a concentration update alike; the term of a concentration is <a> . reg0 + z reg1.

Opt-in: ``VB(..., engine='fused+hyper')`` is ``engine='fused'`` plus ``HyperLDAPlan``;
``engine='fused+topics+hyper'`` is ``engine='fused+topics'`` plus both forms (plans.OPT_IN_HYPER).
Every other engine value keeps its answer for such a model.  A model with two constant
concentrations is declined ("use the LDA block"), so these forms never take a model from the
existing ones.

Scope: full sweeps.  Declined with a reason: a plated concentration, a concentration with other
children or an initial value, ``plates_multiplier`` (stochastic VI with learnt concentrations),
masks, sharded plates and everything the block itself declines.
"""
import ctypes
import math

import numpy as np

from . import _delta
from .lda import LDAKernels, LDAPlan, _match, _narrow_topics
from .lda_wide import WideLDAKernels, WideLDAPlan, _wide_topics

from ... import _lib
from ...device import ptr
from ...nodes.node import Constant
from ...nodes.ml import Concentration

LABEL = 'fused LDA block (concentrations)'
MAX_ITER = 200000       # the cap of the generic engine (families/ml.py ConcentrationFamily)

_ERR_INF = ("Cannot estimate DirichletConcentration because of infs. This means that there are "
            "numerically zero probabilities in the child Dirichlet node.")


class _HyperKernels:
    """Mixin of a kernels class that has ``rt``, ``lib`` and ``ctx``."""

    def stats_ws(self, rows, cols, rs, cs):
        """Doubles of the workspace of ``stats`` for this table."""
        w = ctypes.c_int64()
        rc = self.lib.vmp_lda_concentration_stats_workspace(rows, cols, rs, cs, ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'vmp_lda_concentration_stats_workspace')
        return w.value

    def stats(self, rows, cols, rs, cs, alpha, elog, ws, S, qterm):
        self.rt.check(self.lib.vmp_lda_concentration_stats(
            self.ctx, rows, cols, rs, cs, ptr(alpha), ptr(elog), ptr(ws), ptr(S), ptr(qterm)))

    def prior_fill(self, rows, cols, rs, cs, a, prior):
        self.rt.check(self.lib.vmp_lda_prior_fill(self.ctx, rows, cols, rs, cs, ptr(a),
                                                  ptr(prior)))

    def ml_concentration(self, K, m0, m1, r0, r1, max_iter, alpha, work, z, status):
        """One row of ``K`` elements through ``vmp_ml_concentration``."""
        self.rt.check(self.lib.vmp_ml_concentration(
            self.ctx, 1, K, ptr(m0), ptr(m1), ptr(r0), ptr(r1), int(max_iter), ptr(alpha),
            ptr(work), ptr(z), ctypes.c_void_p(status.data_ptr())))


class HyperLDAKernels(_HyperKernels, LDAKernels):
    pass


class WideHyperLDAKernels(_HyperKernels, WideLDAKernels):
    pass


def _no_batches(words, topics, p_word, p_topic):
    if any(any(m != 1 for m in n.plates_multiplier) for n in (words, topics, p_word, p_topic)):
        return ('plates_multiplier (mini-batches): stochastic VI with learnt concentrations is not '
                'built; it goes through the generic engine')
    return None


def _learnt_parents(p_topic, p_word, nodes):
    """(reason or None, further roles): each Dirichlet has a constant or an unplated, unobserved
    ``Concentration`` that has no other child; at least one has the node.  (A Dirichlet takes its
    dimension from such a parent and accepts no other kind of node, nodes/dirichlet.py.)"""
    extra = {}
    for key, d in (('conc_topic', p_topic), ('conc_word', p_word)):
        c = d.parents[0]
        if isinstance(c, Constant):
            continue
        if tuple(c.plates) != ():
            return ('the Concentration of %s has plates %s (one vector for all rows is what the '
                    'block learns)' % (d.name, tuple(c.plates))), None
        if any(k is not d for k, _ in c.children):
            return 'the Concentration of %s has other children as well' % d.name, None
        if c.observed:
            return 'the Concentration of %s is observed' % d.name, None
        if c._init is not None:
            return 'the Concentration of %s is initialised by %s' % (d.name, c._init[0]), None
        if not any(c is m for m in nodes):
            return 'the Concentration of %s is not among the nodes' % d.name, None
        if getattr(c, '_shard_axis', None) is not None:
            return 'a plate is sharded over ranks', None
        extra[key] = c
    if not extra:
        return 'both concentrations are constants: use the LDA block', None
    return None, extra


# role of a concentration -> (role of its Dirichlet, slot of that Dirichlet's bound in ``scal``)
_CHILD = {'conc_topic': ('p_topic', 3), 'conc_word': ('p_word', 4)}


class _HyperMixin:
    """What ``HyperLDAPlan`` and ``WideHyperLDAPlan`` add to their block."""

    def gradient_step(self, nodes, scale=1.0):
        raise NotImplementedError(
            '%s: gradient steps (stochastic VI) with learnt concentrations are not built; use '
            'VB(..., engine="generic")' % LABEL)

    # -- set-up ------------------------------------------------------------------------------------
    def _conc_key(self, node):
        for key in _CHILD:
            if self.roles.get(key) is node:
                return key
        return None

    def _prior_table(self, node, shape):
        """A learnt concentration starts at ones (dirichlet.py:257): the prior the Dirichlets are
        initialised and drawn from at set-up."""
        if isinstance(node.parents[0], Concentration):
            return np.ones(shape)
        return super()._prior_table(node, shape)

    def _table(self, key):
        """(rows, cols, row stride, column stride, alpha, elog, prior) of a concentration's child."""
        D, V, K = self.D, self.V, self.K
        if key == 'conc_topic':
            return D, K, K, 1, self.alpha_theta, self.elog_theta, self.prior_theta
        return K, V, 1, K, self.alpha_beta_t, self.elog_beta_t, self.prior_beta_t

    def _materialize(self, recount=True):
        fresh = not self._ready
        super()._materialize(recount)
        if not fresh:
            return
        rt, k = self.rt, self.kernels
        torch = rt.torch
        self.hyper = {}
        for key in _CHILD:
            if key not in self.roles:
                continue
            rows, cols, rs, cs = self._table(key)[:4]
            h = dict(a=rt.empty(cols), work=rt.empty(cols), z=rt.empty(1), S=rt.empty(cols),
                     qterm=rt.empty(1), ws=rt.empty(max(k.stats_ws(rows, cols, rs, cs), 1)),
                     m1=rt.empty(1), r0=rt.empty(cols), r1=rt.empty(1),
                     status=torch.zeros(3, dtype=torch.int32, device=rt.device),
                     table_version=0, stats_version=-1)
            h['a'].fill_(1.0)
            h['z'].fill_(math.lgamma(cols))          # lgamma(sum of ones) - sum lgamma(1)
            h['m1'].fill_(float(rows))
            self.hyper[key] = h
        self.hscal = rt.zeros(2)                     # bound terms of conc_topic, conc_word
        self._reg_stale = True

    def _regularization(self):
        """The regularization of every concentration on the device (uploaded when it changed)."""
        if not self._reg_stale:
            return
        torch = self.rt.torch
        for key, h in self.hyper.items():
            reg = self.roles[key].regularization
            cols = h['a'].numel()
            r0 = np.ascontiguousarray(np.broadcast_to(np.asarray(reg[0], dtype=np.float64), (cols,)))
            h['r0'].copy_(torch.from_numpy(r0.copy()).to(self.rt.device))
            h['r1'].fill_(float(np.asarray(reg[1], dtype=np.float64)))
        self._reg_stale = False

    def invalidate(self, node, keep_state=False):
        if keep_state and self._conc_key(node) is not None:
            # the regularization setter: the estimate and every table stay, the concentration's
            # next update and bound term read the new values
            self._reg_stale = True
            self._version += 1
            return
        super().invalidate(node)

    # -- operations ----------------------------------------------------------------------------------
    def _stats(self, key):
        """S and qterm of the present tables of a concentration's child: one pass per state."""
        h = self.hyper[key]
        if h['stats_version'] == h['table_version']:
            return
        rows, cols, rs, cs, alpha, elog, _ = self._table(key)
        self.kernels.stats(rows, cols, rs, cs, alpha, elog, h['ws'], h['S'], h['qterm'])
        h['stats_version'] = h['table_version']

    def _update_dirichlet(self, node):
        super()._update_dirichlet(node)
        for key, (child, _) in _CHILD.items():
            if key in self.hyper and node is self.roles[child]:
                self.hyper[key]['table_version'] += 1

    def update(self, node):
        key = self._conc_key(node)
        if key is None:
            return super().update(node)
        self._materialize()
        rt, k = self.rt, self.kernels
        h = self.hyper[key]
        rows, cols, rs, cs, _, _, prior = self._table(key)
        with rt.operation():
            self._regularization()
            self._stats(key)
            k.ml_concentration(cols, h['S'], h['m1'], h['r0'], h['r1'], MAX_ITER, h['a'], h['work'],
                               h['z'], h['status'])
            k.prior_fill(rows, cols, rs, cs, h['a'], prior)
            rt.defer_check(h['status'][0:1], ValueError, _ERR_INF)
            rt.defer_check(h['status'][1:2], RuntimeError,
                           'The fixed point of %s did not converge in %d iterations'
                           % (node.name, MAX_ITER))
        self._version += 1

    def _lower_bound_terms(self):
        self._materialize()
        if self._L_version != self._version:
            self.rt.sync_stream()
            self._regularization()
            for i, key in enumerate(_CHILD):
                if key not in self.hyper:
                    continue
                h = self.hyper[key]
                self._stats(key)
                slot = _CHILD[key][1]
                # the Dirichlet's term under the prior as it is now, beside the other scalars
                self.scal[slot:slot + 1] = (h['m1'] * h['z'] + ((h['a'] - 1.0) * h['S']).sum()
                                            - h['qterm'])
                self.hscal[i:i + 1] = (h['a'] * h['r0']).sum() + h['z'] * h['r1']
            super()._lower_bound_terms()
            hs = self.hscal.cpu().numpy()
            for i, key in enumerate(_CHILD):
                if key in self.hyper:
                    self._L[key] = float(hs[i])
                    self._L['total'] += float(hs[i])
        return _delta.bound_terms(self._L, self._delta)

    def lower_bound_contribution(self, node):
        key = self._conc_key(node)
        if key is not None:
            return self._lower_bound_terms()[key]
        return super().lower_bound_contribution(node)

    def get_moments(self, node):
        key = self._conc_key(node)
        if key is None:
            return super().get_moments(node)
        self._materialize()
        h = self.hyper[key]
        return [h['a'].cpu().numpy().copy(), h['z'].cpu().numpy().reshape(()).copy()]

    def get_parameters(self, node):
        if self._conc_key(node) is not None:
            raise NotImplementedError('natural parameters of %s: a maximum-likelihood node has no '
                                      'distribution (the reference does not define it either)'
                                      % type(node).__name__)
        self._materialize()
        if node is self.p_topic:
            return [self.alpha_theta.cpu().numpy().copy()]
        if node is self.p_word:
            return [self.alpha_beta_t.cpu().numpy().T.copy()]
        raise NotImplementedError('%s: get_parameters of %s; use VB(..., engine="generic")'
                                  % (LABEL, node.name))

    # -- persistence -----------------------------------------------------------------------------------
    def save_state(self, put, nodes, index):
        super().save_state(put, nodes, index)
        base = 'plans/%d/' % index
        for key, h in self.hyper.items():
            put(base + key + '_a', h['a'].cpu().numpy())
            put(base + key + '_z', h['z'].cpu().numpy())

    def load_state(self, reader, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        # a file of this form must learn the very concentrations this model learns: told apart
        # before any state is touched (a file of another form is refused by the block's own check)
        if reader.has(base + 'kind') and bytes(np.asarray(
                reader.get(base + 'kind'), dtype=np.uint8)).decode() == self._KIND:
            held = sorted(k for k in _CHILD if reader.has(base + k + '_a'))
            if held != sorted(self.hyper):
                raise Exception('File holds the learnt concentrations of %s, this model learns %s'
                                % (', '.join(_CHILD[k][0] for k in held),
                                   ', '.join(_CHILD[k][0] for k in sorted(self.hyper))))
        super().load_state(reader, nodes, index)
        torch = self.rt.torch
        self.rt.sync_stream()
        for key, h in self.hyper.items():
            for nm in ('a', 'z'):
                h[nm].copy_(torch.from_numpy(np.array(reader.get(base + key + '_' + nm),
                                                      dtype=np.float64)).to(self.rt.device))
            rows, cols, rs, cs, _, _, prior = self._table(key)
            self.kernels.prior_fill(rows, cols, rs, cs, h['a'], prior)
            h['table_version'] += 1
        self._version += 1


class HyperLDAPlan(_HyperMixin, LDAPlan):
    """``LDAPlan`` with a ``Concentration`` parent on p_topic, p_word or both.  Opt-in:
    ``VB(..., engine='fused+hyper')``, tried right after the LDA block."""

    _KIND = 'lda_hyper'

    @staticmethod
    def describe():
        return LDAPlan.describe() + '; either const may be a DirichletConcentration node'

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, _no_batches, label=LABEL, topics_rule=_narrow_topics,
                      parent_rule=_learnt_parents)

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = HyperLDAKernels(self.rt)
        return self._kernels


class WideHyperLDAPlan(_HyperMixin, WideLDAPlan):
    """``WideLDAPlan`` with a ``Concentration`` parent on p_topic, p_word or both.  Opt-in:
    ``VB(..., engine='fused+topics+hyper')``, tried right after the wide-topic form."""

    _KIND = 'lda_wide_hyper'

    @staticmethod
    def describe():
        return WideLDAPlan.describe() + '; either const may be a DirichletConcentration node'

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why, _no_batches, label=LABEL, topics_rule=_wide_topics,
                      parent_rule=_learnt_parents)

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = WideHyperLDAKernels(self.rt)
        return self._kernels
