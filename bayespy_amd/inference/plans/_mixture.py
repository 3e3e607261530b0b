"""
What the plate-mixture blocks share (bmm.py, dgmm.py, dgmm_masked.py, cmm.py, pmm.py)

    W = Dirichlet(const);  Z = Categorical(W, plates=(N, 1))
    parameters with plates (D, K);  X = Mixture(Z, family, parameters...);  X.observe(x)

``PlateMixturePlan`` owns the bookkeeping of such a block: the roles, the lazy runtime and kernels,
the version-guarded cache of the bound terms, the labels of an initialised ``Z``, the Dirichlet
step of the mixing weights, the mask of the observed node and the masks of its parents, and the
checkpoint group.  ``match_plate_mixture`` holds the checks every matcher makes, in the order
they were always made; a ``MixtureSpec`` supplies the family's own checks and every text that
differs between the blocks.  A family's file keeps its limits, kernels class, allocations, priors,
tables, pass, updates, the launches behind the bound terms and the moments.  mmm.py (count vectors,
plates (N,) and (K,)) derives from ``PlateMixturePlan`` too, with a matcher of its own.
"""
from collections import namedtuple

import numpy as np

from . import _delta

from ...device import get_runtime, ptr
from ...nodes.node import Constant, DeviceMask
from ...nodes.dirichlet import Dirichlet
from ...nodes.categorical import Categorical
from ...nodes.mixture import Mixture


def _p(t):
    return ptr(t) if t is not None else None


def _mask_shape(mask):
    return tuple(mask.shape) if isinstance(mask, DeviceMask) else np.shape(mask)


def _takes_mask(X):
    """No mask, or one of the full shape of the plates of ``X``."""
    return X._mask is True or _mask_shape(X._mask) == tuple(X.plates)


def observed_tensor(rt, node, N, D, dtypes, widen_bool=True):
    """``node._data`` as a contiguous (N, D) device tensor of a dtype of the table ``dtypes``, and
    its code there.  ``widen_bool``: bool becomes uint8 first; any other dtype outside the table
    becomes float64."""
    torch = rt.torch
    x = node._data
    if x is None:
        raise ValueError('Node %s has not been observed' % node.name)
    if isinstance(x, torch.Tensor):
        t = x.to(rt.device)
        if widen_bool and t.dtype == torch.bool:
            t = t.to(torch.uint8)
        if str(t.dtype).replace('torch.', '') not in dtypes:
            t = t.to(torch.float64)
    else:
        a = np.asarray(x)
        if widen_bool and a.dtype == bool:
            a = a.astype(np.uint8)
        if a.dtype.name not in dtypes:
            a = a.astype(np.float64)
        t = torch.from_numpy(np.array(np.broadcast_to(a, (N, D)), order='C')).to(rt.device)
    if tuple(t.shape) != (N, D) or not t.is_contiguous():
        t = t.expand(N, D).contiguous()
    return t, dtypes[str(t.dtype).replace('torch.', '')]


# -- the matcher -----------------------------------------------------------------------------------
# ``label``: the block in its reasons.  ``takes(X)``: whether the block looks at the Mixture ``X``
# at all (another family's is passed over in silence).  ``observed`` / ``weights``: the names of
# those two roles; ``params``: (name, node type, allowed initialisations or None for any) of the
# roles with plates (D, K), in the order of the parents.  ``parents`` / ``constant`` /
# ``role_plates``: the reasons for other parents, a parameter that is a node ('%s' twice) and
# other plates of the roles (str.format with the plates of Z, the parameters and the weights).
# ``mask(X)``, ``plates(X, first parameter)`` and ``limits(roles)``: a reason or None; ``mask`` may
# return '' to pass the node over in silence.  ``first(X)``: a reason before the parents are
# looked at, or None; ``arity``: the reason for another number of parents where it is not that of
# ``parents``.
MixtureSpec = namedtuple('MixtureSpec', 'label takes observed weights params parents constant '
                                        'role_plates mask plates limits first arity',
                         defaults=(None, None))


def full_mask_reason(X):
    if not _takes_mask(X):
        return ('it has a mask of shape %s: the block takes no mask or a mask of the full shape of '
                'the plates of X, here %s; a scalar mask or one that broadcasts over a plate goes '
                'through the generic engine' % (_mask_shape(X._mask), tuple(X.plates)))


def cluster_plate_reason(X):
    if X.cluster_plate != -1:
        return ('cluster_plate is %d, the block needs the clusters on the last plate axis (-1)'
                % X.cluster_plate)


def plates_of_p_reason(X, P):
    if X.cluster_plate != -1 or len(X.plates) != 2 or len(P.plates) != 2:
        return ('it needs plates (N, D) with the clusters on the last plate axis of P, X has '
                'plates %s and P has plates %s' % (X.plates, P.plates))


def batch_multiplier(Z):
    """The factor on the row axis of ``Z`` (the mini-batch stands for that many times its rows)."""
    m = tuple(np.ravel(Z.plates_multiplier))
    return float(m[0]) if m else 1.0


def batch_reason(X, Z, globals_):
    """What is wrong with the plate multipliers of a block under mini-batches (a reason), or None:
    ``Z`` and ``X`` carry one and the same positive factor on the row axis and nothing else does."""
    if any(any(m != 1 for m in n.plates_multiplier) for n in globals_):
        return ('a global node (%s) carries a plates_multiplier; only the mini-batch plate of Z and '
                'the observed node may' % ', '.join(
                    n.name or '<unnamed>' for n in globals_
                    if any(m != 1 for m in n.plates_multiplier)))
    mz, mx = tuple(np.ravel(Z.plates_multiplier)), tuple(np.ravel(X.plates_multiplier))
    if any(m != 1 for m in mz[1:]) or any(m != 1 for m in mx[1:]):
        return ('a plates_multiplier on an axis other than the rows: %s on Z, %s on the observed '
                'node' % (mz, mx))
    if not mz or not mx or not (mz[0] > 0 and mx[0] > 0) or mz[0] != mx[0]:
        return ('the plates_multiplier of Z / the observed node is not one positive factor on the '
                'row axis: %s, %s' % (mz, mx))
    return None


def match_plate_mixture(nodes, why, spec, batches=False):
    """The roles of the first Mixture among ``nodes`` that the block of ``spec`` takes, or None;
    the reason of every one it looks at and declines goes to ``why`` (a list, or None).
    ``batches``: the form under stochastic VI (_mixture_svi.py), which differs in the check of the
    plate multipliers and in the label of its reasons."""
    label = spec.label + (' (stochastic VI)' if batches else '')
    for X in nodes:
        if not isinstance(X, Mixture) or not spec.takes(X):
            continue

        def no(msg, X=X):
            if why is not None:
                why.append('%s, observed node %s: %s' % (label, X.name or '<unnamed>', msg))
        msg = spec.first(X) if spec.first is not None else None
        if msg is not None:
            no(msg)
            continue
        if len(X.parents) != 1 + len(spec.params):
            no(spec.arity or spec.parents)
            continue
        Z, params = X.parents[0], tuple(X.parents[1:])
        if type(Z) is not Categorical or type(Z.parents[0]) is not Dirichlet \
                or any(type(n) is not t for n, (_, t, _) in zip(params, spec.params)):
            no(spec.parents)
            continue
        W = Z.parents[0]
        names = ('Z',) + tuple(nm for nm, _, _ in spec.params) + (spec.weights,)
        below = (Z,) + params + (W,)
        if not all(any(n is m for m in nodes) for n in (X,) + below):
            continue
        if batches:
            msg = batch_reason(X, Z, params + (W,))
            if msg is not None:
                no(msg)
                continue
        elif any(any(m != 1 for m in n.plates_multiplier) for n in (X,) + below):
            no('plates_multiplier (mini-batches) goes through the generic engine')
            continue
        if any(getattr(n, '_shard_axis', None) is not None for n in (X,) + below):
            no('a plate is sharded over ranks')
            continue
        msg = spec.mask(X)
        if msg is not None:
            if msg:
                no(msg)
            continue
        bad = [(n, p) for n in params + (W,) for p in n.parents if not isinstance(p, Constant)]
        if bad:
            no(spec.constant % (bad[0][0].name, type(bad[0][1]).__name__))
            continue
        msg = spec.plates(X, params[0])
        if msg is not None:
            no(msg)
            continue
        N, D = X.plates
        K = X.clusters
        if Z.plates != (N, 1) or any(n.plates != (D, K) for n in params) \
                or any(p != 1 for p in W.plates):
            no(spec.role_plates.format(*[n.plates for n in below]))
            continue
        roles = dict(zip((spec.observed,) + names, (X,) + below))
        msg = spec.limits(roles)
        if msg is not None:
            no(msg)
            continue
        kids = [(W, [Z]), (Z, [X]), (X, [])] + [(n, [X]) for n in params]
        if any([c for c, _ in n.children] != want for n, want in kids):
            no('one of its roles has other children as well')
            continue
        if any(n.observed for n in below):
            no('%s or %s is observed' % (', '.join(names[:-1]), names[-1]))
            continue
        allowed = (('value',),) + tuple(ok for _, _, ok in spec.params) + (('parameters',),)
        bad = [(nm, n._init[0]) for n, nm, ok in zip(below, names, allowed)
               if ok is not None and n._init is not None and n._init[0] not in ok]
        if bad:
            no('%s is initialised by %s' % bad[0])
            continue
        return roles
    return None


# -- the plan --------------------------------------------------------------------------------------
class PlateMixturePlan:
    """A subclass names ``KERNELS`` (its kernels class), ``LABEL`` and ``KIND`` (the block in its
    messages and in a checkpoint), ``OBSERVED`` and ``WEIGHTS`` (those two roles), ``TERMS`` (the
    roles in the order their bound terms are summed), ``_SAVED`` (the device arrays of a
    checkpoint) and supplies ``match``, ``_repacks``, ``_materialize``, ``_run_pass``, ``update``,
    ``_bound_terms`` and ``get_moments``."""

    KERNELS = None
    LABEL = KIND = None
    OBSERVED, WEIGHTS = 'X', 'R'
    TERMS = ()
    DIMS = ('N', 'D', 'K')      # of a checkpoint
    _SAVED = ()
    _FLAGS = ()                 # boolean attributes a checkpoint keeps after 'labels is given'

    def __init__(self, roles, runtime=None, kernels=None):
        self.roles = roles
        for key, nd in roles.items():
            setattr(self, key, nd)
        self._set_shape(roles)
        self.K = roles[self.OBSERVED].clusters
        self._rt, self._kernels = runtime, kernels
        self._ready = False
        self._stale = False         # new observations wait to be packed
        self.maskd = None           # (N, D) uint8 in HBM when the observed node has a mask
        self._version = 0
        self._L_version = -1
        self._L = None
        for nd in roles.values():
            nd._plan = self

    def _set_shape(self, roles):
        """The plate sizes of the block; mmm.py, whose rows are count vectors, has (N,) and M."""
        self.N, self.D = roles[self.OBSERVED].plates

    @property
    def rt(self):
        if self._rt is None:
            self._rt = get_runtime()
        return self._rt

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = self.KERNELS(self.rt)
        return self._kernels

    def nodes(self):
        return list(self.roles.values())

    def has_state(self):
        return bool(self._ready)

    def invalidate(self, node):
        if node is self.roles[self.OBSERVED] and node.observed and self._repacks(node):
            # new observations of the same shape: they are packed again, the posteriors stay
            self._stale = True
            self._version += 1
            return
        _delta.warn_state_discarded(self, node)
        self._ready = False
        self._version += 1
        if type(self).match(self.nodes()) is None:
            self._hand_over()

    def _hand_over(self):
        from .generic import GenericPlan
        GenericPlan(self.nodes())

    # -- set-up ------------------------------------------------------------------------------------
    def _up(self, a):
        torch = self.rt.torch
        return torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(self.rt.device)

    def _upload_mask(self):
        rt, torch = self.rt, self.rt.torch
        m = self.roles[self.OBSERVED]._mask
        if m is True:
            self.maskd = None
        elif isinstance(m, DeviceMask):
            self.maskd = m.tensor.to(rt.device).reshape(self.N, self.D).to(torch.uint8).contiguous()
        else:
            self.maskd = torch.from_numpy(np.ascontiguousarray(
                np.asarray(m, dtype=bool).reshape(self.N, self.D).astype(np.uint8))).to(rt.device)

    def _repack(self):
        """New observations of the same shape: the mask and the pack."""
        self._upload_mask()
        self._pack()

    def _adopt_form(self):
        """The form of the pass for the packed data, where a block has more than one."""

    def _set_form(self):
        """... and, when it changes, the tables of the last ``Z`` update formed again in it."""

    def _restate(self):
        """New observations: packed again, then the statistics of the present ``Z`` state on
        them."""
        self._repack()
        self._set_form()
        self._run_pass()

    def _labels_from_init(self):
        """``labels``: the fixed labels of an initialised ``Z`` (device, int32), or None: its
        moments under the prior (no observation term)."""
        self.labels = None
        init = self.Z._init
        if init is None:
            return
        N = self.N
        lab = np.asarray(init[1])
        if lab.dtype.kind == 'f':
            if np.any(lab != np.round(lab)):
                raise ValueError("Values must be integers")
        elif lab.dtype.kind not in 'iub':
            raise ValueError("Values must be integers")
        lab = np.array(np.broadcast_to(lab, self.Z.plates), dtype=np.int64).reshape(N)
        if lab.size and (lab.min() < 0 or lab.max() >= self.K):
            raise ValueError("Invalid category index")
        self.labels = self.rt.torch.from_numpy(lab.astype(np.int32)).to(self.rt.device)

    def _weights_init_counts(self, prior):
        """What given initial parameters of the mixing weights add to ``prior`` (device), or
        None."""
        W = self.roles[self.WEIGHTS]
        if W._init is None:
            return None
        a = np.asarray(W._init[1][0], dtype=np.float64)
        if np.any(a <= 0):
            raise ValueError("Natural parameters should be positive")
        return self._up(np.broadcast_to(a, W.plates + (self.K,)).reshape(self.K) - prior)

    def _weights_step(self, slot, counts):
        """The Dirichlet step of the mixing weights from ``counts`` (None: the prior); its bound
        term goes to ``scal[slot]``."""
        K = self.K
        self.kernels.dirichlet(1, K, K, 1, self.prior_r, counts, self.alpha_r, self.elog_r,
                               self.ws_small, self.scal[slot:slot + 1])

    # -- operations ----------------------------------------------------------------------------------
    def _host_scal(self):
        """``scal`` on the host and the entropy term of ``Z`` in it."""
        s = self.scal.cpu().numpy()
        return s, (0.0 if self.labels is not None else float(s[0] - s[1] - s[2]))

    def _lower_bound_terms(self):
        self._materialize()
        if self._L_version != self._version:
            self.rt.sync_stream()
            t = self._bound_terms()
            total = t[self.TERMS[0]]
            for key in self.TERMS[1:]:
                total = total + t[key]
            t['total'] = total
            self._L = t
            self._L_version = self._version
        return _delta.bound_terms(self._L, self._delta)

    def lower_bound_contribution(self, node):
        terms = self._lower_bound_terms()
        for key in self.TERMS:
            if node is self.roles[key]:
                return terms[key]
        return 0.0

    def responsibilities(self):
        """(N, K) responsibilities of ``Z`` as a device array: formed by the pass in its write mode
        from the tables of the last ``Z`` update; not kept."""
        self._materialize()
        rt = self.rt
        rt.sync_stream()
        r = rt.empty(self.N, self.K)
        if self.N:
            self._run_pass(r)
        return r

    def _host_mask(self):
        """The mask as a boolean host array of shape (N, D), or None without one."""
        m = self.roles[self.OBSERVED]._mask
        return None if m is True else np.asarray(m, dtype=bool).reshape(self.N, self.D)

    def get_mask(self, node):
        """The observed node: its mask; ``Z``: any entry of the row observed, (N, 1); a parameter
        with plates (D, K): any entry of the column observed, (D, 1); the mixing weights: any
        entry observed -- the masks the reference propagates from the observed node to its
        parents."""
        m = self._host_mask()
        if m is None:
            return np.array(True)
        if node is self.roles[self.OBSERVED]:
            return m.copy()
        if node is self.Z:
            return m.any(axis=1)[:, None]
        if any(node is n for key, n in self.roles.items()
               if key not in (self.OBSERVED, 'Z', self.WEIGHTS)):
            return m.any(axis=0)[:, None]
        return np.array(bool(m.any()))

    # -- persistence -----------------------------------------------------------------------------------
    def _saved(self):
        return self._SAVED

    def _dims(self):
        return tuple(getattr(self, d) for d in self.DIMS)

    def save_state(self, put, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        _delta.save(put, base, self._delta)
        put(base + 'kind', np.array([ord(ch) for ch in self.KIND], dtype=np.uint8))
        put(base + 'dims', np.array(self._dims(), dtype=np.int64))
        put(base + 'flags', np.array([1 if self.labels is not None else 0]
                                     + [1 if getattr(self, f) else 0 for f in self._FLAGS],
                                     dtype=np.int64))
        if self.labels is not None:
            put(base + 'labels', self.labels.cpu().numpy())
        if self.maskd is not None:
            put(base + 'mask', self.maskd.cpu().numpy())
        for name in self._saved():
            put(base + name, getattr(self, name).cpu().numpy())

    def load_state(self, reader, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        if not reader.has(base + 'kind') or bytes(np.asarray(reader.get(base + 'kind'),
                                                             dtype=np.uint8)) != self.KIND.encode():
            raise Exception("File does not contain the state of the %s" % self.LABEL)
        dims = tuple(int(v) for v in reader.get(base + 'dims'))
        if dims != self._dims():
            raise ValueError('checkpoint is for (%s) = %s, the model has %s'
                             % (', '.join(self.DIMS), dims, self._dims()))
        saved = np.asarray(reader.get(base + 'mask'), dtype=np.uint8).reshape(-1) \
            if reader.has(base + 'mask') else None
        mine = None if self.maskd is None else self.maskd.cpu().numpy().reshape(-1)
        if (saved is None) != (mine is None) or (saved is not None
                                                 and not np.array_equal(saved != 0, mine != 0)):
            X = self.OBSERVED
            said = tuple('no mask on %s' % X if m is None else
                         'a mask on %s with %d of %d entries observed'
                         % (X, int(np.count_nonzero(m)), m.size) for m in (saved, mine))
            raise ValueError('checkpoint was saved with %s, the model has %s: observe %s with the '
                             'mask of the checkpoint before loading it' % (said + (X,)))
        torch = self.rt.torch
        self._delta = _delta.load(reader, base)
        flags = np.asarray(reader.get(base + 'flags')).ravel()
        if int(flags[0]):
            self.labels = torch.from_numpy(
                np.array(reader.get(base + 'labels'), dtype=np.int32)).to(self.rt.device)
        else:
            self.labels = None
        for i, f in enumerate(self._FLAGS, 1):
            setattr(self, f, bool(int(flags[i])))
        for name in self._saved():
            getattr(self, name).copy_(torch.from_numpy(
                np.array(reader.get(base + name), dtype=np.float64)).reshape(
                    getattr(self, name).shape).to(self.rt.device))
        self._version += 1
