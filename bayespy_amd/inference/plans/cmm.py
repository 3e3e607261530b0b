"""
Execution plan of the categorical-mixture block (the latent class model)

    R = Dirichlet(const);  Z = Categorical(R, plates=(N, 1))
    P = Dirichlet(const, plates=(D, K));  X = Mixture(Z, Categorical, P);  X.observe(x)

with constant concentrations, x (N, D) integers in [0, M), K <= 64, 2 <= M <= 32 and a count table
of roundup(D, 64 / KP) M KP doubles (KP = 16, 32 or 64 lanes for the K clusters) within the LDS cap
of ``vmp_cmm_limits``; ``X`` fully observed or observed with a mask of the full shape (N, D).
Opt-in: ``VB(..., engine='fused')``; the default engine runs this model on the generic engine as
before.  The plan owns, in HBM: ``x`` as one byte per entry (255 = hidden), the Dirichlet
parameters and <log P> CATEGORY-MAJOR as (M, D K) tables -- a (d, k) row of ``P`` has row stride 1
and column stride D K, ``vmp_lda_dirichlet`` updates all D K rows in one launch and the K values
a lookup needs are contiguous --, those of ``R`` (K), the tables L = <log P> and c = <log pi> less
its maximum that the last ``Z`` update used, and the statistics
S[m, d, k] = sum_n r_nk [x_nd = m], N_k = sum_n r_nk.  Nothing of size (N, K), (N, D, K) or
(N, D, M) exists: the responsibilities of ``Z`` are formed inside ``vmp_cmm_pass`` and only on
request written out (``Z.get_moments()``).

All plate terms of the lower bound follow from the statistics, sum_n lse_n and the tables:
    <log p(X)>           = sum S . <log P>            (the present table)
    <log p(Z)> + entropy = sum_k N_k <log pi_k> + sum_n lse_n - N_k . c_used - S . L_used
``L`` and ``c`` are written by a ``Z`` update only, so ``Z.get_moments()`` after a later ``P``
update is still that update's posterior.

Masks: ``X.observe(x, mask=m)`` with ``m`` a boolean host array or a ``DeviceMask`` of shape
exactly (N, D).  A hidden position becomes the reserved byte when ``x`` is packed and is never
interpreted: NaN, -1 or 1e300 may stand there.  The pass is the same kernel with or without a mask
(a mask of ones gives the bits of the unmasked run) and the Dirichlet counts need no separate
M_dk: S already counts the observed entries only.  A row with nothing observed has ``Z.mask``
False: its moment is softmax(<log pi>) of the tables the last update used and it enters neither
N_k nor the bound term of ``Z``.  A column with nothing observed leaves its rows of ``P`` at the
prior, with a bound term of exactly zero.  A scalar mask or one that broadcasts over a plate is
declined (generic engine).

Checkpoints: the block writes its own ``plans/<i>/`` group (kind 'cmm'); a checkpoint whose mask
differs is refused.
"""
import ctypes

import numpy as np

from . import _delta
from ._dirichlet import DirichletKernels, prior_table
from .bmm import _mask_shape, _takes_mask

from ... import _lib
from ...device import get_runtime, ptr
from ...nodes.node import Constant, DeviceMask
from ...nodes.dirichlet import Dirichlet
from ...nodes.categorical import Categorical
from ...nodes.categorical_markov_chain import CategoricalMarkovChainToCategorical
from ...nodes.multinomial import Multinomial
from ...nodes.mixture import Mixture

_DTYPES = {'float64': 0, 'int64': 1, 'uint8': 2, 'int32': 3}
_LIMITS = []


def cmm_limits():
    """(max K, min M, max M, max cells of the LDS count table) of the built pass: host-only
    ``vmp_cmm_limits``."""
    if not _LIMITS:
        v = [ctypes.c_int32() for _ in range(4)]
        _lib.raise_for_status(_lib.load().vmp_cmm_limits(*[ctypes.byref(a) for a in v]))
        _LIMITS.append(tuple(a.value for a in v))
    return _LIMITS[0]


def cmm_supported(N, D, K, M):
    """Whether the built pass takes the shape: host-only ``vmp_cmm_plan``."""
    c, w = ctypes.c_int64(), ctypes.c_int64()
    return _lib.load().vmp_cmm_plan(N, D, K, M, ctypes.byref(c), ctypes.byref(w)) == _lib.VMP_OK


def _limits_text():
    return ('K <= %d, %d <= M <= %d and a count table of roundup(D, 64 / KP) M KP <= %d doubles '
            'in LDS (KP = 16, 32 or 64 lanes for the K clusters)' % cmm_limits())


class CMMKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def plan(self, N, D, K, M):
        """(rows of a chunk, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_cmm_plan(N, D, K, M, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused categorical-mixture block supports '
                                  + _limits_text())
        return c.value, w.value

    def pack(self, N, D, M, dtype, x, mask, xb, flag):
        self.rt.check(self.lib.vmp_cmm_pack(self.ctx, N, D, M, dtype, ptr(x),
                                            ptr(mask) if mask is not None else None, ptr(xb),
                                            ptr(flag)))

    def tables(self, D, K, M, elog_p, elog_pi, L, c):
        self.rt.check(self.lib.vmp_cmm_tables(self.ctx, D, K, M,
                                              ptr(elog_p) if elog_p is not None else None,
                                              ptr(elog_pi), ptr(L), ptr(c)))

    def pass_(self, N, D, K, M, xb, labels, L, c, ws, S, Nk, scal, r_out=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_cmm_pass(self.ctx, N, D, K, M, p(xb), p(labels), p(L), p(c),
                                            p(ws), p(S), p(Nk), p(scal), p(r_out)))


def _match(nodes, why):
    for X in nodes:
        if not isinstance(X, Mixture) or not (isinstance(X.node_class, type)
                                              and issubclass(X.node_class,
                                                             (Categorical, Multinomial))):
            continue
        if isinstance(X.parents[0], CategoricalMarkovChainToCategorical):
            continue            # a hidden Markov model: plans/hmm_cat.py gives its reasons

        def no(msg, X=X):
            if why is not None:
                why.append('fused categorical-mixture block, observed node %s: %s'
                           % (X.name or '<unnamed>', msg))
        if X.node_class is not Categorical:
            no('the mixed distribution is %s, not Categorical' % X.node_class.__name__)
            continue
        if len(X.parents) != 2:
            no('its parents are not (Categorical(Dirichlet), Dirichlet)')
            continue
        Z, P = X.parents[0], X.parents[1]
        if type(Z) is not Categorical or type(P) is not Dirichlet \
                or type(Z.parents[0]) is not Dirichlet:
            no('its parents are not (Categorical(Dirichlet), Dirichlet)')
            continue
        R = Z.parents[0]
        four = (X, Z, P, R)
        if not all(any(n is m for m in nodes) for n in four):
            continue
        if any(any(m != 1 for m in n.plates_multiplier) for n in four):
            no('plates_multiplier (mini-batches) goes through the generic engine')
            continue
        if any(getattr(n, '_shard_axis', None) is not None for n in four):
            no('a plate is sharded over ranks')
            continue
        if not _takes_mask(X):
            no('it has a mask of shape %s: the block takes no mask or a mask of the full shape of '
               'the plates of X, here %s; a scalar mask or one that broadcasts over a plate goes '
               'through the generic engine' % (_mask_shape(X._mask), tuple(X.plates)))
            continue
        bad = [n for n in (P, R) if not isinstance(n.parents[0], Constant)]
        if bad:
            no('the concentration of %s is a node (%s), not a constant'
               % (bad[0].name, type(bad[0].parents[0]).__name__))
            continue
        if X.cluster_plate != -1 or len(X.plates) != 2 or len(P.plates) != 2:
            no('it needs plates (N, D) with the clusters on the last plate axis of P, X has plates '
               '%s and P has plates %s' % (X.plates, P.plates))
            continue
        N, D = X.plates
        K = X.clusters
        M = P.dims[0][0]
        if Z.plates != (N, 1) or P.plates != (D, K) or any(p != 1 for p in R.plates):
            no('plates of Z / P / R are not (N, 1), (D, K), ()')
            continue
        if not cmm_supported(N, D, K, M):
            no('D = %d, K = %d, M = %d exceed the limits of the block (%s)'
               % (D, K, M, _limits_text()))
            continue
        kids = ((R, [Z]), (Z, [X]), (P, [X]), (X, []))
        if any([c for c, _ in n.children] != want for n, want in kids):
            no('one of its roles has other children as well')
            continue
        if Z.observed or P.observed or R.observed:
            no('Z, P or R is observed')
            continue
        if Z._init is not None and Z._init[0] != 'value':
            no('Z is initialised by %s' % Z._init[0])
            continue
        if R._init is not None and R._init[0] != 'parameters':
            no('R is initialised by %s' % R._init[0])
            continue
        return dict(X=X, Z=Z, P=P, R=R)
    return None


class CategoricalMixturePlan:

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates=(N, 1)), Categorical, "
                "Dirichlet(const, plates=(D, K))) over M categories, fully observed or observed "
                "with a mask of the full shape (N, D), %s; a scalar mask or one that broadcasts "
                "over a plate is declined" % _limits_text())

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why)

    def __init__(self, roles, runtime=None, kernels=None):
        self.roles = roles
        self.X, self.Z, self.P, self.R = roles['X'], roles['Z'], roles['P'], roles['R']
        self.N, self.D = self.X.plates
        self.K = self.X.clusters
        self.M = self.P.dims[0][0]
        self._rt, self._kernels = runtime, kernels
        self._ready = False
        self._x_stale = False
        self.maskd = None           # (N, D) uint8 in HBM when X has a mask
        self._version = 0
        self._L_version = -1
        self._L = None
        for nd in roles.values():
            nd._plan = self

    @property
    def rt(self):
        if self._rt is None:
            self._rt = get_runtime()
        return self._rt

    @property
    def kernels(self):
        if self._kernels is None:
            self._kernels = CMMKernels(self.rt)
        return self._kernels

    def nodes(self):
        return list(self.roles.values())

    def has_state(self):
        return bool(self._ready)

    def invalidate(self, node):
        if node is self.X and node.observed and _takes_mask(node):
            # new observations of the same shape, with any mask of the full shape or none: the
            # bytes are packed again, the posteriors stay
            self._x_stale = True
            self._version += 1
            return
        _delta.warn_state_discarded(self, node)
        self._ready = False
        self._version += 1
        if CategoricalMixturePlan.match(self.nodes()) is None:
            from .generic import GenericPlan
            GenericPlan(self.nodes())

    # -- set-up ------------------------------------------------------------------------------------
    def _upload_mask(self):
        rt, torch = self.rt, self.rt.torch
        m = self.X._mask
        if m is True:
            self.maskd = None
        elif isinstance(m, DeviceMask):
            self.maskd = m.tensor.to(rt.device).reshape(self.N, self.D).to(torch.uint8).contiguous()
        else:
            self.maskd = torch.from_numpy(np.ascontiguousarray(
                np.asarray(m, dtype=bool).reshape(self.N, self.D).astype(np.uint8))).to(rt.device)

    def _pack(self):
        """``X._data`` as bytes; an observed value that is no integer in [0, M) is the reference's
        ValueError (categorical.py)."""
        rt, torch = self.rt, self.rt.torch
        N, D = self.N, self.D
        x = self.X._data
        if x is None:
            raise ValueError('Node %s has not been observed' % self.X.name)
        if isinstance(x, torch.Tensor):
            t = x.to(rt.device)
            if t.dtype == torch.bool:
                t = t.to(torch.uint8)
            if str(t.dtype).replace('torch.', '') not in _DTYPES:
                t = t.to(torch.float64)
        else:
            a = np.asarray(x)
            if a.dtype == bool:
                a = a.astype(np.uint8)
            if a.dtype.name not in _DTYPES:
                a = a.astype(np.float64)
            t = torch.from_numpy(np.array(np.broadcast_to(a, (N, D)), order='C')).to(rt.device)
        if tuple(t.shape) != (N, D) or not t.is_contiguous():
            t = t.expand(N, D).contiguous()
        dtype = _DTYPES[str(t.dtype).replace('torch.', '')]
        self.xb = torch.zeros(max(N * D, 8), dtype=torch.uint8, device=rt.device)
        flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
        self.kernels.pack(N, D, self.M, dtype, t, self.maskd, self.xb, flag)
        if int(flag.cpu().numpy()[0]) != 0:
            raise ValueError("Invalid category index")
        self._x_stale = False

    def _materialize(self):
        if self._ready:
            if self._x_stale:
                self._upload_mask()
                self._pack()
                self._run_pass()
            return
        self._delta = _delta.delta_roles(self.roles)
        rt, k = self.rt, self.kernels
        torch = rt.torch
        N, D, K, M = self.N, self.D, self.K, self.M
        rt.sync_stream()
        self._upload_mask()
        self.chunk, wsd = k.plan(N, D, K, M)
        self._pack()
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(rt.device)  # noqa: E731
        pp = prior_table(self.P, (D, K, M))
        pr = prior_table(self.R, (K,))
        # D K Dirichlet rows of M columns in the category-major table: element (dk, m) at dk + m D K
        self.prior_p, self.prior_r = up(pp.reshape(D * K, M).T), up(pr)
        self.alpha_p, self.elog_p = rt.empty(M, D * K), rt.empty(M, D * K)
        self.alpha_r, self.elog_r = rt.empty(K), rt.empty(K)
        self.L, self.c = rt.zeros(M, D * K), rt.zeros(K)
        self.S, self.Nk = rt.zeros(M, D * K), rt.zeros(K)
        self.ws = rt.empty(int(wsd))
        self.ws_small = rt.empty(max(D * K, 1024))
        # [0] sum lse, [1] N_k . c used, [2] S . L used, [3] bound of P, [4] bound of R,
        # [5] S . <log P>, [6] N_k . <log pi>
        self.scal = rt.zeros(8)
        self._init_p(pp)
        self._init_r(pr)
        # Z: fixed labels, or its moments under the prior (no observation term)
        self.labels = None
        init = self.Z._init
        if init is not None:
            lab = np.asarray(init[1])
            if lab.dtype.kind == 'f':
                if np.any(lab != np.round(lab)):
                    raise ValueError("Values must be integers")
            elif lab.dtype.kind not in 'iub':
                raise ValueError("Values must be integers")
            lab = np.array(np.broadcast_to(lab, (N, 1)), dtype=np.int64).reshape(N)
            if lab.size and (lab.min() < 0 or lab.max() >= K):
                raise ValueError("Invalid category index")
            self.labels = torch.from_numpy(lab.astype(np.int32)).to(rt.device)
        self._tables(None)
        self._ready = True
        self._run_pass()

    def _init_r(self, prior):
        rt, k = self.rt, self.kernels
        init = self.R._init
        counts = None
        if init is not None:
            a = np.asarray(init[1][0], dtype=np.float64)
            if np.any(a <= 0):
                raise ValueError("Natural parameters should be positive")
            a = np.broadcast_to(a, (self.K,))
            counts = rt.torch.from_numpy(np.array(a - prior, order='C')).to(rt.device)
        k.dirichlet(1, self.K, self.K, 1, self.prior_r, counts, self.alpha_r, self.elog_r,
                    self.ws_small, self.scal[4:5])

    def _init_p(self, prior):
        """Initial parameters and <log P> table: the prior, given parameters (device), or the logs
        of a value / of a draw from the prior (host, set-up)."""
        rt, k = self.rt, self.kernels
        torch = rt.torch
        D, K, M = self.D, self.K, self.M
        init = self.P._init

        def major(a):       # (D, K, M) -> (M, D K)
            return torch.from_numpy(np.array(a.reshape(D * K, M).T, order='C')).to(rt.device)
        counts = None
        if init is not None and init[0] == 'parameters':
            a = np.asarray(init[1][0], dtype=np.float64)
            if np.any(a <= 0):
                raise ValueError("Natural parameters should be positive")
            counts = major(np.broadcast_to(a, (D, K, M)) - prior)
        k.dirichlet(D * K, M, 1, D * K, self.prior_p, counts, self.alpha_p, self.elog_p,
                    self.ws_small, self.scal[3:4])
        if init is None or init[0] == 'parameters':
            return
        if init[0] == 'value':
            p = np.broadcast_to(np.asarray(init[1], dtype=np.float64), (D, K, M))
        else:
            g = np.random.gamma(prior)
            p = g / g.sum(axis=-1, keepdims=True)
        with np.errstate(divide='ignore'):
            e = np.log(p)
        self.elog_p.copy_(major(e))
        self.alpha_p.fill_(float('nan'))                # a point mass has no parameters

    def _tables(self, elog_p):
        """The tables of the pass from ``elog_p`` (None: no observation term) and ``elog_r``."""
        self.kernels.tables(self.D, self.K, self.M, elog_p, self.elog_r, self.L, self.c)

    def _run_pass(self, r_out=None):
        """The statistics of the present ``Z`` state (tables ``L`` / ``c`` or labels)."""
        self.kernels.pass_(self.N, self.D, self.K, self.M, self.xb, self.labels, self.L, self.c,
                           self.ws, self.S, self.Nk, self.scal, r_out)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        rt, k = self.rt, self.kernels
        rt.sync_stream()
        D, K, M = self.D, self.K, self.M
        if node is self.Z:
            self.labels = None
            self._tables(self.elog_p)
            self._run_pass()
        elif node is self.P:
            k.dirichlet(D * K, M, 1, D * K, self.prior_p, self.S, self.alpha_p, self.elog_p,
                        self.ws_small, self.scal[3:4])
        elif node is self.R:
            k.dirichlet(1, K, K, 1, self.prior_r, self.Nk, self.alpha_r, self.elog_r,
                        self.ws_small, self.scal[4:5])
        else:
            return
        self._version += 1

    def _lower_bound_terms(self):
        self._materialize()
        if self._L_version != self._version:
            rt, k = self.rt, self.kernels
            rt.sync_stream()
            k.dot(self.M * self.D * self.K, self.S, self.elog_p, self.ws_small, self.scal[5:6])
            k.dot(self.K, self.Nk, self.elog_r, self.ws_small, self.scal[6:7])
            s = self.scal.cpu().numpy()
            entropy = 0.0 if self.labels is not None else float(s[0] - s[1] - s[2])
            t = dict(X=float(s[5]), Z=float(s[6]) + entropy, P=float(s[3]), R=float(s[4]))
            t['total'] = t['X'] + t['Z'] + t['P'] + t['R']
            self._L = t
            self._L_version = self._version
        return _delta.bound_terms(self._L, self._delta)

    def lower_bound_contribution(self, node):
        terms = self._lower_bound_terms()
        for key in ('X', 'Z', 'P', 'R'):
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

    def get_moments(self, node):
        self._materialize()
        if node is self.R:
            return [self.elog_r.cpu().numpy().reshape(self.R.plates + (self.K,)).copy()]
        if node is self.P:
            return [self.elog_p.cpu().numpy().reshape(self.M, self.D, self.K)
                    .transpose(1, 2, 0).copy()]
        if node is self.Z:
            return [self.responsibilities().cpu().numpy().reshape(self.N, 1, self.K)]
        if node is self.X:
            xb = self.xb.cpu().numpy()[:self.N * self.D].reshape(self.N, self.D)
            return [(xb[..., None] == np.arange(self.M)).astype(np.float64)]
        raise NotImplementedError

    def _host_mask(self):
        """The mask as a boolean host array of shape (N, D), or None without one."""
        m = self.X._mask
        return None if m is True else np.asarray(m, dtype=bool).reshape(self.N, self.D)

    def get_mask(self, node):
        """``X``: its mask; ``Z``: any entry of the row observed, (N, 1); ``P``: any entry of the
        column observed, (D, 1); ``R``: any entry observed -- the masks the reference propagates
        from ``X`` to its parents."""
        m = self._host_mask()
        if m is None:
            return np.array(True)
        if node is self.X:
            return m.copy()
        if node is self.Z:
            return m.any(axis=1)[:, None]
        if node is self.P:
            return m.any(axis=0)[:, None]
        return np.array(bool(m.any()))

    # -- persistence -----------------------------------------------------------------------------------
    _SAVED = ('alpha_p', 'elog_p', 'alpha_r', 'elog_r', 'L', 'c', 'S', 'Nk', 'scal')

    def save_state(self, put, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        _delta.save(put, base, self._delta)
        put(base + 'kind', np.array([ord(ch) for ch in 'cmm'], dtype=np.uint8))
        put(base + 'dims', np.array([self.N, self.D, self.K, self.M], dtype=np.int64))
        put(base + 'flags', np.array([1 if self.labels is not None else 0], dtype=np.int64))
        if self.labels is not None:
            put(base + 'labels', self.labels.cpu().numpy())
        if self.maskd is not None:
            put(base + 'mask', self.maskd.cpu().numpy())
        for name in self._SAVED:
            put(base + name, getattr(self, name).cpu().numpy())

    def load_state(self, reader, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        if not reader.has(base + 'kind') or bytes(np.asarray(reader.get(base + 'kind'),
                                                             dtype=np.uint8)) != b'cmm':
            raise Exception("File does not contain the state of the fused categorical-mixture "
                            "block")
        dims = tuple(int(v) for v in reader.get(base + 'dims'))
        if dims != (self.N, self.D, self.K, self.M):
            raise ValueError('checkpoint is for (N, D, K, M) = %s, the model has %s'
                             % (dims, (self.N, self.D, self.K, self.M)))
        saved = np.asarray(reader.get(base + 'mask'), dtype=np.uint8).reshape(-1) \
            if reader.has(base + 'mask') else None
        mine = None if self.maskd is None else self.maskd.cpu().numpy().reshape(-1)
        if (saved is None) != (mine is None) or (saved is not None
                                                 and not np.array_equal(saved != 0, mine != 0)):
            raise ValueError('checkpoint was saved with %s, the model has %s: observe X with the '
                             'mask of the checkpoint before loading it'
                             % tuple('no mask on X' if m is None else
                                     'a mask on X with %d of %d entries observed'
                                     % (int(np.count_nonzero(m)), m.size) for m in (saved, mine)))
        torch = self.rt.torch
        self._delta = _delta.load(reader, base)
        if int(np.asarray(reader.get(base + 'flags')).ravel()[0]):
            self.labels = torch.from_numpy(
                np.array(reader.get(base + 'labels'), dtype=np.int32)).to(self.rt.device)
        else:
            self.labels = None
        for name in self._SAVED:
            getattr(self, name).copy_(torch.from_numpy(
                np.array(reader.get(base + name), dtype=np.float64)).reshape(
                    getattr(self, name).shape).to(self.rt.device))
        self._version += 1
