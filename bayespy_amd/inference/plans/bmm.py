"""
Execution plan of the Bernoulli-mixture block (doc/source/examples/bmm.rst)

    R = Dirichlet(const);  Z = Categorical(R, plates=(N, 1))
    P = Beta(const [a, b], plates=(D, K));  X = Mixture(Z, Bernoulli, P);  X.observe(x)

with constant priors, K <= 64 and D <= 1024; ``X`` fully observed or observed with a mask of the
full shape (N, D) (below).  Opt-in: ``VB(...,
engine='fused')``; the default engine runs this model on the generic engine as before.  The plan
owns, in HBM: ``x`` as bits (ceil(D / 64) words per row), the Beta parameters and moments of ``P``
as a (D K, 2) table, those of ``R`` (K), the tables w = <log p> - <log(1 - p)> and c = <log pi> +
sum_d <log(1 - p)> the last ``Z`` update used, and the statistics S_dk = sum_n r_nk x_nd,
N_k = sum_n r_nk.  Nothing of size (N, D, K) or (N, K) exists: the responsibilities of ``Z`` are
formed inside ``vmp_bmm_pass`` and only on request written out (``Z.get_moments()``).

All plate terms of the lower bound follow from the statistics, sum_n lse_n and the tables:
    <log p(X)>           = sum_dk S_dk <log p_dk> + (N_k - S_dk) <log(1 - p_dk)>
    <log p(Z)> + entropy = sum_k N_k <log pi_k>
                           + sum_n lse_n - sum_k N_k c_used[k] - sum_dk S_dk w_used[d, k]

Masks: ``X.observe(x, mask=m)`` with ``m`` a boolean host array or a ``DeviceMask`` of shape
exactly (N, D).  The row then carries two bit planes, xm = x & m and m (N D / 4 bytes in all), and
the plan keeps ``M`` and ``l0`` beside ``S`` and ``w``:
    logit_nk = c[k] + sum_d xm_nd w[d, k] + sum_d m_nd l0[d, k],   l0 = <log(1 - p)>,
    c = <log pi> (less its maximum),  S_dk = sum_n r_nk xm_nd,  M_dk = sum_n r_nk m_nd,
    N_k = sum over the rows with an observed entry of r_nk,  message to P = (S, M - S).
The two bound formulas above hold on these sums with ``counts`` = (S, M - S) for the first and
S . w + M . l0 for the last product of the second.  A row with nothing observed has ``Z.mask``
False: its moment is softmax(<log pi>) of the tables the last update used and it enters neither
N_k nor the bound term of ``Z``.  A hidden position of ``x`` is never read by the kernels.  A
scalar mask or one that broadcasts over a plate is declined (generic engine).

Checkpoints: the block writes its own ``plans/<i>/`` group (kind 'bmm') like every fused plan.  A
checkpoint of the generic engine holds the natural parameters of every node, the (N, 1, K) array
of ``Z`` among them, which this block never keeps; the two are not interchangeable.  A masked plan
adds ``mask``, ``M`` and ``l0`` and refuses a checkpoint whose mask differs; an unmasked plan
writes what it always wrote.
"""
import ctypes

import numpy as np

from . import _delta
from ._dirichlet import DirichletKernels, prior_table

from ... import _lib
from ...device import get_runtime, ptr
from ...nodes.node import Constant, DeviceMask
from ...nodes.dirichlet import Dirichlet
from ...nodes.beta import Beta
from ...nodes.categorical import Categorical
from ...nodes.binomial import Bernoulli, Binomial
from ...nodes.mixture import Mixture

BMM_MAX_K = 64          # vmp_bmm_limits
BMM_MAX_D = 1024
BMM_MASKED_MAX_K = 64   # vmp_bmm_limits_masked as documented; the matcher reads the built values
BMM_MASKED_MAX_D = 1024

_DTYPES = {'float64': 0, 'int64': 1, 'bool': 2, 'uint8': 2}
_MASKED_LIMITS = []


def bmm_masked_limits():
    """(max K, max D) of the built masked pass: host-only ``vmp_bmm_limits_masked``."""
    if not _MASKED_LIMITS:
        k, d = ctypes.c_int32(), ctypes.c_int32()
        _lib.raise_for_status(_lib.load().vmp_bmm_limits_masked(ctypes.byref(k), ctypes.byref(d)))
        _MASKED_LIMITS.append((k.value, d.value))
    return _MASKED_LIMITS[0]


class BMMKernels(DirichletKernels):

    def __init__(self, rt):
        self.rt, self.lib, self.ctx = rt, rt.lib, rt.ctx

    def plan(self, N, D, K):
        """(rows of a chunk, workspace doubles) of the pass."""
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_bmm_plan(N, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused Bernoulli-mixture block supports K <= %d and '
                                      'D <= %d' % (BMM_MAX_K, BMM_MAX_D))
        return c.value, w.value

    def pack(self, N, D, dtype, x, xw, flag):
        self.rt.check(self.lib.vmp_bmm_pack(self.ctx, N, D, dtype, ptr(x), ptr(xw), ptr(flag)))

    def tables(self, D, K, elog_p, elog_pi, w, c):
        self.rt.check(self.lib.vmp_bmm_tables(self.ctx, D, K,
                                              ptr(elog_p) if elog_p is not None else None,
                                              ptr(elog_pi), ptr(w), ptr(c)))

    def pass_(self, N, D, K, xw, labels, w, c, ws, S, Nk, counts, scal, r_out=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_bmm_pass(self.ctx, N, D, K, p(xw), p(labels), p(w), p(c), p(ws),
                                            p(S), p(Nk), p(counts), p(scal), p(r_out)))

    # -- missing observations: two bit planes per row, tables (w, l0, c), statistics (S, M) --------
    def plan_masked(self, N, D, K):
        c, w = ctypes.c_int64(), ctypes.c_int64()
        rc = self.lib.vmp_bmm_plan_masked(N, D, K, ctypes.byref(c), ctypes.byref(w))
        if rc != _lib.VMP_OK:
            _lib.raise_for_status(rc, 'the fused Bernoulli-mixture block with a mask supports '
                                      'K <= %d and D <= %d' % bmm_masked_limits())
        return c.value, w.value

    def pack_masked(self, N, D, dtype, x, mask, xw, flag):
        self.rt.check(self.lib.vmp_bmm_pack_masked(self.ctx, N, D, dtype, ptr(x), ptr(mask),
                                                   ptr(xw), ptr(flag)))

    def tables_masked(self, D, K, elog_p, elog_pi, w, l0, c):
        self.rt.check(self.lib.vmp_bmm_tables_masked(self.ctx, D, K,
                                                     ptr(elog_p) if elog_p is not None else None,
                                                     ptr(elog_pi), ptr(w), ptr(l0), ptr(c)))

    def pass_masked(self, N, D, K, xw, labels, w, l0, c, ws, S, M, Nk, counts, scal, r_out=None):
        def p(t):
            return ptr(t) if t is not None else None
        self.rt.check(self.lib.vmp_bmm_pass_masked(self.ctx, N, D, K, p(xw), p(labels), p(w),
                                                   p(l0), p(c), p(ws), p(S), p(M), p(Nk),
                                                   p(counts), p(scal), p(r_out)))


def _mask_shape(mask):
    return tuple(mask.shape) if isinstance(mask, DeviceMask) else np.shape(mask)


def _takes_mask(X):
    """No mask, or one of the full shape of the plates of ``X``."""
    return X._mask is True or _mask_shape(X._mask) == tuple(X.plates)


def _match(nodes, why):
    for X in nodes:
        if not isinstance(X, Mixture) or not (isinstance(X.node_class, type)
                                              and issubclass(X.node_class, Binomial)):
            continue

        def no(msg, X=X):
            if why is not None:
                why.append('fused Bernoulli-mixture block, observed node %s: %s'
                           % (X.name or '<unnamed>', msg))
        if X.node_class is not Bernoulli:
            no('the mixed distribution is %s, not Bernoulli' % X.node_class.__name__)
            continue
        Z, P = X.parents[0], X.parents[1]
        if type(Z) is not Categorical or type(P) is not Beta \
                or not isinstance(Z.parents[0], Dirichlet) or type(Z.parents[0]) is not Dirichlet:
            no('its parents are not (Categorical(Dirichlet), Beta)')
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
            no('the parameter of %s is a node (%s), not a constant'
               % (bad[0].name, type(bad[0].parents[0]).__name__))
            continue
        if X.cluster_plate != -1 or len(X.plates) != 2 or len(P.plates) != 2:
            no('it needs plates (N, D) with the clusters on the last plate axis of P, X has plates '
               '%s and P has plates %s' % (X.plates, P.plates))
            continue
        N, D = X.plates
        K = X.clusters
        if Z.plates != (N, 1) or P.plates != (D, K) or any(p != 1 for p in R.plates):
            no('plates of Z / P / R are not (N, 1), (D, K), ()')
            continue
        if K > BMM_MAX_K or D > BMM_MAX_D:
            no('D = %d, K = %d exceed the limits of the block (D <= %d, K <= %d)'
               % (D, K, BMM_MAX_D, BMM_MAX_K))
            continue
        if X._mask is not True and (K > bmm_masked_limits()[0] or D > bmm_masked_limits()[1]):
            no('D = %d, K = %d exceed the limits of the block with a mask (D <= %d, K <= %d)'
               % ((D, K) + bmm_masked_limits()[::-1]))
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


class BernoulliMixturePlan:

    @staticmethod
    def describe():
        return ("Mixture(Categorical(Dirichlet(const), plates=(N, 1)), Bernoulli, Beta(const, "
                "plates=(D, K))), fully observed (D <= %d, K <= %d) or observed with a mask of "
                "the full shape (N, D) (D <= %d, K <= %d); a scalar mask or one that broadcasts "
                "over a plate is declined"
                % (BMM_MAX_D, BMM_MAX_K, BMM_MASKED_MAX_D, BMM_MASKED_MAX_K))

    @staticmethod
    def match(nodes, why=None):
        return _match(nodes, why)

    def __init__(self, roles, runtime=None, kernels=None):
        self.roles = roles
        self.X, self.Z, self.P, self.R = roles['X'], roles['Z'], roles['P'], roles['R']
        self.N, self.D = self.X.plates
        self.K = self.X.clusters
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
            self._kernels = BMMKernels(self.rt)
        return self._kernels

    def nodes(self):
        return list(self.roles.values())

    def has_state(self):
        return bool(self._ready)

    def invalidate(self, node):
        if node is self.X and node.observed and _takes_mask(node) \
                and (not self._ready or (node._mask is True) == (self.maskd is None)):
            # new observations of the same shape, with a mask of the full shape or none: the bits
            # are packed again, the posteriors stay
            self._x_stale = True
            self._version += 1
            return
        _delta.warn_state_discarded(self, node)
        self._ready = False
        self._version += 1
        if BernoulliMixturePlan.match(self.nodes()) is None:
            from .generic import GenericPlan
            GenericPlan(self.nodes())

    # -- set-up ------------------------------------------------------------------------------------
    def _pack(self):
        """``X._data`` as bits (with ``maskd``, uploaded before: two planes); a value that is neither 0 nor 1 is the reference's ValueError
        (binomial.py, through Bernoulli's observe)."""
        rt, torch = self.rt, self.rt.torch
        N, D = self.N, self.D
        x = self.X._data
        if x is None:
            raise ValueError('Node %s has not been observed' % self.X.name)
        if isinstance(x, torch.Tensor):
            t = x.to(rt.device)
            if str(t.dtype).replace('torch.', '') not in _DTYPES:
                t = t.to(torch.float64)
        else:
            a = np.asarray(x)
            if a.dtype.name not in _DTYPES:
                a = a.astype(np.float64)
            t = torch.from_numpy(np.array(np.broadcast_to(a, (N, D)), order='C')).to(rt.device)
        if tuple(t.shape) != (N, D) or not t.is_contiguous():
            t = t.expand(N, D).contiguous()
        dtype = _DTYPES[str(t.dtype).replace('torch.', '')]
        W = (D + 63) // 64
        planes = 1 if self.maskd is None else 2
        self.xw = torch.zeros(max(N, 1) * W * planes, dtype=torch.int64, device=rt.device)
        flag = torch.zeros(1, dtype=torch.int32, device=rt.device)
        if self.maskd is None:
            self.kernels.pack(N, D, dtype, t, self.xw, flag)
        else:
            self.kernels.pack_masked(N, D, dtype, t, self.maskd, self.xw, flag)
        if int(flag.cpu().numpy()[0]) != 0:
            raise ValueError("Invalid count")
        self._x_stale = False

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
        N, D, K = self.N, self.D, self.K
        rt.sync_stream()
        self._upload_mask()
        masked = self.maskd is not None
        self.chunk, wsd = k.plan_masked(N, D, K) if masked else k.plan(N, D, K)
        self._pack()
        up = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, order='C')).to(rt.device)  # noqa: E731
        pp = prior_table(self.P, (D, K, 2)).reshape(D * K, 2)
        pr = prior_table(self.R, (K,))
        self.prior_p, self.prior_r = up(pp), up(pr)
        self.alpha_p, self.elog_p = rt.empty(D * K, 2), rt.empty(D * K, 2)
        self.alpha_r, self.elog_r = rt.empty(K), rt.empty(K)
        self.w, self.c = rt.zeros(D, K), rt.zeros(K)
        self.S, self.Nk, self.counts = rt.zeros(D, K), rt.zeros(K), rt.zeros(D * K, 2)
        if masked:
            self.l0, self.M = rt.zeros(D, K), rt.zeros(D, K)
        self.ws = rt.empty(int(wsd))
        self.ws_small = rt.empty(max(D * K, 1024))
        # [0] sum lse, [1] N_k . c used, [2] S . w (+ M . l0) used, [3] bound of P, [4] bound of R,
        # [5] counts . <log p>, [6] N_k . <log pi>
        self.scal = rt.zeros(8)
        self._init_table(self.P, pp, D * K, 2, self.prior_p, self.alpha_p, self.elog_p,
                         self.scal[3:4])
        self._init_table(self.R, pr.reshape(1, K), 1, K, self.prior_r, self.alpha_r, self.elog_r,
                         self.scal[4:5])
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

    def _init_table(self, node, prior, rows, cols, prior_d, alpha, elog, bound):
        """Initial parameters and <log> table of a Beta / Dirichlet table: the prior, given
        parameters (device), or the logs of a value / of a draw from the prior (host, set-up)."""
        rt, k = self.rt, self.kernels
        torch = rt.torch
        init = node._init
        counts = None
        if init is not None and init[0] == 'parameters':
            a = np.asarray(init[1][0], dtype=np.float64)
            if np.any(a <= 0):
                raise ValueError("Natural parameters should be positive")
            a = np.broadcast_to(a, node.plates + (cols,)).reshape(rows, cols)
            counts = torch.from_numpy(np.array(a - prior, order='C')).to(rt.device)
        k.dirichlet(rows, cols, cols, 1, prior_d, counts, alpha, elog, self.ws_small, bound)
        if init is None or init[0] == 'parameters':
            return
        if init[0] == 'value':
            p = np.broadcast_to(np.asarray(init[1], dtype=np.float64), (self.D, self.K))
        else:
            p = np.random.beta(prior[:, 0], prior[:, 1]).reshape(self.D, self.K)
        with np.errstate(divide='ignore'):
            e = np.stack([np.log(p), np.log(1 - p)], -1)
        elog.copy_(torch.from_numpy(np.array(e.reshape(rows, cols), order='C')).to(rt.device))
        alpha.fill_(float('nan'))                    # a point mass has no parameters

    def _tables(self, elog_p):
        """The tables of the pass from ``elog_p`` (None: no observation term) and ``elog_r``."""
        if self.maskd is None:
            self.kernels.tables(self.D, self.K, elog_p, self.elog_r, self.w, self.c)
        else:
            self.kernels.tables_masked(self.D, self.K, elog_p, self.elog_r, self.w, self.l0,
                                       self.c)

    def _run_pass(self, r_out=None):
        """The statistics of the present ``Z`` state (tables ``w`` / ``c`` or labels)."""
        if self.maskd is None:
            self.kernels.pass_(self.N, self.D, self.K, self.xw, self.labels, self.w, self.c,
                               self.ws, self.S, self.Nk, self.counts, self.scal, r_out)
        else:
            self.kernels.pass_masked(self.N, self.D, self.K, self.xw, self.labels, self.w, self.l0,
                                     self.c, self.ws, self.S, self.M, self.Nk, self.counts,
                                     self.scal, r_out)
        self._version += 1

    # -- operations ----------------------------------------------------------------------------------
    def update(self, node):
        self._materialize()
        _delta.updated(self._delta, self.roles, node)
        rt, k = self.rt, self.kernels
        rt.sync_stream()
        D, K = self.D, self.K
        if node is self.Z:
            self.labels = None
            self._tables(self.elog_p)
            self._run_pass()
        elif node is self.P:
            k.dirichlet(D * K, 2, 2, 1, self.prior_p, self.counts, self.alpha_p, self.elog_p,
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
            k.dot(2 * self.D * self.K, self.counts, self.elog_p, self.ws_small, self.scal[5:6])
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
            return [self.elog_p.cpu().numpy().reshape(self.D, self.K, 2).copy()]
        if node is self.Z:
            return [self.responsibilities().cpu().numpy().reshape(self.N, 1, self.K)]
        if node is self.X:
            x = self.X._data
            x = x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x)
            return [np.array(np.broadcast_to(x, (self.N, self.D)), dtype=np.float64)]
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
    _SAVED = ('alpha_p', 'elog_p', 'alpha_r', 'elog_r', 'w', 'c', 'S', 'Nk', 'counts', 'scal')
    _SAVED_MASKED = ('M', 'l0')

    def _saved(self):
        return self._SAVED + (self._SAVED_MASKED if self.maskd is not None else ())

    def save_state(self, put, nodes, index):
        self._materialize()
        base = 'plans/%d/' % index
        _delta.save(put, base, self._delta)
        put(base + 'kind', np.array([ord(ch) for ch in 'bmm'], dtype=np.uint8))
        put(base + 'dims', np.array([self.N, self.D, self.K], dtype=np.int64))
        put(base + 'flags', np.array([1 if self.labels is not None else 0], dtype=np.int64))
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
                                                             dtype=np.uint8)) != b'bmm':
            raise Exception("File does not contain the state of the fused Bernoulli-mixture block")
        dims = tuple(int(v) for v in reader.get(base + 'dims'))
        if dims != (self.N, self.D, self.K):
            raise ValueError('checkpoint is for (N, D, K) = %s, the model has %s'
                             % (dims, (self.N, self.D, self.K)))
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
        for name in self._saved():
            getattr(self, name).copy_(torch.from_numpy(
                np.array(reader.get(base + name), dtype=np.float64)).reshape(
                    getattr(self, name).shape).to(self.rt.device))
        self._version += 1
