"""``SimpleGPModel``: one independent ARD-RBF GP per output dimension, evaluated on MI355X.

Mirrors the public surface of the reference class
/root/reference/safe_exploration/ssm_gpy/gaussian_process.py:15-634 (constructor signature,
``train`` / ``update_model`` / ``predict`` / ``predictive_gradients`` / ``__call__`` /
``to_dict`` / ``from_dict`` and the cached attributes ``z, beta, inv_K, hyp, kern_types, x_train,
y_train, gp_trained``), but none of its implementation: GPy is replaced by the C-ABI in
include/safereach.h (Gram + blocked fp64-MFMA Cholesky at model-update time; fused RBF
cross-covariance / triangular contraction kernels at prediction time).

Also provided, each through its own C entry point: ``opt_hyp=True`` (L-BFGS-B over ``sr_gp_mll``),
``choose_datapoints_maxvar`` (opt-in ``route="downdate"``: ``sr_gp_select_maxvar``), ``sample_from_gp`` (``sr_gp_sample``), ``information_gain`` (``sr_gp_logdet``),
``linearize_predict(jacobians=True)`` with ``get_reverse`` / ``get_linearize_reverse`` (``has_reverse`` is True).
Sparse GP regression (``do_sparse_gp = True``, GPy's ``SparseGPRegression``): ``train(X, y, m, Z=..., opt_hyp=False)`` fits
the DTC posterior of m inducing inputs over ALL of X, y through ``sr_gp_fit_sparse``; ``beta`` / ``inv_K`` are GPy's
``woodbury_vector`` / ``woodbury_inv`` and every prediction route works as on an exact model of m points.
Not provided: ``opt_hyp=True`` and ``information_gain()`` of a sparse model (NotImplementedError).
"""
import ctypes
import os
import warnings

import numpy as np
import torch

from .. import _buffers as B
from .._lib import lib, check, last_error, SR_EUNSUPPORTED, SR_EBUSY
from ..state_space_models import StateSpaceModel

_server_call = lib.sr_gp_server_call

GPY_JITTER = 1e-8   # GPy's exact inference adds this to diag(K) (from knowledge of GPy; unverifiable here)
SPARSE_JITTER = 1e-6   # GPy's VarDTC.const_jitter, added to diag(K_uu) (from knowledge of GPy; unverifiable here)
SELECT_ROUTES = ("predict", "downdate")   # choose_datapoints_maxvar(route=...)


class _Handle(object):
    """Owns one sr_gp_t; shared between deep copies of a model (state_space_models.py:166 deep-copies
    the SSM when handing it to CasADi -- the device state is immutable between updates)."""

    def __init__(self, device, N, D, n_out):
        self.device = device
        self.h = ctypes.c_void_p()
        check(lib.sr_gp_create(ctypes.byref(self.h), device.index, N, D, n_out))
        self.N, self.D, self.n_out = N, D, n_out
        self.shared = False              # set when a deep copy of the model holds this handle too
        self._server_armed = False       # SimpleGPModel.start_server
        npad = ctypes.c_long(0)
        check(lib.sr_gp_padded_n(self.h, ctypes.byref(npad)))
        self.Np = npad.value

    def __del__(self):
        try:
            if self.h:
                lib.sr_gp_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def Np_now(self):
        npad = ctypes.c_long()
        check(lib.sr_gp_padded_n(self.h, ctypes.byref(npad)))
        return npad.value

    def single_io(self):
        """Staging of the single-query (CasADi/IPOPT callback) entry points: one pinned host block in, one
        packed device block [mu | var | jac_mu | jac_var | hess_mu] out, one pinned host block back.  The way back is
        ``sr_publish`` + ``sr_wait_flag`` (results and a sequence number written into pinned memory by a kernel, the
        host spins on the number): ~4 us less per blocking call than a D2H copy + stream sync."""
        io = getattr(self, "_single_io", None)
        if io is None:
            n, D = self.n_out, self.D
            total = 2 * n + 2 * n * D + n * D * D
            io = {"h_in": torch.empty(D, dtype=torch.float64).pin_memory(),
                  "d_in": torch.empty((1, D), dtype=torch.float64, device=self.device),
                  "d_out": torch.empty(total, dtype=torch.float64, device=self.device),
                  "h_out": torch.empty(total, dtype=torch.float64).pin_memory(),
                  "h_flag": torch.zeros(1, dtype=torch.int64).pin_memory(), "seq": 0, "mailbox": True,
                  "direct": True}
            o = io["d_out"]
            io["mu"], io["var"] = o[:n], o[n:2 * n]
            io["jm"] = o[2 * n:2 * n + n * D]
            io["jv"] = o[2 * n + n * D:2 * n + 2 * n * D]
            io["hm"] = o[2 * n + 2 * n * D:]
            io["h_in_np"], io["h_out_np"] = io["h_in"].numpy(), io["h_out"].numpy()
            io["p_in"], io["p_out"], io["p_flag"] = B.ptr(io["h_in"]), B.ptr(io["h_out"]), B.ptr(io["h_flag"])
            io["srv_np"] = np.empty(total)                       # where sr_gp_server_call leaves its answer
            io["p_srv"] = ctypes.c_void_p(io["srv_np"].ctypes.data)
            self._single_io = io
        return io

    def call1(self, second_order, k, stream):
        """One blocking single query as ONE command (sr_gp_call1: the query, already in the pinned input block, travels
        in the kernel arguments; results and sequence number are written to the pinned block by the posterior kernel
        itself).  Returns the first k doubles of the packed result, or None where the library has no one-launch
        posterior for this model."""
        io = self._single_io
        if not io["mailbox"]:
            return None
        # The library declines (SR_EUNSUPPORTED) by padded size AND by what is asked (512 padded rows: second order only):
        # refusals are remembered per (padded size, order); a model whose padded size has changed is asked again.
        # io["direct"] = False with no refusal on record is a switch thrown by hand (measurements).
        so = int(bool(second_order))
        if not io["direct"]:
            off = io.get("direct_off")
            if not off or (self.Np_now(), so) in off:
                return None
        io["seq"] = seq = io["seq"] + 1
        rc = lib.sr_gp_call1(self.h, io["p_in"], second_order, io["p_out"], io["p_flag"], seq, stream.cuda_stream)
        if rc != 0:
            if rc != -5:                       # anything but SR_EUNSUPPORTED is an error of this call
                check(rc)
            if "not device-visible" in last_error():
                io["mailbox"] = False          # the pinned blocks are not mapped here: plain copies from now on
            else:
                npad = self.Np_now()
                io.setdefault("direct_off", set()).add((npad, so))
                io["direct_off_np"] = npad
            io["direct"] = False
            return None
        rc = lib.sr_wait_flag(io["p_flag"], seq, 5.0)
        if rc != 0:
            stream.synchronize()
            check(rc)
        return io["h_out_np"][:k].copy()

    def server_call(self, second_order, k):
        """One blocking single query through the RESIDENT server (sr_gp_server_call: the query in the pinned input block
        goes into the mailbox the resident workgroups poll; no launch).  Returns the first k doubles of the packed result,
        or None where no server is armed for this model (``SimpleGPModel.start_server``)."""
        if not self._server_armed:
            return None
        io = self._single_io
        rc = _server_call(self.h, io["p_in"], second_order, io["p_srv"], 5.0)
        if rc != 0:
            if rc != -5:                       # anything but SR_EUNSUPPORTED is an error of this call
                check(rc)
            self._server_armed = False         # the model outgrew the server (or it was stopped): the launched routes
            return None
        return io["srv_np"][:k].copy()

    def fetch(self, k, stream):
        """first k doubles of the packed device block -> NumPy (copy), blocking."""
        io = self._single_io
        if io["mailbox"]:
            io["seq"] += 1
            rc = lib.sr_publish(self.device.index or 0, B.ptr(io["d_out"]), int(k), B.ptr(io["h_out"]),
                                B.ptr(io["h_flag"]), io["seq"], ctypes.c_void_p(stream.cuda_stream))
            if rc == 0:
                rc = lib.sr_wait_flag(B.ptr(io["h_flag"]), io["seq"], 5.0)
                if rc == 0:
                    return io["h_out_np"][:k].copy()
                stream.synchronize()           # surfaces a failed kernel as the HIP error it is
                check(rc)
            io["mailbox"] = False              # the host block is not device-visible here: plain copies from now on
        io["h_out"][:k].copy_(io["d_out"][:k], non_blocking=True)
        stream.synchronize()
        return io["h_out_np"][:k].copy()


class _MomentMatchFn(torch.autograd.Function):
    """``SimpleGPModel.moment_match_device(m, S, differentiable=True)``: the forward is the plain call, the backward
    ``moment_match_vjp_device`` at the saved inputs.  Seeds of outputs nobody used arrive as None (= zero, the same bits)."""

    @staticmethod
    def forward(ctx, model, m, S):
        mu, cov, V = model.moment_match_device(m, S)
        hd = model._handle
        ctx.model = model
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(B.as_dev(m, hd.device), None if S is None else B.as_dev(S, hd.device))
        return mu, cov, V

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, mu_bar, cov_bar, V_bar):
        m, S = ctx.saved_tensors
        m_bar, S_bar = ctx.model.moment_match_vjp_device(m, S, mu_bar, cov_bar, V_bar)
        return None, m_bar, (None if S is None else S_bar)


class _PathsRolloutFn(torch.autograd.Function):
    """``SimpleGPModel.paths_rollout_diff_device(x0, K, k)``: the forward is ``paths_rollout_device``, the backward
    ``paths_rollout_vjp_device`` at the saved inputs and states.  An output nobody used has a zero seed: zero gradients."""

    @staticmethod
    def forward(ctx, model, x0, K, k):
        X_all = model.paths_rollout_device(x0, K, k)
        ctx.model = model
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x0, K, k, X_all)
        return X_all

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, X_bar):
        x0, K, k, X_all = ctx.saved_tensors
        if X_bar is None:
            X_bar = torch.zeros_like(X_all)
        x0_bar, K_bar, k_bar = ctx.model.paths_rollout_vjp_device(x0, K, k, X_all, X_bar)
        need = ctx.needs_input_grad
        return None, (x0_bar if need[1] else None), (K_bar if need[2] else None), (k_bar if need[3] else None)


class SimpleGPModel(StateSpaceModel):
    """GP dynamics model x_{t+1} - prior(x_t,u_t) ~ GP, one output per state dimension.

    Parameters follow ssm_gpy/gaussian_process.py:32-33.  ``hyp`` is a list (one dict per output)
    with the reference's keys ``"lengthscale"`` (D,) and ``"variance"``; the Gaussian noise
    variance may be given as ``"noise_variance"`` (GPy's GPRegression default 1.0 otherwise).
    ``device`` (extension) selects the GPU.
    """

    def __init__(self, n_s_out, n_s_in, n_u, X=None, y=None, m=None, kern_types=None, hyp=None,
                 train=False, Z=None, device=None):
        self.n_s_out = n_s_out
        self.n_s_in = n_s_in
        self.n_u = n_u
        self.gp_trained = False
        self.m = m
        self.Z = Z
        self.z = None
        self.x_train = None
        self.y_train = None
        self._beta = None
        self._inv_K = None
        self._inv_K_dev = None
        self._handle = None
        self._noise_diag = None
        self._z_fit = None           # the inputs / targets the device model is conditioned on (== z unless Z was
        self._y_z = None             # fixed by the caller): what a broadcast receiver has to be given
        self._device_arg = device
        self.do_sparse_gp = False
        self.z_fixed = Z is not None
        self._init_kernel_function(kern_types, hyp)
        if X is None or y is None:
            train = False
        # reverse mode is implemented (get_reverse / get_linearize_reverse below): CasadiSSMEvaluator reads both
        # flags from the model it wraps (state_space_models.py:166, 423-425)
        super(SimpleGPModel, self).__init__(n_s_out, n_u, has_jacobian=True, has_reverse=True)
        if train:
            self.train(X, y, m, Z=Z)

    # ------------------------------------------------------------------ construction helpers
    def _init_kernel_function(self, kern_types=None, hyp=None):
        """Kernel bookkeeping (ssm_gpy/gaussian_process.py:421-489, hyper-parameter key names of
        ``_create_hyp_dict`` :491-544).  Supported identifiers: "rbf", "mat52" (ARD over all inputs),
        "lin_rbf", "lin_mat52" (linear x stationary on input dimension 1 + ARD linear, the structure
        the reference's in-tree formulas evaluate: gp_models_utils_casadi.py:72-128)."""
        D = self.n_s_in + self.n_u
        if kern_types is None:
            kern_types = ["rbf"] * self.n_s_out
        if hyp is None:
            hyp = [None] * self.n_s_out
        if len(kern_types) != self.n_s_out or len(hyp) != self.n_s_out:
            raise ValueError("kern_types / hyp need one entry per output dimension")

        def vec(h, key, n, default=1.0):
            v = np.reshape(np.asarray(h.get(key, default), dtype=np.float64), (-1,))
            if v.size == 1:
                v = np.full(n, float(v[0]))
            if v.size != n:
                raise ValueError("{} needs {} entries".format(key, n))
            return v

        def scal(h, key, default=1.0):
            return float(np.asarray(h.get(key, default), dtype=np.float64).reshape(-1)[0])

        hyp_out = []
        self._noise = np.empty(self.n_s_out)
        # keys given by the caller stay fixed under opt_hyp=True (the reference fixes them in GPy, :478-486)
        self._hyp_fixed = [set(h.keys()) if h is not None else set() for h in hyp]
        for i in range(self.n_s_out):
            kt = kern_types[i]
            h = dict(hyp[i]) if hyp[i] is not None else {}
            self._noise[i] = scal(h, "noise_variance")
            if kt in ("rbf", "mat52"):
                hyp_out.append({"lengthscale": vec(h, "lengthscale", D), "variance": scal(h, "variance")})
            elif kt in ("lin_rbf", "lin_mat52"):
                st = "rbf" if kt == "lin_rbf" else "mat52"
                hyp_out.append({"prod.%s.lengthscale" % st: vec(h, "prod.%s.lengthscale" % st, 1),
                                "prod.%s.variance" % st: scal(h, "prod.%s.variance" % st),
                                "prod.linear.variances": vec(h, "prod.linear.variances", 1),
                                "linear.variances": vec(h, "linear.variances", D)})
            else:
                raise ValueError("kernel type '{}' not supported".format(kt))
        self.kern_types = list(kern_types)
        self.hyp = hyp_out

    def _pack_kernel_params(self, only=None):
        """(n_out, 3+3D) packed parameters of sr_gp_set_data_general:
        [kappa, v, c0, s[D], a[D], b[D]] with k = (c0 + sum a x y) v kappa(r) + sum b x y.
        ``only=i`` packs output i alone (1, 3+3D)."""
        D = self.n_s_in + self.n_u
        pairs = list(zip(self.kern_types, self.hyp)) if only is None else [(self.kern_types[only], self.hyp[only])]
        kp = np.zeros((len(pairs), 3 + 3 * D))
        for i, (kt, h) in enumerate(pairs):
            if kt in ("rbf", "mat52"):
                kp[i, 0] = 0.0 if kt == "rbf" else 1.0
                kp[i, 1], kp[i, 2] = h["variance"], 1.0
                kp[i, 3:3 + D] = 1.0 / h["lengthscale"]
            else:
                st = "rbf" if kt == "lin_rbf" else "mat52"
                kp[i, 0] = 0.0 if st == "rbf" else 1.0
                kp[i, 1], kp[i, 2] = h["prod.%s.variance" % st], 0.0
                kp[i, 3 + 1] = 1.0 / h["prod.%s.lengthscale" % st][0]          # stationary factor: input dim 1
                kp[i, 3 + D + 1] = h["prod.linear.variances"][0]               # product-linear factor: dim 1
                kp[i, 3 + 2 * D:3 + 3 * D] = h["linear.variances"]
        return kp

    @classmethod
    def from_dict(cls, gp_dict):
        """ssm_gpy/gaussian_process.py:72-133 (same keys)."""
        x = y = None
        data_available = False
        if gp_dict.get("data_path") is not None:
            data = np.load(gp_dict["data_path"])
            x, y = data["S"], data["y"]
            data_available = True
        elif "x" in gp_dict and "y" in gp_dict:
            x, y = gp_dict["x"], gp_dict["y"]
            data_available = True
        else:
            warnings.warn("GP needs a data_path or the data itself (keys 'x' and 'y'); "
                          "instantiating without training")
        if "prior_model" in gp_dict and data_available:
            y = y - gp_dict["prior_model"](x)
        train = bool(gp_dict.get("train", False)) and data_available
        return cls(gp_dict["n_s_out"], gp_dict["n_s_in"], gp_dict["n_u"], x, y, gp_dict.get("m"),
                   gp_dict.get("kern_types"), gp_dict.get("hyp"), train, gp_dict.get("Z"),
                   device=gp_dict.get("device"))

    def to_dict(self):
        """ssm_gpy/gaussian_process.py:177-187 (same keys)."""
        return {"x": self.x_train, "y": self.y_train, "kern_types": self.kern_types,
                "hyp": self.hyp, "beta": self.beta, "inv_K": self.inv_K}

    def __deepcopy__(self, memo):
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            new.__dict__[k] = v          # arrays are replaced, never mutated, on update
        if self._handle is not None:
            self._handle.shared = True   # from now on updates build a new handle instead of touching this one
        return new

    # ------------------------------------------------------------------ training
    def _select_subset(self, X, y, m, Z, choose_data, noise_diag=1e-5):
        n_data = X.shape[0]
        if m is None or n_data < m:
            if m is not None:
                warnings.warn("The desired number of datapoints is not available. Dataset consist "
                              "of {} Datapoints!".format(n_data))
            return X, y
        if choose_data:
            return self.choose_datapoints_maxvar(X, y, m, noise_diag=noise_diag)
        idx = np.random.choice(n_data, size=m, replace=False)
        return X[idx, :], y[idx, :]

    # route of choose_datapoints_maxvar when a call names none (set_select_route)
    _select_route = "predict"

    def set_select_route(self, route):
        """Route of ``choose_datapoints_maxvar`` for this model when a call names none -- what ``train(m=...)`` and
        ``update_model`` use: "predict" (the default) or "downdate" (``sr_gp_select_maxvar``)."""
        if route not in SELECT_ROUTES:
            raise ValueError("route must be one of {}".format(SELECT_ROUTES))
        self._select_route = route

    def choose_datapoints_maxvar(self, x, y, m, k=10, min_ratio_k=0.25, n_reopt_gp=1, init_idx=None,
                                 noise_diag=1e-5, return_index=False, route=None, return_scores=False):
        """Choose m datapoints by the maximum-predicted-variance criterion  (gaussian_process.py:280-345).

        Same scheme as the reference: k-means picks ``k`` seed points (one random member per cluster), then
        the point of the remaining pool with the largest summed posterior variance under the GP conditioned on
        the points chosen so far is added, m - k times.  Here every round is one batched ``sr_gp_predict`` over
        the whole pool (resident on the device) and one row append ``sr_gp_append`` -- no refactorisation.
        Differences, both forced: hyper-parameters are fixed (the reference re-optimises them on the pool
        ``n_reopt_gp`` times, :327-328, which also makes those rounds score the pool with a GP conditioned on
        the pool itself), and the seed set is random (k-means + ``np.random.choice``) unless ``init_idx`` is
        given.

        ``route``: "predict" (the loop above), "downdate" (``sr_gp_select_maxvar``: the same greedy rule as pivoted
        Cholesky downdates of K_pool + noise on the device -- one launch per round, one read-back at the end, then one fit
        on the chosen rows) or None (the model's, ``set_select_route``: "predict" unless set).  ``return_scores=True``
        (downdate route only) appends the m scores sum_d var_d(pick) just before each pick (None when n_data <= m)."""
        route = self._select_route if route is None else route
        if route not in SELECT_ROUTES:
            raise ValueError("route must be one of {}".format(SELECT_ROUTES))
        if return_scores and route != "downdate":
            raise ValueError("return_scores needs route='downdate'")
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        n_data = x.shape[0]
        if n_data <= m:
            out = (x, y, np.arange(n_data)) if return_index else (x, y)
            return out + (None,) if return_scores else out
        if init_idx is None:
            from sklearn import cluster
            k = int(np.minimum(int(n_data * min_ratio_k), k))
            clust_ids = cluster.KMeans(n_clusters=k, n_init=10).fit_predict(x)
            init_idx = [int(np.random.choice(np.nonzero(clust_ids == c)[0])) for c in np.unique(clust_ids)]
        chosen = [int(i) for i in init_idx][:m]
        if len(set(chosen)) != len(chosen) or min(chosen) < 0 or max(chosen) >= n_data:
            raise ValueError("init_idx must hold distinct row indices of x")
        if route == "downdate":
            return self._choose_downdate(x, y, m, chosen, noise_diag, return_index, return_scores)
        self._fit(x[chosen], y[chosen], noise_diag)
        self._noise_diag = noise_diag
        self.gp_trained = True
        hd = self._handle
        s = B.stream_ptr(hd.device)
        tx, ty = B.as_dev(x, hd.device), B.as_dev(y, hd.device)
        taken = torch.zeros(n_data, dtype=torch.bool, device=hd.device)
        taken[torch.as_tensor(chosen, device=hd.device)] = True
        info = (ctypes.c_int * self.n_s_out)()
        npad = ctypes.c_long(0)
        while len(chosen) < m:
            _, var = self.predict_device(tx)
            score = var.sum(dim=1).masked_fill_(taken, -float("inf"))
            j = int(torch.argmax(score))
            chosen.append(j)
            taken[j] = True
            check(lib.sr_gp_append(hd.h, B.ptr(tx[j:j + 1]), B.ptr(ty[j:j + 1]), 1, s, info))
            hd.N += 1
            check(lib.sr_gp_padded_n(hd.h, ctypes.byref(npad)))
            hd.Np = npad.value
        idx = np.asarray(chosen)
        self.z, self.x_train, self.y_train = x[idx], x, y         # the model now is the GP on the chosen rows
        self._z_fit, self._y_z = x[idx], y[idx]
        self._beta = self._inv_K = self._inv_K_dev = None
        return (x[idx], y[idx], idx) if return_index else (x[idx], y[idx])

    def _choose_downdate(self, x, y, m, chosen, noise_diag, return_index, return_scores):
        """choose_datapoints_maxvar(route="downdate"): a fit on the seeds puts kernel and noise on the handle, one
        sr_gp_select_maxvar over the pool, one read-back of picks and scores, one fit on the chosen rows in pick order."""
        self._fit(x[chosen], y[chosen], noise_diag)
        hd = self._handle
        tx = B.as_dev(x, hd.device)
        seeds = torch.as_tensor(np.asarray(chosen, dtype=np.int32), device=hd.device)
        out = B.empty((m + (m + 1) // 2,), hd.device)          # [scores: m doubles | picks: m int32]
        check(lib.sr_gp_select_maxvar(hd.h, B.ptr(tx), x.shape[0], m, B.ptr(seeds), len(chosen),
                                      B.ptr(out[m:].view(torch.int32)), B.ptr(out), B.stream_ptr(hd.device)))
        host = B.to_numpy(out)
        scores = host[:m].copy()
        idx = host[m:].view(np.int32)[:m].astype(np.int64)
        self._fit(x[idx], y[idx], noise_diag)
        self._noise_diag = noise_diag
        self.gp_trained = True
        self.z, self.x_train, self.y_train = x[idx], x, y
        self._z_fit, self._y_z = x[idx], y[idx]
        self._beta = self._inv_K = self._inv_K_dev = None
        res = (x[idx], y[idx], idx) if return_index else (x[idx], y[idx])
        return res + (scores,) if return_scores else res

    def train(self, X, y, m=None, opt_hyp=True, noise_diag=1e-5, Z=None, choose_data=True):
        """Condition the GPs on data (ssm_gpy/gaussian_process.py:189-278).

        ``opt_hyp=True`` maximises the exact marginal likelihood over the hyper-parameters the caller did not fix
        (``optimize_hyperparameters``; the reference calls GPy's ``optimize`` there, :249-250)."""
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if X.ndim != 2 or y.ndim != 2 or X.shape[0] != y.shape[0]:
            raise ValueError("X must be (N, n_s_in+n_u) and y (N, n_s_out)")
        if X.shape[1] != self.n_s_in + self.n_u or y.shape[1] != self.n_s_out:
            raise ValueError("X must be (N, n_s_in+n_u) and y (N, n_s_out)")
        if self.do_sparse_gp:
            self._train_sparse(X, y, m, opt_hyp, noise_diag, Z, choose_data)
            return
        Zs, yz = self._select_subset(X, y, m, Z, choose_data, noise_diag)
        if opt_hyp:
            self.optimize_hyperparameters(Zs, yz)
        self._fit(Zs, yz, noise_diag)
        self._noise_diag = noise_diag
        self._z_fit, self._y_z = Zs, yz
        self.z = self.Z if self.z_fixed else Zs
        self.x_train = X
        self.y_train = y
        self.gp_trained = True

    def _train_sparse(self, X, y, m, opt_hyp, noise_diag, Z, choose_data, jitter=None):
        """``do_sparse_gp``: m inducing inputs -- the caller's ``Z`` (gaussian_process.py:204) or the rows
        ``_select_subset`` picks -- summarise all of X, y (``sr_gp_fit_sparse``; GPy's SparseGPRegression posterior,
        :224-243).  The likelihood variance is sigma_n^2 + noise_diag (:252-253)."""
        if m is None:
            raise ValueError("Number of inducing points m needs to be specified for sparse gp regression")
        if opt_hyp:
            raise NotImplementedError("opt_hyp=True with do_sparse_gp: the variational bound is not optimised here")
        if Z is not None:
            Zu = np.ascontiguousarray(Z, dtype=np.float64)
            if Zu.ndim != 2 or Zu.shape[1] != X.shape[1]:
                raise ValueError("Z must be (m, n_s_in+n_u)")
            if X.shape[0] < Zu.shape[0]:
                raise ValueError("sparse GP regression needs at least as many data rows as inducing inputs")
        else:
            Zu, _ = self._select_subset(X, y, m, None, choose_data, noise_diag)
        self._fit_sparse(Zu, X, y, noise_diag, SPARSE_JITTER if jitter is None else jitter)
        self._noise_diag = noise_diag
        # the device model is a model of the m inducing rows; they carry no targets of their own
        self._z_fit, self._y_z = Zu, np.zeros((Zu.shape[0], self.n_s_out))
        self.z = Zu
        self._m_sparse = m
        self.x_train = X
        self.y_train = y
        self.gp_trained = True

    def _fit_sparse(self, Zu, X, Y, noise_diag, jitter):
        dev = B.resolve_device(self._device_arg)
        m, D = Zu.shape
        old = self._handle
        if (old is not None and not old.shared and (old.N, old.D, old.n_out) == (m, D, self.n_s_out)
                and old.device == dev and old.Np_now() == old.Np):
            handle = old
        else:
            handle = _Handle(dev, m, D, self.n_s_out)
        s2 = self._noise + float(noise_diag)
        s = B.stream_ptr(dev)
        self._set_data(handle, Zu, np.zeros((m, self.n_s_out)), s2, dev, s)
        if getattr(self, "_sparse_chunk", None) is not None:
            check(lib.sr_gp_set_chunk(handle.h, self._sparse_chunk))
        tx = B.as_dev(np.ascontiguousarray(X, dtype=np.float64), dev)
        ty = B.as_dev(np.ascontiguousarray(Y, dtype=np.float64), dev)
        info = (ctypes.c_int * self.n_s_out)()
        check(lib.sr_gp_fit_sparse(handle.h, B.ptr(tx), B.ptr(ty), X.shape[0], float(jitter), s, info))
        self._handle = handle
        self._beta = None
        self._inv_K = None
        self._inv_K_dev = None
        if old is not None and old is not handle and getattr(old, "_server_armed", False):
            try:
                self.start_server(old._server_idle)
            except RuntimeError as e:
                warnings.warn("resident server not re-armed after the model update: {}".format(e))

    def set_sparse_chunk(self, chunk):
        """Data rows per streamed chunk of the following sparse fits (``sr_gp_set_chunk``; at most 16384 are used)."""
        if int(chunk) < 1:
            raise ValueError("chunk must be positive")
        self._sparse_chunk = int(chunk)

    @property
    def is_sparse(self):
        return self._handle is not None and lib.sr_gp_is_sparse(self._handle.h) == 1

    def _free_hyp(self, i):
        """[(key, size)] of the hyper-parameters of output i that ``opt_hyp`` may move: everything the caller
        did not pass in ``hyp`` (ssm_gpy/gaussian_process.py:478-486 fixes what was passed), noise included."""
        return [(k, int(np.size(v))) for k, v in list(self.hyp[i].items()) + [("noise_variance", self._noise[i])]
                if k not in self._hyp_fixed[i]]

    def neg_log_marginal_likelihood(self, Z, Y, i, with_grad=True):
        """nll of output i on (Z, Y[:, i]) at the current hyper-parameters and its gradient with respect to the
        FREE hyper-parameters (natural scale, order of ``_free_hyp``), through sr_gp_factorize + sr_gp_mll.
        Noise term as during GPy's optimisation: sigma_n^2 + 1e-8, no ``noise_diag``.  Returns (inf, None) when
        K_y is not positive definite at these hyper-parameters."""
        dev = B.resolve_device(self._device_arg)
        Z = np.asarray(Z, dtype=np.float64)
        N, D = Z.shape
        hd = getattr(self, "_mll_handle", None)
        if hd is None or (hd.N, hd.D, hd.device) != (N, D, dev):
            hd = self._mll_handle = _Handle(dev, N, D, 1)      # reused by every evaluation of the optimiser
        s = B.stream_ptr(dev)
        tz = B.as_dev(Z, dev)
        ty = B.as_dev(np.ascontiguousarray(np.asarray(Y, dtype=np.float64)[:, i:i + 1]), dev)
        tk = B.as_dev(self._pack_kernel_params(only=i), dev)
        tn = B.as_dev(np.array([self._noise[i] + GPY_JITTER]), dev)
        check(lib.sr_gp_set_data_general(hd.h, B.ptr(tz), B.ptr(ty), B.ptr(tk), B.ptr(tn), s))
        info = (ctypes.c_int * 1)()
        if lib.sr_gp_factorize(hd.h, s, info) != 0:
            return np.inf, None
        nll, g = B.empty((1,), dev), B.empty((3 + 3 * D,), dev)
        check(lib.sr_gp_mll(hd.h, B.ptr(nll), B.ptr(g), s))
        nll, g = float(nll.item()), B.to_numpy(g)
        if not with_grad:
            return nll, None
        kt, h = self.kern_types[i], self.hyp[i]
        full = {"noise_variance": np.array([g[-1]])}
        if kt in ("rbf", "mat52"):
            full["variance"] = np.array([g[0]])
            full["lengthscale"] = -g[2:2 + D] / h["lengthscale"] ** 2            # s = 1 / lengthscale
        else:
            st = "rbf" if kt == "lin_rbf" else "mat52"
            full["prod.%s.variance" % st] = np.array([g[0]])
            full["prod.%s.lengthscale" % st] = np.array([-g[2 + 1] / h["prod.%s.lengthscale" % st][0] ** 2])
            full["prod.linear.variances"] = np.array([g[2 + D + 1]])
            full["linear.variances"] = g[2 + 2 * D:2 + 3 * D]
        free = self._free_hyp(i)
        return nll, (np.concatenate([full[k] for k, _ in free]) if free else np.zeros(0))

    def _get_free(self, i):
        vals = dict(self.hyp[i], noise_variance=self._noise[i])
        free = self._free_hyp(i)
        return np.concatenate([np.reshape(vals[k], (-1,)) for k, _ in free]) if free else np.zeros(0)

    def _set_free(self, i, theta):
        pos = 0
        for k, n in self._free_hyp(i):
            v = np.asarray(theta[pos:pos + n], dtype=np.float64)
            pos += n
            if k == "noise_variance":
                self._noise[i] = float(v[0])
            elif np.ndim(self.hyp[i][k]) == 0:
                self.hyp[i][k] = float(v[0])
            else:
                self.hyp[i][k] = v.copy()

    def optimize_hyperparameters(self, Z, Y, max_iters=1000):
        """Maximum-likelihood hyper-parameters per output (what ``model_gp.optimize(max_iters=1000)`` does in
        ssm_gpy/gaussian_process.py:249-250): L-BFGS-B (scipy) over the logarithms of the free parameters,
        every objective/gradient evaluation is one factorisation + ``sr_gp_mll`` on the device.  GPy's own
        parameter transformation and stopping rule are not reproduced (GPy is not available: parity unpinned
        at that boundary); the optimum of the same likelihood is."""
        from scipy import optimize
        for i in range(self.n_s_out):
            if not self._free_hyp(i):
                continue
            start = self._get_free(i)

            def fun(phi):
                self._set_free(i, np.exp(np.clip(phi, -25.0, 25.0)))
                nll, g = self.neg_log_marginal_likelihood(Z, Y, i)
                if not np.isfinite(nll):
                    return 1e25, np.zeros_like(phi)
                return nll, g * np.exp(np.clip(phi, -25.0, 25.0))

            res = optimize.minimize(fun, np.log(start), jac=True, method="L-BFGS-B",
                                    options={"maxiter": int(max_iters)})
            best = np.exp(np.clip(res.x, -25.0, 25.0))
            self._set_free(i, best if np.isfinite(res.fun) and res.fun < 1e24 else start)
        self._mll_handle = None
        return self.hyp

    RETIRE_RULES = ("oldest", "redundant")   # update_model(n_max=..., retire=...)

    def update_model(self, x, y, opt_hyp=False, replace_old=True, noise_diag=1e-5, choose_data=True, n_max=None,
                     retire="oldest"):
        """ssm_gpy/gaussian_process.py:347-419.

        ``n_max`` (extension; None = the reference's behaviour): with ``replace_old=False`` the model keeps at most ``n_max``
        training rows -- after the new rows are in, rows are retired (``remove_data``: O(N^2) each, no refit) until
        N <= n_max.  ``retire="oldest"`` retires row 0 (a sliding window); ``"redundant"`` retires the row whose removal
        changes the posterior mean least, the first argmin over j of sum_d alpha_dj^2 var_loo[d, j] (the Csato-Opper score
        summed over the outputs).  Where the call refits instead of appending, the same rows are dropped on the host first
        (a sparse model, ``m`` or a fixed ``Z``: always the oldest ones -- the score is that of the exact model)."""
        if retire not in self.RETIRE_RULES:
            raise ValueError("retire must be one of {}, not {!r}".format(self.RETIRE_RULES, retire))
        if n_max is not None and (int(n_max) != n_max or int(n_max) < 1):
            raise ValueError("n_max must be a positive integer or None")
        x = np.asarray(x, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if (not self.do_sparse_gp and not replace_old and not opt_hyp and self.gp_trained and self._handle is not None
                and not self._handle.shared and self.m is None and self.x_train is not None and not self.z_fixed
                and noise_diag == self._noise_diag and 0 < x.shape[0] <= self._append_limit_now()):
            self._append(x, y)                       # O(N^2 m) block row append instead of O(N^3)
            while n_max is not None and self._handle.N > int(n_max):
                self.remove_data(0 if retire == "oldest" else self._most_redundant())
            return
        if not replace_old and self.x_train is not None:
            x = np.vstack((self.x_train, x))
            y = np.vstack((self.y_train, y))
            if n_max is not None and x.shape[0] > int(n_max):
                # the refit route drops the same rows on the host: the oldest ones, or, one at a time, the most redundant
                # row of an exact fit of what is left (as the append route scores them)
                if retire == "oldest" or self.do_sparse_gp or self.m is not None or self.z_fixed:
                    x, y = x[x.shape[0] - int(n_max):], y[y.shape[0] - int(n_max):]
                else:
                    self.train(x, y, None, opt_hyp=False, noise_diag=noise_diag, choose_data=choose_data)
                    while self._handle.N > int(n_max):
                        self.remove_data(self._most_redundant())
                    if not opt_hyp:
                        return
                    x, y = self.x_train, self.y_train
        m = self.m
        if m is None and self.do_sparse_gp:
            m = getattr(self, "_m_sparse", None)         # a sparse model keeps its size: refit over the grown / replaced data
        self.train(x, y, m, opt_hyp=opt_hyp, noise_diag=noise_diag, Z=self.Z,
                   choose_data=choose_data)

    # More new points than this: refactorise.  None = by model size, N / 5 (at least 16): measured break-even of
    # update_model(replace_old=False), appends in chunks of 128 against a refit of everything -- N = 300: ~50 points,
    # 1000: ~200, 2000: ~350, 5000: ~1000, 10000: > 1024.  (Round 2's fixed 1024 appended 512 points to an N = 1000 model
    # in 2.7 ms where the refit takes 1.2.)  An integer fixes it.
    append_limit = None

    def _append_limit_now(self):
        if self.append_limit is not None:
            return int(self.append_limit)
        return max(16, int(self.x_train.shape[0]) // 5)

    def _append(self, x, y):
        """Condition on additional points through sr_gp_append (chunks of <= 128 rows)."""
        if x.ndim != 2 or y.ndim != 2 or x.shape[0] != y.shape[0] or x.shape[1] != self.n_s_in + self.n_u \
                or y.shape[1] != self.n_s_out:
            raise ValueError("x must be (n, n_s_in+n_u) and y (n, n_s_out)")
        hd = self._handle
        s = B.stream_ptr(hd.device)
        # <= 16 rows per call take the matrix-vector shaped path of sr_gp_append (0.29-0.57 ms at N = 5000; one point on <= 512 padded rows: one launch), more rows
        # go 128 at a time through its MFMA path
        step = 16 if x.shape[0] <= 16 else 128
        for lo in range(0, x.shape[0], step):
            xs, ys = x[lo:lo + step], y[lo:lo + step]
            info = (ctypes.c_int * self.n_s_out)()
            rc = None
            if xs.shape[0] == 1 and getattr(hd, "_append1_off_np", None) != hd.Np:
                # one point (the exploration loop, exploration_runner.py:186-188): it travels in the kernel arguments, status
                # and log det come back through a pinned block -- no copy command either way (sr_gp_append1_host)
                xr, yr = np.ascontiguousarray(xs[0]), np.ascontiguousarray(ys[0])
                rc = lib.sr_gp_append1_host(hd.h, ctypes.c_void_p(xr.ctypes.data), ctypes.c_void_p(yr.ctypes.data), s, info)
                if rc == SR_EUNSUPPORTED:
                    hd._append1_off_np = hd.Np       # not for this padded size: the general route from now on
                    rc = None
                elif rc == SR_EBUSY:
                    rc = None                        # this time only (the grid did not assemble): stage the point
            if rc is not None:
                check(rc)
            elif xs.shape[0] <= 16:
                # one pinned block, one H2D copy for both arrays (two pageable copies cost 35 us of the 125 us of a
                # one-point append); sr_gp_append returns after its own stream synchronisation, the block is free again
                st = getattr(hd, "_staging", None)
                if st is None:
                    st = hd._staging = B.Staging(hd.device)
                (tx, ty), _ = st.stage([np.ascontiguousarray(xs), np.ascontiguousarray(ys)], [])
            else:
                tx, ty = B.as_dev(xs, hd.device), B.as_dev(ys, hd.device)
            # a failing chunk (SR_ENOTPD on a near-duplicate point, out of memory) leaves the handle as it was
            # before THAT chunk: the host state below is committed chunk by chunk, so both always agree
            if rc is None:
                check(lib.sr_gp_append(hd.h, B.ptr(tx), B.ptr(ty), xs.shape[0], s, info))
            hd.N += xs.shape[0]
            npad = ctypes.c_long(0)
            check(lib.sr_gp_padded_n(hd.h, ctypes.byref(npad)))
            hd.Np = npad.value
            self.x_train, self.y_train = self._grown(self.x_train, xs, self.y_train, ys)
            self.z = self.x_train
            self._z_fit, self._y_z = self.x_train, self.y_train
            self._beta = None
            self._inv_K = None
            self._inv_K_dev = None

    def _check_remove_idx(self, idx):
        """idx (int or sequence of ints) -> sorted unique array of row indices; ValueError before the device is touched."""
        if self.x_train is None or not self.gp_trained:
            raise ValueError("remove_data: the model holds no training data")
        arr = np.atleast_1d(np.asarray(idx))
        if arr.ndim != 1 or arr.size == 0 or arr.dtype.kind not in "iu":
            raise ValueError("remove_data: idx must be an int or a non-empty sequence of ints")
        n = int(self.x_train.shape[0])
        arr = arr.astype(np.int64)
        if arr.min() < 0 or arr.max() >= n:
            raise ValueError("remove_data: index outside [0, {})".format(n))
        if np.unique(arr).size != arr.size:
            raise ValueError("remove_data: an index is given twice")
        if arr.size >= n:
            raise ValueError("remove_data: at least one training row must stay")
        return np.sort(arr)

    def remove_data(self, idx):
        """Retire training rows ``idx`` (an int or a sequence of distinct indices into the current ``x_train``) without
        refitting: ``sr_gp_remove``, O(N^2) per row.  The model is then the one a fit on the remaining rows, in their old
        order, gives.  Where the row append would not apply either (sparse model, handle shared with a deep copy, ``m`` set,
        fixed ``Z``) the remaining rows are refitted instead."""
        arr = self._check_remove_idx(idx)
        keep = np.ones(self.x_train.shape[0], dtype=bool)
        keep[arr] = False
        hd = self._handle
        if (self.do_sparse_gp or hd is None or hd.shared or self.m is not None or self.z_fixed
                or self.x_train.shape[0] != hd.N):
            m = self.m
            if m is None and self.do_sparse_gp:
                m = getattr(self, "_m_sparse", None)
            if m is not None:
                m = min(int(m), int(keep.sum()))
            self.train(self.x_train[keep], self.y_train[keep], m, opt_hyp=False,
                       noise_diag=self._noise_diag if self._noise_diag is not None else 1e-5, Z=self.Z)
            return
        cidx = (ctypes.c_int * arr.size)(*[int(i) for i in arr])
        check(lib.sr_gp_remove(hd.h, cidx, int(arr.size), B.stream_ptr(hd.device)))
        hd.N -= int(arr.size)
        hd.Np = hd.Np_now()
        self.x_train, self.y_train = self._shrunk(keep)
        self.z = self.x_train
        self._z_fit, self._y_z = self.x_train, self.y_train
        self._beta = None
        self._inv_K = None
        self._inv_K_dev = None

    def _shrunk(self, keep):
        """x_train[keep], y_train[keep] -- compacted inside the buffers of ``_grown`` where the training set lives there (the
        next append then finds its room as before)"""
        x0, y0 = self.x_train, self.y_train
        bufs = getattr(self, "_train_bufs", None)
        xk, yk = x0[keep], y0[keep]
        if (bufs is not None and x0.base is bufs[0] and y0.base is bufs[1]
                and x0.ctypes.data == bufs[0].ctypes.data and y0.ctypes.data == bufs[1].ctypes.data):
            n1 = xk.shape[0]
            bufs[0][:n1], bufs[1][:n1] = xk, yk
            return bufs[0][:n1], bufs[1][:n1]
        return xk, yk

    def loo_device(self):
        """Leave-one-out posterior of the training rows as device tensors (mu_loo, var_loo), each (N, n_s_out):
        ``sr_gp_loo``.  var_loo includes the noise term (the predictive variance of the observation).  Asynchronous."""
        self._need_trained()
        hd = self._handle
        mu, var = B.empty((hd.n_out, hd.N), hd.device), B.empty((hd.n_out, hd.N), hd.device)
        check(lib.sr_gp_loo(hd.h, B.ptr(mu), B.ptr(var), B.stream_ptr(hd.device)))
        return mu.T, var.T

    def loo(self):
        """``loo_device`` as NumPy arrays (mu_loo, var_loo), each (N, n_s_out)."""
        mu, var = self.loo_device()
        return np.ascontiguousarray(B.to_numpy(mu)), np.ascontiguousarray(B.to_numpy(var))

    def _most_redundant(self):
        """first argmin over j of sum_d alpha_dj^2 var_loo[d, j]: the squared change of the posterior mean at x_j, in units
        of the prior, that retiring row j causes (Csato & Opper's score), summed over the outputs"""
        _, var = self.loo()
        return int(np.argmin((self.beta ** 2 * var).sum(axis=1)))

    def _grown(self, x0, xs, y0, ys):
        """[x0; xs], [y0; ys] as views of buffers with room to grow (a vstack per appended point copies the whole
        training set: 15 us at N = 50, more with N)."""
        n0, n1 = x0.shape[0], x0.shape[0] + xs.shape[0]
        bufs = getattr(self, "_train_bufs", None)
        if (bufs is None or bufs[0].shape[0] < n1 or bufs[0].shape[1:] != x0.shape[1:] or bufs[1].shape[1:] != y0.shape[1:]
                or x0.base is not bufs[0] or y0.base is not bufs[1]
                or x0.ctypes.data != bufs[0].ctypes.data or y0.ctypes.data != bufs[1].ctypes.data):
            cap = max(64, 2 * n1)
            bufs = (np.empty((cap,) + x0.shape[1:]), np.empty((cap,) + y0.shape[1:]))
            bufs[0][:n0], bufs[1][:n0] = x0, y0
            self._train_bufs = bufs
        bufs[0][n0:n1], bufs[1][n0:n1] = xs, ys
        return bufs[0][:n1], bufs[1][:n1]

    def _fit(self, Z, Y, noise_diag):
        dev = B.resolve_device(self._device_arg)
        N, D = Z.shape
        old = self._handle
        if (old is not None and not old.shared and (old.N, old.D, old.n_out) == (N, D, self.n_s_out)
                and old.device == dev):
            handle = old                 # same shape: refactorise in place, no device allocation
        else:
            handle = _Handle(dev, N, D, self.n_s_out)
        # diagonal term: sigma_n^2 + noise_diag (gaussian_process.py:252-253) + GPy's internal jitter
        noise = self._noise + float(noise_diag) + GPY_JITTER
        s = B.stream_ptr(dev)
        self._set_data(handle, Z, Y, noise, dev, s)
        if getattr(self, "_fact_panel", None) is not None:
            check(lib.sr_gp_set_fact_panel(handle.h, self._fact_panel))
        if getattr(self, "_fact_pipeline", None) is not None:
            check(lib.sr_gp_set_fact_pipeline(handle.h, self._fact_pipeline))
        info = (ctypes.c_int * self.n_s_out)()
        check(lib.sr_gp_factorize(handle.h, s, info))
        self._handle = handle
        self._beta = None
        self._inv_K = None
        self._inv_K_dev = None
        if old is not None and old is not handle and getattr(old, "_server_armed", False):
            # a refit with a new size replaced the handle: the server follows -- the model is already in place, so a
            # failure to re-arm leaves the launched routes, not an exception out of the update
            try:
                self.start_server(old._server_idle)
            except RuntimeError as e:
                warnings.warn("resident server not re-armed after the model update: {}".format(e))

    def _set_data(self, handle, Z, Y, noise, dev, s):
        rbf = all(kt == "rbf" for kt in self.kern_types)         # ARD-RBF fast path (north_star kernel)
        if rbf:
            params = [np.stack([h["lengthscale"] for h in self.hyp]), np.array([h["variance"] for h in self.hyp])]
        else:
            params = [self._pack_kernel_params()]
        arrays = [np.ascontiguousarray(a, dtype=np.float64) for a in [Z, Y, noise] + params]
        if sum(a.size for a in arrays) <= B.STAGING_MAX_DOUBLES:
            # one pinned block, one asynchronous copy (five pageable copies, each synchronous: 125 us per update -- a sixth
            # of a refit at N = 1000)
            st = getattr(handle, "_staging", None)
            if st is None:
                st = handle._staging = B.Staging(handle.device)
            tens, _ = st.stage(arrays, [])
        else:
            tens = [B.as_dev(a, dev) for a in arrays]
        if rbf:
            tz, ty, tn, tl, tf = tens
            check(lib.sr_gp_set_data(handle.h, B.ptr(tz), B.ptr(ty), B.ptr(tl), B.ptr(tf), B.ptr(tn), s))
        else:
            tz, ty, tn, tk = tens
            check(lib.sr_gp_set_data_general(handle.h, B.ptr(tz), B.ptr(ty), B.ptr(tk), B.ptr(tn), s))

    # ------------------------------------------------------------------ cached posterior state
    def _need_trained(self):
        if not self.gp_trained or self._handle is None:
            raise RuntimeError("SimpleGPModel: call train()/update_model() before predicting")

    @property
    def device(self):
        self._need_trained()
        return self._handle.device

    @property
    def beta(self):
        """(N, n_s_out) = K_y^-1 y  (``woodbury_vector``; gaussian_process.py:264)."""
        if self._handle is None:
            return None
        if self._beta is None:
            hd = self._handle
            t = B.empty((hd.n_out, hd.N), hd.device)
            check(lib.sr_gp_export(hd.h, B.ptr(t), None, B.stream_ptr(hd.device)))
            self._beta = B.to_numpy(t).T.copy()
        return self._beta

    @property
    def inv_K(self):
        """list of (N, N) explicit inverses (``woodbury_inv``; gaussian_process.py:262).  Cold path."""
        if self._handle is None:
            return None
        if self._inv_K is None:
            hd = self._handle
            out = []
            for d in range(hd.n_out):
                t = B.empty((hd.N, hd.N), hd.device)
                check(lib.sr_gp_inv_k(hd.h, d, B.ptr(t), B.stream_ptr(hd.device)))
                out.append(B.to_numpy(t))
            self._inv_K = out
        return self._inv_K

    def inv_K_device(self):
        """(n_out, N, N) device tensor of the matrices ``sr_gp_inv_k`` writes (K_y^-1 per output; P P^T of a sparse model), kept
        until the next model update: what ``moment_match_device`` contracts the double sum against."""
        self._need_trained()
        if self._inv_K_dev is None:
            hd = self._handle
            t = B.empty((hd.n_out, hd.N, hd.N), hd.device)
            for d in range(hd.n_out):
                check(lib.sr_gp_inv_k(hd.h, d, B.ptr(t[d]), B.stream_ptr(hd.device)))
            self._inv_K_dev = t
        return self._inv_K_dev

    def _mm_inputs(self, m, S, reverse=False):
        self._need_trained()
        if any(kt not in ("rbf", "lin_rbf") for kt in self.kern_types):
            raise NotImplementedError("moment matching: the closed form is for ARD-RBF and lin_rbf models only "
                                      "(a Matern kernel has none)")
        if reverse and any(kt != "rbf" for kt in self.kern_types):
            raise NotImplementedError("moment matching: the reverse pass is for ARD-RBF models only")
        hd = self._handle
        tm = B.as_dev(m, hd.device)
        if tm.dim() != 2 or tm.shape[1] != hd.D:
            raise ValueError("m must be (T, {})".format(hd.D))
        T = tm.shape[0]
        tS = B.as_dev(S, hd.device, (T, hd.D, hd.D)) if S is not None else None
        return hd, tm, tS, T

    def moment_match_device(self, m, S=None, differentiable=False):
        """Exact moment matching on device tensors (``sr_gp_moment_match``): the GP at T Gaussian inputs z ~ N(m[t], S[t]).
        m (T, D); S (T, D, D) symmetric PSD (may be singular) or None = point inputs.
        Returns mu (T, n), cov (T, n, n) -- the full covariance across outputs -- and V (T, n, D) with cov(z, g_a) = S V_a
        (V -> the mean Jacobian as S -> 0).  Models whose kernels are all "rbf" or "lin_rbf" (NotImplementedError for a Matern
        kernel, which has no closed form); a model with a "lin_rbf" output goes through the general-family route.  Asynchronous.
        ``differentiable=True``: the same three tensors (the same bits), hanging on a ``torch.autograd.Function`` whose
        backward is ``moment_match_vjp_device`` (once differentiable; gradients in m and S, not in the model).  ARD-RBF
        models only: the reverse pass of the general family is not provided (NotImplementedError before any launch)."""
        if differentiable:
            if any(kt != "rbf" for kt in self.kern_types):
                raise NotImplementedError("moment matching: the reverse pass is for ARD-RBF models only")
            return _MomentMatchFn.apply(self, m, S)
        hd, tm, tS, T = self._mm_inputs(m, S)
        kinv = self.inv_K_device()
        mu, cov = B.empty((T, hd.n_out), hd.device), B.empty((T, hd.n_out, hd.n_out), hd.device)
        V = B.empty((T, hd.n_out, hd.D), hd.device)
        check(lib.sr_gp_moment_match(hd.h, B.ptr(tm), B.ptr(tS), T, B.ptr(kinv), B.ptr(mu), B.ptr(cov), B.ptr(V),
                                     B.stream_ptr(hd.device)))
        return mu, cov, V

    MM_ROLLOUT_MAX_N = 1024          # sr_gp_moment_match_rollout refuses larger models (and D > 12)

    def moment_match_rollout_supported(self):
        """Whether ``moment_match_rollout_device`` takes this (trained) model: ARD-RBF kernels on every output, exact or
        sparse, N <= 1024 rows (inducing rows of a sparse model), D <= 12."""
        self._need_trained()
        hd = self._handle
        return all(kt == "rbf" for kt in self.kern_types) and hd.N <= self.MM_ROLLOUT_MAX_N and hd.D <= 12

    def moment_match_rollout_device(self, mu0, k_ff, k_fb, a, b, sigma0=None, a_gp_inp_x=None, with_cov=True):
        """T trajectories through H closed-loop steps of exact moment matching in ONE launch (``sr_gp_moment_match_rollout``):
        what ``uncertainty_propagation_casadi.moment_matching_batch`` computes in H rounds, to rounding.  Device tensors in and
        out.  mu0 (T, n_s); sigma0 (T, n_s, n_s) or None (points); k_ff (H, n_u) and k_fb (H-1, n_u, n_s) -- one policy for all
        trajectories -- or (T, H, n_u) and (T, H-1, n_u, n_s), one per trajectory (k_fb may be None when H == 1; step 0 has no
        feedback, step i >= 1 uses k_fb[i-1]); a (n_s, n_s), b (n_s, n_u); a_gp_inp_x (n_x_in, n_s) or None (the GP sees the
        whole state).  Returns mu_all (T, H, n_s), sigma_all (T, H, n_s, n_s) and, with_cov, the GP's output covariance per
        step (T, H, n_s, n_s), else None.  The same bits on every call, with and without with_cov.  ARD-RBF models with
        N <= 1024 and D <= 12 only: NotImplementedError otherwise, before anything is prepared on the device (the per-step
        route, ``moment_matching_batch``, takes those).  Asynchronous."""
        if not self.moment_match_rollout_supported():
            raise NotImplementedError("moment_match_rollout_device: ARD-RBF models with N <= {} and D <= 12 only; "
                                      "use the per-step route (moment_matching_batch)".format(self.MM_ROLLOUT_MAX_N))
        hd = self._handle
        n_s, dev = hd.n_out, hd.device
        tz = None if a_gp_inp_x is None else B.as_dev(a_gp_inp_x, dev)
        if tz is not None and (tz.dim() != 2 or tz.shape[1] != n_s or not 1 <= tz.shape[0] <= hd.D - 1):
            raise ValueError("a_gp_inp_x must be (n_x_in, {}) with 1 <= n_x_in <= {}".format(n_s, hd.D - 1))
        n_x_in = n_s if tz is None else tz.shape[0]
        n_u = hd.D - n_x_in
        if n_u < 1:
            raise ValueError("the closed loop needs D = n_x_in + n_u with n_u >= 1")
        mu = B.as_dev(mu0, dev)
        if mu.dim() != 2 or mu.shape[1] != n_s:
            raise ValueError("mu0 must be (T, {})".format(n_s))
        T = mu.shape[0]
        kff = B.as_dev(k_ff, dev)
        if kff.dim() not in (2, 3) or kff.shape[-1] != n_u or (kff.dim() == 3 and kff.shape[0] != T):
            raise ValueError("k_ff must be (H, {0}) or (T, H, {0})".format(n_u))
        per_traj = int(kff.dim() == 3)
        H = kff.shape[-2]
        if H < 1:
            raise ValueError("k_ff needs H >= 1 steps")
        kfb = None
        if H > 1:
            kfb = B.as_dev(k_fb, dev, ((T,) if per_traj else ()) + (H - 1, n_u, n_s))
        sig = B.as_dev(sigma0, dev, (T, n_s, n_s)) if sigma0 is not None else None
        ta, tb = B.as_dev(a, dev, (n_s, n_s)), B.as_dev(b, dev, (n_s, n_u))
        kinv = self.inv_K_device()
        mu_all, sigma_all = B.empty((T, H, n_s), dev), B.empty((T, H, n_s, n_s), dev)
        cov_all = B.empty((T, H, n_s, n_s), dev) if with_cov else None
        check(lib.sr_gp_moment_match_rollout(hd.h, T, H, n_x_in, per_traj, B.ptr(mu), B.ptr(sig), B.ptr(kff), B.ptr(kfb),
                                             B.ptr(ta), B.ptr(tb), B.ptr(tz), B.ptr(kinv), B.ptr(mu_all), B.ptr(sigma_all),
                                             B.ptr(cov_all), B.stream_ptr(dev)))
        return mu_all, sigma_all, cov_all

    def moment_match_rollout_vjp_device(self, mu0, k_ff, k_fb, a, b, mu_all, sigma_all, mu_all_bar=None, sigma_all_bar=None,
                                        cov_all_bar=None, sigma0=None, a_gp_inp_x=None):
        """Reverse pass of the moment-matching roll-out in one call (``sr_gp_moment_match_rollout_vjp``): the gradient of
        sum(mu_all_bar * mu_all) + sum(sigma_all_bar * sigma_all) + sum(cov_all_bar * cov_all) in mu0, sigma0, k_ff and k_fb.
        The forward arguments are those of ``moment_match_rollout_device``; mu_all (T, H, n_s) and sigma_all (T, H, n_s, n_s) are
        what a forward returned (the fused call or ``moment_matching_batch``); the seeds are shaped like the three forward
        outputs, None = zero, not all three.  Returns (mu0_bar (T, n_s), sigma0_bar (T, n_s, n_s) exactly symmetric | None
        without sigma0, kff_bar, kfb_bar | None when H == 1), the gain gradients shaped like k_ff and k_fb: per trajectory, or
        summed over T for a shared policy (2-D k_ff).  The domain of ``moment_match_vjp_device``: ARD-RBF models, exact or
        sparse, of ANY size (not only those of the fused forward), D <= 12, n_s <= 12; NotImplementedError for any other kernel
        before anything is prepared on the device.  The same bits on every call and for any chunk size.  Asynchronous."""
        self._need_trained()
        if any(kt != "rbf" for kt in self.kern_types):
            raise NotImplementedError("moment matching: the reverse pass is for ARD-RBF models only")
        hd = self._handle
        n_s, dev = hd.n_out, hd.device
        tz = None if a_gp_inp_x is None else B.as_dev(a_gp_inp_x, dev)
        if tz is not None and (tz.dim() != 2 or tz.shape[1] != n_s or not 1 <= tz.shape[0] <= hd.D - 1):
            raise ValueError("a_gp_inp_x must be (n_x_in, {}) with 1 <= n_x_in <= {}".format(n_s, hd.D - 1))
        n_x_in = n_s if tz is None else tz.shape[0]
        n_u = hd.D - n_x_in
        if n_u < 1:
            raise ValueError("the closed loop needs D = n_x_in + n_u with n_u >= 1")
        mu = B.as_dev(mu0, dev)
        if mu.dim() != 2 or mu.shape[1] != n_s:
            raise ValueError("mu0 must be (T, {})".format(n_s))
        T = mu.shape[0]
        kff = B.as_dev(k_ff, dev)
        if kff.dim() not in (2, 3) or kff.shape[-1] != n_u or (kff.dim() == 3 and kff.shape[0] != T):
            raise ValueError("k_ff must be (H, {0}) or (T, H, {0})".format(n_u))
        per_traj = int(kff.dim() == 3)
        H = kff.shape[-2]
        if H < 1:
            raise ValueError("k_ff needs H >= 1 steps")
        kfb = B.as_dev(k_fb, dev, ((T,) if per_traj else ()) + (H - 1, n_u, n_s)) if H > 1 else None
        sig = B.as_dev(sigma0, dev, (T, n_s, n_s)) if sigma0 is not None else None
        ta, tb = B.as_dev(a, dev, (n_s, n_s)), B.as_dev(b, dev, (n_s, n_u))
        tmu, tsig = B.as_dev(mu_all, dev, (T, H, n_s)), B.as_dev(sigma_all, dev, (T, H, n_s, n_s))
        seeds = [None if x is None else B.as_dev(x, dev, shp)
                 for x, shp in ((mu_all_bar, (T, H, n_s)), (sigma_all_bar, (T, H, n_s, n_s)), (cov_all_bar, (T, H, n_s, n_s)))]
        if all(x is None for x in seeds):
            raise ValueError("at least one of mu_all_bar, sigma_all_bar, cov_all_bar is required")
        kinv = self.inv_K_device()
        mu0_bar = B.empty((T, n_s), dev)
        sigma0_bar = B.empty((T, n_s, n_s), dev) if sig is not None else None
        kff_bar = B.empty((T, H, n_u), dev)
        kfb_bar = B.empty((T, H - 1, n_u, n_s), dev) if H > 1 else None
        check(lib.sr_gp_moment_match_rollout_vjp(hd.h, T, H, n_x_in, per_traj, B.ptr(mu), B.ptr(sig), B.ptr(kff), B.ptr(kfb),
                                                 B.ptr(ta), B.ptr(tb), B.ptr(tz), B.ptr(kinv), B.ptr(tmu), B.ptr(tsig),
                                                 B.ptr(seeds[0]), B.ptr(seeds[1]), B.ptr(seeds[2]), B.ptr(mu0_bar),
                                                 B.ptr(sigma0_bar), B.ptr(kff_bar), B.ptr(kfb_bar), B.stream_ptr(dev)))
        if not per_traj:                               # one policy for all: its gradient is the sum over the trajectories
            kff_bar = kff_bar.sum(dim=0)
            kfb_bar = None if kfb_bar is None else kfb_bar.sum(dim=0)
        return mu0_bar, sigma0_bar, kff_bar, kfb_bar

    def moment_match_vjp_device(self, m, S, mu_bar=None, cov_bar=None, V_bar=None):
        """Reverse pass of ``moment_match_device`` (``sr_gp_moment_match_vjp``): for seeds mu_bar (T, n), cov_bar (T, n, n),
        V_bar (T, n, D) (None = zero) the derivatives m_bar (T, D) and S_bar (T, D, D) of
        sum(mu_bar * mu) + sum(cov_bar * cov) + sum(V_bar * V) in m and S (S None = zero; S_bar is returned all the same: it is
        not zero there).  S_bar is exactly symmetric; the clip of the covariance diagonal is ignored.  Asynchronous."""
        hd, tm, tS, T = self._mm_inputs(m, S, reverse=True)
        n, D = hd.n_out, hd.D
        seeds = [None if x is None else B.as_dev(x, hd.device, shp)
                 for x, shp in ((mu_bar, (T, n)), (cov_bar, (T, n, n)), (V_bar, (T, n, D)))]
        kinv = self.inv_K_device()
        m_bar, S_bar = B.empty((T, D), hd.device), B.empty((T, D, D), hd.device)
        check(lib.sr_gp_moment_match_vjp(hd.h, B.ptr(tm), B.ptr(tS), T, B.ptr(kinv), B.ptr(seeds[0]), B.ptr(seeds[1]),
                                         B.ptr(seeds[2]), B.ptr(m_bar), B.ptr(S_bar), B.stream_ptr(hd.device)))
        return m_bar, S_bar

    def predict_uncertain_vjp(self, mean, cov=None, mu_bar=None, cov_bar=None, V_bar=None):
        """NumPy form of ``moment_match_vjp_device``: mean (T, D) or (D,), cov (T, D, D) or (D, D) or None, seeds shaped
        as the outputs of ``predict_uncertain`` -> m_bar (T, D), S_bar (T, D, D)."""
        mean = np.atleast_2d(np.asarray(mean, dtype=np.float64))
        if cov is not None:
            cov = np.asarray(cov, dtype=np.float64).reshape(mean.shape[0], mean.shape[1], mean.shape[1])
        return tuple(B.to_numpy(o) for o in self.moment_match_vjp_device(mean, cov, mu_bar, cov_bar, V_bar))

    def predict_uncertain(self, mean, cov=None):
        """NumPy form of ``moment_match_device``: mean (T, D) or (D,), cov (T, D, D) or (D, D) or None
        -> mu (T, n), Cov (T, n, n), V (T, n, D)."""
        mean = np.atleast_2d(np.asarray(mean, dtype=np.float64))
        if cov is not None:
            cov = np.asarray(cov, dtype=np.float64).reshape(mean.shape[0], mean.shape[1], mean.shape[1])
        return tuple(B.to_numpy(o) for o in self.moment_match_device(mean, cov))

    def export_state(self):
        """(alpha (n_out,N), Wt (n_out,Np,Np)) device tensors -- what a broadcast receiver imports."""
        self._need_trained()
        hd = self._handle
        alpha = B.empty((hd.n_out, hd.N), hd.device)
        wt = B.empty((hd.n_out, hd.Np, hd.Np), hd.device)
        check(lib.sr_gp_export(hd.h, B.ptr(alpha), B.ptr(wt), B.stream_ptr(hd.device)))
        return alpha, wt

    # ---- packed replication (one-time broadcast to the other GPUs; parallel.replicate_model) ----------------------
    def export_alpha(self):
        """alpha (n_out, N) as a device tensor."""
        self._need_trained()
        hd = self._handle
        alpha = B.empty((hd.n_out, hd.N), hd.device)
        check(lib.sr_gp_export(hd.h, B.ptr(alpha), None, B.stream_ptr(hd.device)))
        return alpha

    def packed_count(self, row0, row1):
        n = lib.sr_gp_packed_count(self._handle.h, int(row0), int(row1))
        if n < 0:
            raise ValueError("rows [%d, %d) outside the model" % (row0, row1))
        return int(n)

    def export_packed(self, d, row0, row1, buf):
        """Rows [row0, row1) of the upper triangle of U^-1 of output d, packed back to back into ``buf`` (device
        tensor with room for ``packed_count(row0, row1)`` doubles), on the current stream."""
        self._need_trained()
        hd = self._handle
        assert buf.is_cuda and buf.dtype == torch.float64 and buf.numel() >= self.packed_count(row0, row1)
        check(lib.sr_gp_export_packed(hd.h, int(d), int(row0), int(row1), B.ptr(buf), B.stream_ptr(hd.device)))

    def begin_import(self, Z, Y, alpha, noise_diag=1e-5):
        """Receiver side of the packed replication: data + alpha now, then ``import_packed`` for every piece of every
        output, then ``end_import``.  No factorisation here."""
        dev = B.resolve_device(self._device_arg)
        Z = np.asarray(Z, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        N, D = Z.shape
        handle = _Handle(dev, N, D, self.n_s_out)
        noise = self._noise + float(noise_diag) + GPY_JITTER
        s = B.stream_ptr(dev)
        self._set_data(handle, Z, Y, noise, dev, s)
        ta = B.as_dev(alpha, dev, (self.n_s_out, N))
        check(lib.sr_gp_import_begin(handle.h, B.ptr(ta), s))
        torch.cuda.current_stream(dev).synchronize()        # ta may go
        self._import = (handle, Z, Y, noise_diag)

    def import_packed(self, d, row0, row1, buf):
        handle = self._import[0]
        check(lib.sr_gp_import_packed(handle.h, int(d), int(row0), int(row1), B.ptr(buf), B.stream_ptr(handle.device)))

    def end_import(self):
        handle, Z, Y, noise_diag = self._import
        check(lib.sr_gp_import_end(handle.h))
        torch.cuda.current_stream(handle.device).synchronize()
        self._import = None
        self._handle = handle
        self._noise_diag = noise_diag
        self._beta = None
        self._inv_K = None
        self._inv_K_dev = None
        self.z = Z
        self.x_train = Z
        self.y_train = Y
        self._z_fit, self._y_z = Z, Y
        self.gp_trained = True

    def import_state(self, Z, Y, alpha, wt, noise_diag=1e-5):
        """Adopt a posterior factorised elsewhere (rank-0 broadcast): no factorisation here."""
        dev = B.resolve_device(self._device_arg)
        Z = np.asarray(Z, dtype=np.float64)
        Y = np.asarray(Y, dtype=np.float64)
        N, D = Z.shape
        handle = _Handle(dev, N, D, self.n_s_out)
        noise = self._noise + float(noise_diag) + GPY_JITTER
        s = B.stream_ptr(dev)
        self._set_data(handle, Z, Y, noise, dev, s)
        ta = B.as_dev(alpha, dev, (self.n_s_out, N))
        tw = B.as_dev(wt, dev, (self.n_s_out, handle.Np, handle.Np))
        check(lib.sr_gp_import(handle.h, B.ptr(ta), B.ptr(tw), s))
        torch.cuda.current_stream(dev).synchronize()
        self._handle = handle
        self._noise_diag = noise_diag
        self._beta = None
        self._inv_K = None
        self._inv_K_dev = None
        self.z = Z
        self.x_train = Z
        self.y_train = Y
        self._z_fit, self._y_z = Z, Y
        self.gp_trained = True

    @property
    def y_z(self):
        """(N, n_s_out) targets of the rows the model is conditioned on (the reference's local ``y_z``,
        gaussian_process.py:207-230; equals ``y_train`` unless ``m`` selected a subset)."""
        return self._y_z

    @property
    def z_fit(self):
        """(N, D) inputs the device model is conditioned on (``z`` unless the caller fixed ``Z``)."""
        return self._z_fit

    # ------------------------------------------------------------------ prediction
    def predict_device(self, x_new, compute_gradients=False):
        """Batched posterior on device tensors: x_new (T, D) -> mu (T,n), var (T,n)[, jac (T,n,D)]."""
        self._need_trained()
        hd = self._handle
        x = B.as_dev(x_new, hd.device)
        if x.dim() != 2 or x.shape[1] != hd.D:
            raise ValueError("x_new must be (T, {})".format(hd.D))
        T = x.shape[0]
        mu = B.empty((T, hd.n_out), hd.device)
        var = B.empty((T, hd.n_out), hd.device)
        jac = B.empty((T, hd.n_out, hd.D), hd.device) if compute_gradients else None
        check(lib.sr_gp_predict(hd.h, B.ptr(x), T, B.ptr(mu), B.ptr(var), B.ptr(jac),
                                B.stream_ptr(hd.device)))
        return (mu, var, jac) if compute_gradients else (mu, var)

    def _predict_host(self, x_new, compute_gradients=False):
        """predict for a NumPy batch: the queries through one pinned block, (mu, var[, jac]) back through one
        (B.Staging) -- one H2D copy, one D2H copy, one synchronisation instead of one per array."""
        self._need_trained()
        hd = self._handle
        x = np.ascontiguousarray(np.asarray(x_new, dtype=np.float64))
        if x.ndim != 2 or x.shape[1] != hd.D:
            raise ValueError("x_new must be (T, {})".format(hd.D))
        T = x.shape[0]
        if T == 0 or T * hd.n_out * (2 + hd.D) > B.STAGING_MAX_DOUBLES:
            return tuple(B.to_numpy(o) for o in self.predict_device(x, compute_gradients))
        if T == 1:
            # one query (what the exploration loop asks after every step, exploration_runner.py:179): the one-command
            # route of __call__ where the model has a one-launch posterior -- query in the kernel arguments, results
            # written to the pinned block by the kernel, no copies: 35 -> 27 us
            # (not at 384 padded rows, where the streamed kernel serves one query faster than the one-launch pass, and
            #  not where the library has already declined the route for this padded size)
            n, D = hd.n_out, hd.D
            io = hd.single_io()
            if getattr(hd, "_server_armed", False):
                io["h_in_np"][:D] = x[0]
                o = hd.server_call(0, 2 * n + n * D)
                if o is not None:
                    out = (o[None, :n], o[None, n:2 * n])
                    return out + (o[2 * n:].reshape(1, n, D),) if compute_gradients else out
            if hd.Np != 384 and io["mailbox"] and (io["direct"] or io.get("direct_off_np") != hd.Np):
                io["h_in_np"][:D] = x[0]
                o = hd.call1(0, 2 * n + n * D, B.current_stream(hd.device))
                if o is not None:
                    out = (o[None, :n], o[None, n:2 * n])
                    return out + (o[2 * n:].reshape(1, n, D),) if compute_gradients else out
        st = getattr(hd, "_staging", None)
        if st is None:
            st = hd._staging = B.Staging(hd.device)
        shapes = [(T, hd.n_out), (T, hd.n_out)] + ([(T, hd.n_out, hd.D)] if compute_gradients else [])
        (dx,), outs = st.stage([x], shapes, zero_copy=True)
        check(lib.sr_gp_predict(hd.h, B.ptr(dx), T, B.ptr(outs[0]), B.ptr(outs[1]),
                                B.ptr(outs[2]) if compute_gradients else None, B.stream_ptr(hd.device)))
        return tuple(st.fetch())

    def predict(self, *args, **kwargs):
        """Predictive mean and variance for a set of test inputs.

        Accepts both historical call shapes of the reference:
          * ``predict(x_new (T,D), quantiles=None, compute_gradients=False)``
            -> (T,n_s), (T,n_s)[, (T,n_s,D)]                   gaussian_process.py:546-568
          * ``predict(states (N,n), actions (N,m), jacobians=False, full_cov=False)``
            -> mean (N,n), var (N,n)[, jac_mean (N,n,n+m), jac_var (N,n,n+m)]   state_space_models.py:74-104
        """
        two = (len(args) >= 2 and hasattr(args[1], "shape") and np.ndim(args[1]) == 2) or "actions" in kwargs
        if two:
            states = args[0] if args else kwargs.pop("states")
            actions = args[1] if len(args) > 1 else kwargs.pop("actions")
            jacobians = args[2] if len(args) > 2 else kwargs.pop("jacobians", False)
            full_cov = args[3] if len(args) > 3 else kwargs.pop("full_cov", False)
            if full_cov:
                raise NotImplementedError("full covariance is not supported")
            if jacobians:
                return self.predict_with_jacobians(states, actions)
            as_t = B.is_tensor(states)
            if as_t:
                x_new = torch.cat((states, actions), dim=1)
            else:
                x_new = np.hstack((np.asarray(states, dtype=np.float64),
                                   np.asarray(actions, dtype=np.float64)))
            if not as_t:
                return self._predict_host(x_new, bool(jacobians))
            return self.predict_device(x_new, bool(jacobians))
        x_new = args[0] if args else kwargs.pop("x_new")
        quantiles = args[1] if len(args) > 1 else kwargs.pop("quantiles", None)
        compute_gradients = args[2] if len(args) > 2 else kwargs.pop("compute_gradients", False)
        if quantiles is not None:
            raise NotImplementedError()
        if not B.is_tensor(x_new):
            return self._predict_host(x_new, bool(compute_gradients))
        return self.predict_device(x_new, bool(compute_gradients))

    def predictive_gradients(self, x_new, grad_sigma=False):
        """(T, n_s, D) gradients of the predictive mean (gaussian_process.py:570-596).  With ``grad_sigma=True``
        (the reference raises there; GPy returns it) the pair (grad_mu, grad_var), each (T, n_s, D), through the
        batched gradient pass.  NumPy or tensors like the input."""
        if grad_sigma:
            if B.is_tensor(x_new):
                return self.predict_device_grad(x_new)[2:]
            return self._predict_grad_host(x_new)[2:]
        out = self.predict_device(x_new, True)[2]
        return out if B.is_tensor(x_new) else B.to_numpy(out)

    def predict_device_grad(self, x_new):
        """Batched posterior with both gradients on device tensors, no host synchronisation (sr_gp_predict_grad):
        x_new (T, D) -> mu (T,n), var (T,n), jac_mu (T,n,D), jac_var (T,n,D) = d var / dx."""
        self._need_trained()
        hd = self._handle
        x = B.as_dev(x_new, hd.device)
        if x.dim() != 2 or x.shape[1] != hd.D:
            raise ValueError("x_new must be (T, {})".format(hd.D))
        T = x.shape[0]
        mu, var = B.empty((T, hd.n_out), hd.device), B.empty((T, hd.n_out), hd.device)
        jm, jv = B.empty((T, hd.n_out, hd.D), hd.device), B.empty((T, hd.n_out, hd.D), hd.device)
        check(lib.sr_gp_predict_grad(hd.h, B.ptr(x), T, B.ptr(mu), B.ptr(var), B.ptr(jm), B.ptr(jv),
                                     B.stream_ptr(hd.device)))
        return mu, var, jm, jv

    def _predict_grad_host(self, x_new):
        """predict_device_grad for a NumPy batch through one staging round trip (as _predict_host)."""
        self._need_trained()
        hd = self._handle
        x = np.ascontiguousarray(np.asarray(x_new, dtype=np.float64))
        if x.ndim != 2 or x.shape[1] != hd.D:
            raise ValueError("x_new must be (T, {})".format(hd.D))
        T = x.shape[0]
        if T == 0 or T * hd.n_out * (2 + 2 * hd.D) > B.STAGING_MAX_DOUBLES:
            return tuple(B.to_numpy(o) for o in self.predict_device_grad(x))
        st = getattr(hd, "_staging", None)
        if st is None:
            st = hd._staging = B.Staging(hd.device)
        shapes = [(T, hd.n_out), (T, hd.n_out), (T, hd.n_out, hd.D), (T, hd.n_out, hd.D)]
        (dx,), outs = st.stage([x], shapes, zero_copy=True)
        check(lib.sr_gp_predict_grad(hd.h, B.ptr(dx), T, B.ptr(outs[0]), B.ptr(outs[1]), B.ptr(outs[2]),
                                     B.ptr(outs[3]), B.stream_ptr(hd.device)))
        return tuple(st.fetch())

    def __call__(self, states, actions):
        """Single-query evaluation used by onestep_reachability (gaussian_process.py:135-144):
        returns exactly (mu (n,1), sigma (n,1), jac (n,D))."""
        states = np.asarray(states, dtype=np.float64)
        actions = np.asarray(actions, dtype=np.float64)
        N, _ = np.shape(states)
        if N > 1:
            raise NotImplementedError("Currently do not support multiple state-action pairs to "
                                      "evaluate on.")
        self._need_trained()
        hd = self._handle
        n, D = hd.n_out, hd.D
        if states.shape[1] + actions.shape[1] != D:
            raise ValueError("states and actions must have {} columns together".format(D))
        io = hd.single_io()
        io["h_in_np"][:states.shape[1]] = states[0]
        io["h_in_np"][states.shape[1]:] = actions[0]
        o = hd.server_call(0, 2 * n + n * D)          # the resident server, where one is armed: no launch, no stream
        if o is not None:
            return o[:n, None], o[n:2 * n, None], o[2 * n:].reshape(n, D)
        stream = B.current_stream(hd.device)
        o = hd.call1(0, 2 * n + n * D, stream)
        if o is not None:
            return o[:n, None], o[n:2 * n, None], o[2 * n:].reshape(n, D)
        io["d_in"].copy_(io["h_in"].view(1, D), non_blocking=True)
        check(lib.sr_gp_predict(hd.h, B.ptr(io["d_in"]), 1, B.ptr(io["mu"]), B.ptr(io["var"]), B.ptr(io["jm"]),
                                ctypes.c_void_p(stream.cuda_stream)))
        o = hd.fetch(2 * n + n * D, stream)
        return o[:n, None], o[n:2 * n, None], o[2 * n:].reshape(n, D)

    def linearize_device(self, x):
        """Single query x (D,) -> device tensors (mu (n,), var (n,), jac_mu (n,D), jac_var (n,D),
        hess_mu (n,D,D)) through sr_gp_linearize."""
        self._need_trained()
        hd = self._handle
        tx = B.as_dev(x, hd.device).reshape(-1)
        if tx.numel() != hd.D:
            raise ValueError("x must have {} entries".format(hd.D))
        mu, var = B.empty((hd.n_out,), hd.device), B.empty((hd.n_out,), hd.device)
        jm, jv = B.empty((hd.n_out, hd.D), hd.device), B.empty((hd.n_out, hd.D), hd.device)
        hm = B.empty((hd.n_out, hd.D, hd.D), hd.device)
        check(lib.sr_gp_linearize(hd.h, B.ptr(tx), B.ptr(mu), B.ptr(var), B.ptr(jm), B.ptr(jv), B.ptr(hm),
                                  B.stream_ptr(hd.device)))
        return mu, var, jm, jv, hm

    def linearize_predict(self, states, actions, jacobians=False, full_cov=False):
        """Contract of state_space_models.py:106-138 for a single query (what CasadiSSMEvaluator calls,
        :297-303 and :402-415):
          jacobians=False -> (mu (n,1), var (n,1), jac_mu (n,D))
          jacobians=True  -> (mu (n,1), var (n,1), jac_mu (n,D), jac_var (n,D), hess_mu (n,D,D))
        The outputs are cached for ``get_linearize_reverse``."""
        if full_cov:
            raise NotImplementedError("full covariance is not supported")
        states = np.asarray(states, dtype=np.float64)
        actions = np.asarray(actions, dtype=np.float64)
        N, _ = np.shape(states)
        if not jacobians:
            return self.__call__(states, actions)
        if N > 1:
            raise NotImplementedError("'linearize_predict' currently only allows for single inputs, "
                                      "i.e. (1 x n) arrays, when computing jacobians.")
        mu, var, jm, jv, hm = self._linearize_host(np.hstack((states, actions))[0])
        self._linearize_forward_cache = (jm, jv, hm)
        return mu[:, None], var[:, None], jm, jv, hm

    def _linearize_host(self, x):
        """sr_gp_linearize through the pinned single-query staging: host x (D,) -> host arrays."""
        self._need_trained()
        hd = self._handle
        n, D = hd.n_out, hd.D
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if x.size != D:
            raise ValueError("x must have {} entries".format(D))
        io = hd.single_io()
        a, b, c = 2 * n, 2 * n + n * D, 2 * n + 2 * n * D
        io["h_in_np"][:] = x
        o = hd.server_call(1, c + n * D * D)
        if o is not None:
            return o[:n], o[n:a], o[a:b].reshape(n, D), o[b:c].reshape(n, D), o[c:].reshape(n, D, D)
        stream = B.current_stream(hd.device)
        o = hd.call1(1, io["d_out"].numel(), stream)
        if o is not None:
            return o[:n], o[n:a], o[a:b].reshape(n, D), o[b:c].reshape(n, D), o[c:].reshape(n, D, D)
        io["d_in"].copy_(io["h_in"].view(1, D), non_blocking=True)
        check(lib.sr_gp_linearize(hd.h, B.ptr(io["d_in"]), B.ptr(io["mu"]), B.ptr(io["var"]), B.ptr(io["jm"]),
                                  B.ptr(io["jv"]), B.ptr(io["hm"]), ctypes.c_void_p(stream.cuda_stream)))
        o = hd.fetch(io["d_out"].numel(), stream)
        return o[:n], o[n:a], o[a:b].reshape(n, D), o[b:c].reshape(n, D), o[c:].reshape(n, D, D)

    def linearize_device_batch(self, x_new):
        """Second-order outputs for a batch on device tensors, no host synchronisation (sr_gp_linearize_batch):
        x_new (T, D) -> mu (T,n), var (T,n), jac_mu (T,n,D), jac_var (T,n,D), hess_mu (T,n,D,D).  The first four are
        those of predict_device_grad to the bit; hess_mu is exactly symmetric."""
        self._need_trained()
        hd = self._handle
        x = B.as_dev(x_new, hd.device)
        if x.dim() != 2 or x.shape[1] != hd.D:
            raise ValueError("x_new must be (T, {})".format(hd.D))
        T, n, D = x.shape[0], hd.n_out, hd.D
        mu, var = B.empty((T, n), hd.device), B.empty((T, n), hd.device)
        jm, jv = B.empty((T, n, D), hd.device), B.empty((T, n, D), hd.device)
        hm = B.empty((T, n, D, D), hd.device)
        check(lib.sr_gp_linearize_batch(hd.h, B.ptr(x), T, B.ptr(mu), B.ptr(var), B.ptr(jm), B.ptr(jv), B.ptr(hm),
                                        B.stream_ptr(hd.device)))
        return mu, var, jm, jv, hm

    def _linearize_batch_host(self, x):
        """linearize_device_batch for a NumPy batch through one staging round trip (as _predict_grad_host)."""
        hd = self._handle
        T, n, D = x.shape[0], hd.n_out, hd.D
        if T == 0 or T * n * (2 + 2 * D + D * D) > B.STAGING_MAX_DOUBLES:
            return tuple(B.to_numpy(o) for o in self.linearize_device_batch(x))
        st = getattr(hd, "_staging", None)
        if st is None:
            st = hd._staging = B.Staging(hd.device)
        shapes = [(T, n), (T, n), (T, n, D), (T, n, D), (T, n, D, D)]
        (dx,), outs = st.stage([x], shapes, zero_copy=True)
        check(lib.sr_gp_linearize_batch(hd.h, B.ptr(dx), T, B.ptr(outs[0]), B.ptr(outs[1]), B.ptr(outs[2]),
                                        B.ptr(outs[3]), B.ptr(outs[4]), B.stream_ptr(hd.device)))
        return tuple(st.fetch())

    def linearize_predict_batch(self, states, actions):
        """``linearize_predict(..., jacobians=True)`` for a batch of T rows (states (T,n_s), actions (T,n_u)):
        (mu (T,n), var (T,n), jac_mu (T,n,D), jac_var (T,n,D), hess_mu (T,n,D,D)), NumPy or tensors like the input.
        Every batch but a single row takes one batched pass (sr_gp_linearize_batch, D <= GRAD_MAX_D); one row the
        single-query latency route; wider inputs a loop of single-query rows.  Unlike linearize_predict, nothing is
        cached for ``get_linearize_reverse``."""
        self._need_trained()
        hd = self._handle
        if B.is_tensor(states):
            x = torch.cat((states, actions), dim=1)
            if x.shape[1] != hd.D:
                raise ValueError("states and actions must have {} columns together".format(hd.D))
            if x.shape[0] != 1 and hd.D <= self.GRAD_MAX_D:
                return self.linearize_device_batch(x)
            if x.shape[0] == 1:
                return tuple(o.unsqueeze(0) for o in self.linearize_device(x[0]))
            return tuple(B.as_dev(o, hd.device) for o in self._linearize_rows(x.detach().cpu().numpy()))
        x = np.ascontiguousarray(np.hstack((np.asarray(states, dtype=np.float64), np.asarray(actions, dtype=np.float64))))
        if x.ndim != 2 or x.shape[1] != hd.D:
            raise ValueError("states and actions must have {} columns together".format(hd.D))
        if x.shape[0] != 1 and hd.D <= self.GRAD_MAX_D:
            return self._linearize_batch_host(x)
        return self._linearize_rows(x)

    def _linearize_rows(self, x):
        """one single-query linearisation (_linearize_host) per row of a host batch x (T, D)"""
        hd = self._handle
        T, n, D = x.shape[0], hd.n_out, hd.D
        out = (np.empty((T, n)), np.empty((T, n)), np.empty((T, n, D)), np.empty((T, n, D)), np.empty((T, n, D, D)))
        for t in range(T):
            for o, r in zip(out, self._linearize_host(x[t])):
                o[t] = r
        return out

    # from this many queries on predict(states, actions, jacobians=True) takes the batched gradient pass instead of the
    # single-query linearisation per row (inputs of up to GRAD_MAX_D dimensions: the pass's compiled range)
    GRAD_BATCH_MIN = 2
    GRAD_MAX_D = 8

    def predict_with_jacobians(self, states, actions):
        """Base-class ``predict(states, actions, jacobians=True)`` (state_space_models.py:74-104):
        (mean (N,n), var (N,n), jac_mean (N,n,D), jac_var (N,n,D)).  One query: the single-query latency path
        (cached for ``get_reverse``); a batch: one batched gradient pass (sr_gp_predict_grad).  Torch device tensors
        in give device tensors out."""
        batched = self._handle is not None and self._handle.D <= self.GRAD_MAX_D
        if B.is_tensor(states):
            x = torch.cat((states, actions), dim=1)
            if batched and x.shape[0] >= self.GRAD_BATCH_MIN:
                return self.predict_device_grad(x)
            x = x.detach().cpu().numpy()
            as_t = True
        else:
            x = np.hstack((np.asarray(states, dtype=np.float64), np.asarray(actions, dtype=np.float64)))
            as_t = False
        N = x.shape[0]
        hd = self._handle
        self._need_trained()
        if batched and N >= self.GRAD_BATCH_MIN:
            return self._predict_grad_host(x)
        mean, var = np.empty((N, hd.n_out)), np.empty((N, hd.n_out))
        jm, jv = np.empty((N, hd.n_out, hd.D)), np.empty((N, hd.n_out, hd.D))
        for t in range(N):
            mean[t], var[t], jm[t], jv[t], _ = self._linearize_host(x[t])
        if N == 1:
            self._forward_cache = (jm[0], jv[0])
        if as_t:
            return tuple(B.as_dev(o, hd.device) for o in (mean, var, jm, jv))
        return mean, var, jm, jv

    def get_reverse(self, seed):
        """v^T J for the stacked outputs [mu; var] of the last single-query
        ``predict(states, actions, jacobians=True)`` (state_space_models.py:168-179);
        returns (grad_state (n,), grad_action (m,))."""
        if self._forward_cache is None:
            raise RuntimeError("get_reverse needs a preceding single-query predict(..., jacobians=True)")
        jm, jv = self._forward_cache
        n = self.n_s_out
        seed = np.asarray(seed, dtype=np.float64).reshape(-1)
        grad = seed[:n].dot(jm) + seed[n:2 * n].dot(jv)
        return grad[:self.n_s_in], grad[self.n_s_in:]

    def get_linearize_reverse(self, seed):
        """v^T J for the stacked outputs [mu; var; vec(jac_mu)] of the last
        ``linearize_predict(..., jacobians=True)`` (state_space_models.py:181-192; seed length
        2n + n(n+m), jac_mu flattened row-major like ssm_pytorch/gaussian_process.py:372);
        returns (grad_state (n,1), grad_action (m,1))."""
        if self._linearize_forward_cache is None:
            raise RuntimeError("get_linearize_reverse needs a preceding linearize_predict(..., jacobians=True)")
        jm, jv, hm = self._linearize_forward_cache
        n, D = jm.shape
        seed = np.asarray(seed, dtype=np.float64).reshape(-1)
        grad = seed[:n].dot(jm) + seed[n:2 * n].dot(jv) + np.einsum('ij,ijk->k', seed[2 * n:].reshape(n, D), hm)
        return grad[:self.n_s_in, None], grad[self.n_s_in:, None]

    def sample_device(self, inp, size=10, eps=None, generator=None, k_fb=None, k_ff=None):
        """Marginal posterior samples on the device: inp (n, D) -> S (n, size, n_s_out) = mu + sqrt(var) eps.
        eps (n, size, n_s_out) standard-normal draws may be supplied (tests, common random numbers);
        otherwise they come from torch's device generator.  With k_fb (n_u, n_s), k_ff (n_u,) the next GP
        inputs [S, k_fb S + k_ff] (n, size, D) are returned as well (sampling_models.py:66-80)."""
        mu, var = self.predict_device(inp)
        hd = self._handle
        n, n_out = mu.shape
        size = int(size)
        if eps is None:
            eps = torch.randn((n, size, n_out), dtype=torch.float64, device=hd.device, generator=generator)
        else:
            eps = B.as_dev(eps, hd.device, (n, size, n_out))
        S = B.empty((n, size, n_out), hd.device)
        z = tk = tf = None
        n_u = 0
        if k_fb is not None:
            n_u = hd.D - n_out
            if n_u < 0:
                raise ValueError("next inputs need D = n_s_out + n_u")
            tk = B.as_dev(k_fb, hd.device, (n_u, n_out))
            tf = B.as_dev(k_ff, hd.device, (n_u,))
            z = B.empty((n, size, hd.D), hd.device)
        check(lib.sr_gp_sample(hd.device.index, n, size, n_out, n_u, B.ptr(mu), B.ptr(var), B.ptr(eps),
                               B.ptr(S), B.ptr(tk), B.ptr(tf), B.ptr(z), B.stream_ptr(hd.device)))
        return S if z is None else (S, z)

    def sample_from_gp(self, inp, size=10, eps=None, generator=None):
        """Sample from the GP predictive (latent, marginal) distribution  gaussian_process.py:598-619.

        inp (n, n_s+n_u) -> S (n, size, n_s_out); S[i, :, d] ~ N(mu_d(x_i), var_d(x_i)) independently per test
        input, as GPy's ``posterior_samples_f(full_cov=False)`` draws them."""
        S = self.sample_device(inp, size, eps, generator)
        return S if B.is_tensor(inp) else B.to_numpy(S)

    # ------------------------------------------------------------------ posterior function samples (pathwise conditioning)
    def draw_paths(self, size, n_features=1024, generator=None, omega=None, tau=None, w=None, eps=None):
        """Draw `size` whole posterior FUNCTIONS (Matheron's rule on n_features random Fourier features of the ARD-RBF
        kernel; include/safereach.h) and keep them with the model until its next update.  The reference has no
        counterpart: sample_from_gp draws marginal samples only.  The draws -- omega (M, D) and w (n_s_out, size, n_w) and
        eps (n_s_out, size, N) standard normal, tau (M,) uniform in [0, 2 pi) -- come from torch's device generator where
        not supplied.  n_w = paths_weight_count(M): M for "rbf" models; a model with a "lin_rbf" output (the general family
        with the RBF radial part) takes G M + D weights per path, G the number of its active groups.  Matern kernels:
        NotImplementedError."""
        self._need_trained()
        hd = self._handle
        S, M = int(size), int(n_features)
        if S < 1 or M < 1:
            raise ValueError("draw_paths: size and n_features must be positive (got {}, {})".format(size, n_features))
        dev, n_out, N = hd.device, hd.n_out, hd.N
        n_w = self.paths_weight_count(M)       # (the model's refusals come from here: before any shape is looked at)

        def draw(given, shape, uniform=False):
            if given is not None:
                return B.as_dev(given, dev, shape)
            if uniform:
                return torch.rand(shape, dtype=torch.float64, device=dev, generator=generator) * (2.0 * np.pi)
            return torch.randn(shape, dtype=torch.float64, device=dev, generator=generator)

        t_om, t_tau = draw(omega, (M, hd.D)), draw(tau, (M,), uniform=True)
        t_w, t_eps = draw(w, (n_out, S, n_w)), draw(eps, (n_out, S, N))
        check(lib.sr_gp_paths_draw(hd.h, S, M, B.ptr(t_om), B.ptr(t_tau), B.ptr(t_w), B.ptr(t_eps), B.stream_ptr(dev)))

    def paths_weight_count(self, n_features=1024):
        """Weights per path and output that draw_paths(.., n_features) takes (sr_gp_paths_weight_count), with the draw's
        refusals: NotImplementedError for a Matern kernel or D > 8, ValueError for a negative kernel parameter."""
        self._need_trained()
        n_w = ctypes.c_int(0)
        check(lib.sr_gp_paths_weight_count(self._handle.h, int(n_features), ctypes.byref(n_w)))
        return n_w.value

    def _paths_fused_rollout_supported(self):
        """the roll-out in one launch and its reverse pass hold the ARD-RBF feature map: "rbf" models only"""
        return all(kt == "rbf" for kt in self.kern_types)

    def drop_paths(self):
        """Give the memory of the drawn paths back."""
        self._need_trained()
        check(lib.sr_gp_paths_draw(self._handle.h, 0, 0, None, None, None, None, B.stream_ptr(self._handle.device)))

    def _need_paths(self):
        S, _ = self.paths_count()
        if S == 0:
            raise RuntimeError("SimpleGPModel: no valid paths (call draw_paths() after the last model update)")
        return S

    def paths_count(self):
        """(size, n_features) of the valid paths; (0, 0) when there are none (never drawn, or the model changed since)."""
        self._need_trained()
        S, M = ctypes.c_int(0), ctypes.c_int(0)
        check(lib.sr_gp_paths_count(self._handle.h, ctypes.byref(S), ctypes.byref(M)))
        return S.value, M.value

    def sample_paths_device(self, x, jacobians=False):
        """Every drawn path at every input: x (n, D) -> (n, size, n_s_out), the shape of sample_from_gp; the values of one
        path at several inputs are those of ONE function.  jacobians=True: (F, J) with J (n, size, n_s_out, D) the
        derivative of every value in its input (closed form over the same draws; F is bit for bit the F without)."""
        self._need_trained()
        hd = self._handle
        x = B.as_dev(x, hd.device)
        if x.dim() != 2 or x.shape[1] != hd.D:
            raise ValueError("x must be (n, {})".format(hd.D))
        S = self._need_paths()
        F = B.empty((x.shape[0], S, hd.n_out), hd.device)
        if jacobians:
            J = B.empty((x.shape[0], S, hd.n_out, hd.D), hd.device)
            check(lib.sr_gp_paths_eval_grad(hd.h, B.ptr(x), x.shape[0], B.ptr(F), B.ptr(J), B.stream_ptr(hd.device)))
            return F, J
        check(lib.sr_gp_paths_eval(hd.h, B.ptr(x), x.shape[0], B.ptr(F), B.stream_ptr(hd.device)))
        return F

    def sample_paths(self, x, jacobians=False):
        """sample_paths_device, NumPy in / NumPy out (a tensor in: a tensor out)."""
        out = self.sample_paths_device(x, jacobians)
        if B.is_tensor(x):
            return out
        return tuple(B.to_numpy(o) for o in out) if jacobians else B.to_numpy(out)

    def paths_step_device(self, x_s, k_fb=None, k_ff=None, jacobians=False):
        """Path s at its OWN input: x_s (size, D) -> F (size, n_s_out).  With k_fb (n_u, n_s_out) and k_ff (n_u,) the
        closed-loop next inputs [F, k_fb F + k_ff] (size, D) are returned as well, as sample_device returns them.
        jacobians=True: J (size, n_s_out, D), the derivative of F[s] in x_s[s], comes last: (F, J) or (F, z_next, J)."""
        self._need_trained()
        hd = self._handle
        S = self._need_paths()
        x = B.as_dev(x_s, hd.device, (S, hd.D))
        F = B.empty((S, hd.n_out), hd.device)
        z = tk = tf = None
        if k_fb is not None:
            n_u = hd.D - hd.n_out
            if n_u < 1:
                raise ValueError("next inputs need D = n_s_out + n_u")
            tk = B.as_dev(k_fb, hd.device, (n_u, hd.n_out))
            tf = B.as_dev(k_ff, hd.device, (n_u,))
            z = B.empty((S, hd.D), hd.device)
        if jacobians:
            J = B.empty((S, hd.n_out, hd.D), hd.device)
            check(lib.sr_gp_paths_step_grad(hd.h, B.ptr(x), B.ptr(F), B.ptr(J), B.ptr(tk), B.ptr(tf), B.ptr(z),
                                            B.stream_ptr(hd.device)))
            return (F, J) if z is None else (F, z, J)
        check(lib.sr_gp_paths_step(hd.h, B.ptr(x), B.ptr(F), B.ptr(tk), B.ptr(tf), B.ptr(z), B.stream_ptr(hd.device)))
        return F if z is None else (F, z)

    def paths_rollout_device(self, x0, K, k, jacobians=False):
        """Every drawn path through the closed loop u_i = K[i] x_i + k[i] in ONE launch (sr_gp_paths_rollout): x0 (n_s,) or
        (n_s, 1) is the start of every path, (size, n_s) one start per path; K (H, n_u, n_s), k (H, n_u).  Returns the tensor
        X_all (H, size, n_s) of the states after steps 1 .. H -- what H chained paths_step_device calls give, to rounding --
        and with jacobians=True (X_all, A_all), A_all (H, size, n_s, n_s) = J_x + J_u K[i] per step and path.
        "rbf" models only: NotImplementedError for a model with a "lin_rbf" output (chain paths_step_device, as
        MonteCarloSafetyVerification.rollout_paths does)."""
        self._need_trained()
        if not self._paths_fused_rollout_supported():
            raise NotImplementedError("paths_rollout_device: the roll-out in one launch is for ARD-RBF models only")
        hd = self._handle
        n_s, n_u = hd.n_out, hd.D - hd.n_out
        if n_u < 1:
            raise ValueError("the closed loop needs D = n_s_out + n_u")
        K, k = B.as_dev(K, hd.device), B.as_dev(k, hd.device)
        H = K.shape[0] if K.dim() == 3 else 0
        if H < 1 or tuple(K.shape) != (H, n_u, n_s) or tuple(k.shape) != (H, n_u):
            raise ValueError("K must be (H, {}, {}) and k (H, {}) with H >= 1".format(n_u, n_s, n_u))
        S = self._need_paths()
        x = B.as_dev(x0, hd.device)
        if tuple(x.shape) in ((n_s,), (n_s, 1)):
            x, per_path = x.reshape(n_s), 0
        elif tuple(x.shape) == (S, n_s):
            per_path = 1
        else:
            raise ValueError("x0 must be ({0},), ({0}, 1) or ({1}, {0})".format(n_s, S))
        X_all = B.empty((H, S, n_s), hd.device)
        A_all = B.empty((H, S, n_s, n_s), hd.device) if jacobians else None
        check(lib.sr_gp_paths_rollout(hd.h, B.ptr(x), per_path, H, B.ptr(K), B.ptr(k), B.ptr(X_all), B.ptr(A_all),
                                      B.stream_ptr(hd.device)))
        return (X_all, A_all) if jacobians else X_all

    def paths_rollout_vjp_device(self, x0, K, k, X_all, X_bar, jacobians=False):
        """The reverse pass of paths_rollout_device (sr_gp_paths_rollout_vjp): x0, K, k as the forward took them, X_all
        (H, size, n_s) the states it returned, X_bar (H, size, n_s) the seeds of L = sum X_bar * X_all.  Returns the tensors
        (x0_bar, K_bar, k_bar) -- x0_bar in the shape of x0 (a shared start: the sum over the paths), K_bar (H, n_u, n_s),
        k_bar (H, n_u), both summed over the paths -- and with jacobians=True J_all (H, size, n_s, D) behind them, the
        Jacobian of every step and path in its input [x_i, K[i] x_i + k[i]].  Deterministic: the same bits on every call, with
        and without J_all.  The model and the draws get no gradient."""
        self._need_trained()
        hd = self._handle
        n_s, n_u = hd.n_out, hd.D - hd.n_out
        if n_u < 1:
            raise ValueError("the closed loop needs D = n_s_out + n_u")
        K, k = B.as_dev(K, hd.device), B.as_dev(k, hd.device)
        H = K.shape[0] if K.dim() == 3 else 0
        if H < 1 or tuple(K.shape) != (H, n_u, n_s) or tuple(k.shape) != (H, n_u):
            raise ValueError("K must be (H, {}, {}) and k (H, {}) with H >= 1".format(n_u, n_s, n_u))
        S = self._need_paths()
        x = B.as_dev(x0, hd.device)
        shape0 = tuple(x.shape)
        if shape0 in ((n_s,), (n_s, 1)):
            x, per_path = x.reshape(n_s), 0
        elif shape0 == (S, n_s):
            per_path = 1
        else:
            raise ValueError("x0 must be ({0},), ({0}, 1) or ({1}, {0})".format(n_s, S))
        X_all, X_bar = B.as_dev(X_all, hd.device), B.as_dev(X_bar, hd.device)
        if tuple(X_all.shape) != (H, S, n_s) or tuple(X_bar.shape) != (H, S, n_s):
            raise ValueError("X_all and X_bar must be ({}, {}, {})".format(H, S, n_s))
        x0_bar = B.empty((S, n_s) if per_path else (n_s,), hd.device)
        K_bar, k_bar = B.empty((H, n_u, n_s), hd.device), B.empty((H, n_u), hd.device)
        J_all = B.empty((H, S, n_s, hd.D), hd.device) if jacobians else None
        check(lib.sr_gp_paths_rollout_vjp(hd.h, B.ptr(x), per_path, H, B.ptr(K), B.ptr(k), B.ptr(X_all), B.ptr(X_bar),
                                          B.ptr(x0_bar), B.ptr(K_bar), B.ptr(k_bar), B.ptr(J_all), B.stream_ptr(hd.device)))
        x0_bar = x0_bar.reshape(shape0)
        return (x0_bar, K_bar, k_bar, J_all) if jacobians else (x0_bar, K_bar, k_bar)

    def paths_rollout_diff_device(self, x0, K, k):
        """paths_rollout_device(x0, K, k) -- the same bits -- as a node of torch's autograd graph: the backward is
        paths_rollout_vjp_device at the stored states, once differentiable, with gradients for those of x0, K, k that
        require them (not for the model or the draws).  "rbf" models only (NotImplementedError otherwise)."""
        self._need_trained()
        if not self._paths_fused_rollout_supported():
            raise NotImplementedError("paths_rollout_diff_device: the reverse pass of the roll-out is for ARD-RBF models only")
        self._need_paths()
        dev = self._handle.device
        return _PathsRolloutFn.apply(self, B.as_dev(x0, dev), B.as_dev(K, dev), B.as_dev(k, dev))

    def information_gain(self, x=None):
        """Mutual information between the training samples and the system  gaussian_process.py:621-634:
        per output log det(I + K/sigma_n^2) = log det(K + sigma_n^2 I) - N log sigma_n^2, sigma_n^2 being the
        fixed Gaussian noise incl. noise_diag.  The reference always uses the TRAINING Gram matrix
        (``posterior._K``) and x only for its size, so only x=None / x=z is meaningful.  The factor held
        here carries GPy's 1e-8 inference jitter on top: absolute deviation <= N*1e-8/sigma_n^2."""
        self._need_trained()
        hd = self._handle
        if self.do_sparse_gp or lib.sr_gp_is_sparse(hd.h) == 1:
            raise NotImplementedError("information_gain of a sparse model: its factor is not that of K_y")
        if x is not None and np.shape(x)[0] != hd.N:
            raise ValueError("information_gain is defined on the training inputs (got {} rows, model holds {})"
                             .format(np.shape(x)[0], hd.N))
        nv = self._noise + float(self._noise_diag)
        host = (ctypes.c_double * hd.n_out)()
        if lib.sr_gp_logdet_cached(hd.h, host) == 0:   # the last model update read it back with its status words
            return [float(v) for v in np.array(host[:]) - hd.N * np.log(nv)]
        st = getattr(hd, "_staging", None)          # (the result comes back through the pinned block of the NumPy routes)
        if st is None:
            st = hd._staging = B.Staging(hd.device)
        _, (out,) = st.stage([], [(hd.n_out,)])
        check(lib.sr_gp_logdet(hd.h, B.ptr(out), B.stream_ptr(hd.device)))
        ld = st.fetch()[0] - hd.N * np.log(nv)
        return [float(v) for v in ld]

    # ------------------------------------------------------------------ measurement hooks
    def set_chunk(self, chunk):
        self._need_trained()
        check(lib.sr_gp_set_chunk(self._handle.h, int(chunk)))

    def set_var_group(self, group):
        self._need_trained()
        check(lib.sr_gp_set_var_group(self._handle.h, int(group)))

    def set_var_variant(self, variant):
        self._need_trained()
        check(lib.sr_gp_set_var_variant(self._handle.h, int(variant)))

    def set_fact_panel(self, panel):
        """blocks per Cholesky panel of the NEXT model update (0 = by size); works before training too"""
        self._fact_panel = int(panel)
        if self._handle is not None:
            check(lib.sr_gp_set_fact_panel(self._handle.h, int(panel)))

    def set_fact_pipeline(self, on):
        """model updates of 3 .. 128 blocks of 128 rows: 0 (default) one chain of launches; 1 / 2 the pipelined prototypes of
        round 6 (diagonal blocks beside the previous block row: measured slower; identical numbers); 3 the
        tile-flow Cholesky (one resident kernel of tile tasks, csrc/sr_flow.hip: at parity, results to rounding); -1 never the
        tile flow (sr_gp_set_fact_pipeline).  Works before training too."""
        self._fact_pipeline = int(on)
        if self._handle is not None:
            check(lib.sr_gp_set_fact_pipeline(self._handle.h, self._fact_pipeline))

    def fact_pipelined(self):
        """did the last model update run pipelined? (sr_gp_fact_pipelined)"""
        self._need_trained()
        return bool(lib.sr_gp_fact_pipelined(self._handle.h))

    def fact_route(self):
        """how the last model update ran: 0 one chain of launches, 1 pipelined prototype, 4 tile-flow Cholesky (one resident
        kernel, ``set_fact_pipeline(3)``)"""
        self._need_trained()
        return int(lib.sr_gp_fact_pipelined(self._handle.h))

    ROUTE_WORDS = ("route", "src", "width", "nc", "kc", "kr", "nitems", "nwg", "multi", "reduce_items", "polled", "nsplit",
                   "bal_wgs", "final", "unslid", "T")
    ROUTE_NAMES = (None, "K0", "stream1", "mfma1", "runs", "K2s", "K2b", "K2m", "K2")

    def last_route(self):
        """which kernels the last posterior pass launched (sr_gp_last_route): a dict of ROUTE_WORDS, "route" by name
        (ROUTE_NAMES; None before the first pass).  Diagnostics: tests use it to know which kernel form they met."""
        self._need_trained()
        out = (ctypes.c_int * len(self.ROUTE_WORDS))()
        n = lib.sr_gp_last_route(self._handle.h, out, len(out))
        if n != len(out):
            check(n if n < 0 else -1)
        d = dict(zip(self.ROUTE_WORDS, (int(v) for v in out)))
        d["route"] = self.ROUTE_NAMES[d["route"]]
        return d

    UPDATE_FIT_WORDS = ("kind", "nb", "panel", "regime", "own_streams", "n_par", "rounds", "inv_stages", "form")
    UPDATE_APPEND_WORDS = ("kind", "route", "in_place", "Np0", "Np1", "spare")
    UPDATE_KINDS = (None, "fit", "append")
    UPDATE_FORMS = ("plain", "pipelined", "flow")
    UPDATE_ROUTES = ("small", "one_wg", "grid", "tile")

    def last_update(self):
        """how the last model update ran (sr_gp_last_update): a dict of UPDATE_FIT_WORDS after a fit ("form" by name), of
        UPDATE_APPEND_WORDS after an append ("route" by name); "kind" is "fit" / "append".  Diagnostics."""
        self._need_trained()
        out = (ctypes.c_int * len(self.UPDATE_FIT_WORDS))()
        n = lib.sr_gp_last_update(self._handle.h, out, len(out))
        if n != len(out):
            check(n if n < 0 else -1)
        kind = self.UPDATE_KINDS[int(out[0])]
        if kind == "append":
            d = dict(zip(self.UPDATE_APPEND_WORDS, (int(v) for v in out)))
            d["route"] = self.UPDATE_ROUTES[d["route"]]
        else:
            d = dict(zip(self.UPDATE_FIT_WORDS, (int(v) for v in out)))
            d["form"] = self.UPDATE_FORMS[d["form"]]
        d["kind"] = kind
        return d

    REMOVE_WORDS = ("count", "Np0", "Np1", "off0", "q", "slide", "aligned", "spare", "vec_spare", "clean", "kept_old")
    REMOVE_SPARES = ("none", "as_is", "cleared")

    def last_remove(self):
        """how sr_gp_remove retired its last point (sr_gp_last_remove): a dict of REMOVE_WORDS, "spare" by name (REMOVE_SPARES);
        "count" is the number of points retired since the last fit.  Diagnostics."""
        self._need_trained()
        out = (ctypes.c_int * len(self.REMOVE_WORDS))()
        n = lib.sr_gp_last_remove(self._handle.h, out, len(out))
        if n != len(out):
            check(n if n < 0 else -1)
        d = dict(zip(self.REMOVE_WORDS, (int(v) for v in out)))
        d["spare"] = self.REMOVE_SPARES[d["spare"]]
        return d

    def get_forward_model_casadi(self, linearize_mu=True):
        """state_space_models.py:140-166.  The evaluator calls the model once per IPOPT callback and blocks: the resident
        single-query server is armed for it (``start_server``; SR_NO_SERVER=1 in the environment keeps the launched
        routes)."""
        if self.gp_trained and not os.environ.get("SR_NO_SERVER"):
            try:
                self.start_server()
            except RuntimeError:
                pass                                   # the launched routes serve the evaluator
        return super(SimpleGPModel, self).get_forward_model_casadi(linearize_mu)

    def start_server(self, idle_timeout_s=0.005):
        """Put the RESIDENT single-query server of this model on the device (sr_gp_server_start): one workgroup per output
        polls a mailbox in pinned host memory, so that ``__call__`` / ``linearize_predict`` / a one-row ``predict`` cost one
        PCIe round trip plus the evaluation instead of a kernel launch each -- the regime of the MPC's IPOPT callbacks
        (state_space_models.py:278-303, 384-417).  The kernel leaves by itself after ``idle_timeout_s`` without a query
        (so a ``torch.cuda.synchronize()`` elsewhere waits at most that long) and comes back with the next one; model
        updates take it off the device and leave it armed.  Every kernel identifier is served ("rbf", and since round 5
        "mat52" / "lin_rbf" / "lin_mat52", the kernels of the reference's journal experiments); queries are in the GP's
        input space.  Returns False where the model has no such server (more than 512 padded points, more than 5
        inputs): the launched routes serve it as before."""
        self._need_trained()
        hd = self._handle
        hd.single_io()
        rc = lib.sr_gp_server_start(hd.h, float(idle_timeout_s))
        if rc == -5:
            hd._server_armed = False
            return False
        check(rc)
        hd._server_armed = True
        hd._server_idle = float(idle_timeout_s)
        return True

    def stop_server(self):
        """Take the resident server off the device and disarm it (sr_gp_server_stop)."""
        hd = self._handle
        if hd is not None and getattr(hd, "_server_armed", False):
            hd._server_armed = False
            check(lib.sr_gp_server_stop(hd.h))

    def server_state(self):
        """(armed, resident, launches, calls) of the resident server."""
        self._need_trained()
        a, r = ctypes.c_int(0), ctypes.c_int(0)
        nl, nc = ctypes.c_long(0), ctypes.c_long(0)
        check(lib.sr_gp_server_state(self._handle.h, ctypes.byref(a), ctypes.byref(r), ctypes.byref(nl), ctypes.byref(nc)))
        return bool(a.value), bool(r.value), nl.value, nc.value

    def set_small_path(self, on):
        self._need_trained()
        check(lib.sr_gp_set_small_path(self._handle.h, int(on)))

    def release_scratch(self):
        """free what the model update / row append keep for their next call (two Np x Np matrices per output)"""
        self._need_trained()
        check(lib.sr_gp_release_scratch(self._handle.h))

    def set_chain(self, on):
        """multi-step chains of small models inside one persistent launch (default) or step by step"""
        self._need_trained()
        check(lib.sr_gp_set_chain(self._handle.h, int(bool(on))))

    @property
    def last_chain(self):
        """True if the last multi-step chain ran inside the persistent kernel"""
        self._need_trained()
        return bool(lib.sr_gp_last_chain(self._handle.h))

    def prof_enable(self, on=True):
        self._need_trained()
        check(lib.sr_prof_enable(self._handle.h, 1 if on else 0))

    def prof_reset(self):
        self._need_trained()
        check(lib.sr_prof_reset(self._handle.h))

    def prof_get(self, kernel_id):
        self._need_trained()
        ms = ctypes.c_double(0.0)
        n = ctypes.c_long(0)
        check(lib.sr_prof_get(self._handle.h, kernel_id, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value
