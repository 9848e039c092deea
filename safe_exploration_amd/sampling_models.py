"""Monte-Carlo verification of the ellipsoidal state bounds (reference: sampling_models.py:14-107).

Every propagation step is ONE batched GP evaluation of all n_samples particles on the GPU
(`SimpleGPModel.sample_device`: K* -> variance contraction -> `sr_gp_sample`), the particles never
leave HBM between steps; the containment test is the batched `sr_distance_to_center` kernel.
"""
import numpy as np

from . import _buffers as B
from .utils_ellipsoid import distance_to_center_batch


class MonteCarloSafetyVerification(object):
    """Verify probabilistic state bounds of a GP dynamic system through sampling."""

    def __init__(self, GP):
        self.GP = GP
        self.n_s = getattr(GP, "n_s", None) or GP.n_s_out    # the reference reads GP.n_s (:30); SimpleGPModel has n_s_out
        self.n_u = GP.n_u

    def sample_n_step(self, x0, K, k, n=1, n_samples=1000, eps=None, generator=None, as_tensor=False, consistent=False,
                      n_features=1024):
        """Sample from the n-step-ahead distribution of the closed loop u_i = K[i] x_i + k[i].

        x0 (n_s, 1) deterministic start; K (n, n_u, n_s); k (n, n_u)  (sampling_models.py:33-80).
        eps (n, n_samples, n_s): optional standard-normal draws (default: the device generator).
        consistent=True: every particle is rolled through ITS OWN posterior function (SimpleGPModel.draw_paths: pathwise
        conditioning on n_features random features) instead of meeting an unrelated marginal draw at every step; the
        model's valid paths are used if there are n_samples of them, otherwise they are drawn here (eps is not read).
        Models of "rbf" and "lin_rbf" kernels (NotImplementedError for a Matern kernel).
        Returns S (n_samples, n_s) and S_all (n, n_samples, n_s).  With the transition Jacobians of the consistent rollout:
        sample_n_step_jacobians."""
        if consistent:
            return self._consistent_rollout(x0, K, k, n, n_samples, generator, as_tensor, n_features, False)
        n_s, n_u = self.n_s, self.n_u
        K, k, inp = self._closed_loop_start(x0, K, k, n)
        dev = self.GP.device
        S_all = B.empty((n, n_samples, n_s), dev)
        for i in range(n):
            e = None
            if eps is not None:
                e = B.as_dev(eps[i], dev, (n_samples, n_s))
                e = e[None] if i == 0 else e[:, None]
            size = n_samples if i == 0 else 1
            if i + 1 < n:
                S, z = self.GP.sample_device(inp, size, e, generator, K[i + 1], k[i + 1])
                inp = z.reshape(n_samples, n_s + n_u)
            else:
                S = self.GP.sample_device(inp, size, e, generator)
            S_all[i].copy_(S.reshape(n_samples, n_s))
        if as_tensor:
            return S_all[n - 1], S_all
        out = B.to_numpy(S_all)
        return out[n - 1].squeeze(), out

    def sample_n_step_jacobians(self, x0, K, k, n=1, n_samples=1000, generator=None, as_tensor=False, consistent=True,
                                n_features=1024):
        """sample_n_step(consistent=True) with the closed-loop transition Jacobian of every step and particle: returns
        S (n_samples, n_s), S_all (n, n_samples, n_s) -- bit for bit those of sample_n_step(consistent=True) on the same
        paths -- and A_all (n, n_samples, n_s, n_s), A_all[i] = J_i[..., :n_s] + J_i[..., n_s:] K[i] = d x_{i+1} / d x_i with
        J_i the Jacobian of the particle's own path at step i's input (paths_step_device(jacobians=True)); d x_n / d x_0 is
        their ordered product.  consistent=False raises ValueError: a marginal draw has no function to differentiate."""
        if not consistent:
            raise ValueError("sample_n_step_jacobians needs consistent=True (a marginal draw has no function to differentiate)")
        return self._consistent_rollout(x0, K, k, n, n_samples, generator, as_tensor, n_features, True)

    def _closed_loop_start(self, x0, K, k, n):
        n_s, n_u = self.n_s, self.n_u
        assert n > 0, "The time horizon n for the multi-step sampling must be positive!"
        assert np.shape(K) == (n, n_u, n_s), "Required shape of K is ({},{},{})".format(n, n_u, n_s)
        assert np.shape(k) == (n, n_u), "Required shape of k is ({},{})".format(n, n_u)
        K = np.asarray(K, dtype=np.float64)
        k = np.asarray(k, dtype=np.float64)
        x0 = np.asarray(x0, dtype=np.float64).reshape(n_s, 1)
        u0 = K[0].dot(x0) + k[0, :, None]
        return K, k, np.vstack((x0, u0)).T

    def _consistent_rollout(self, x0, K, k, n, n_samples, generator, as_tensor, n_features, jacobians):
        """every particle through its own path (drawn here unless the model holds n_samples valid ones); with jacobians the
        batched product J_x + J_u K[i] per step on the device"""
        n_s, n_u = self.n_s, self.n_u
        K, k, inp = self._closed_loop_start(x0, K, k, n)
        dev = self.GP.device
        S_all = B.empty((n, n_samples, n_s), dev)
        if self.GP.paths_count()[0] != n_samples:
            self.GP.draw_paths(n_samples, n_features, generator)
        inp = B.as_dev(inp, dev, (1, n_s + n_u)).expand(n_samples, n_s + n_u).contiguous()
        if jacobians:
            A_all = B.empty((n, n_samples, n_s, n_s), dev)
            Kt = B.as_dev(K, dev, (n, n_u, n_s))
        for i in range(n):
            if i + 1 < n:
                out = self.GP.paths_step_device(inp, K[i + 1], k[i + 1], jacobians=jacobians)
                S, inp = out[0], out[1]
            else:
                out = self.GP.paths_step_device(inp, jacobians=jacobians)
                S = out[0] if jacobians else out
            S_all[i].copy_(S)
            if jacobians:
                J = out[-1]
                A_all[i].copy_(J[..., :n_s] + J[..., n_s:].matmul(Kt[i]))
        res = (S_all[n - 1], S_all) + ((A_all,) if jacobians else ())
        if as_tensor:
            return res
        out = tuple(B.to_numpy(t) for t in res[1:])
        return (out[0][n - 1].squeeze(),) + out

    def rollout_paths(self, x0, K, k, n=1, n_samples=1000, generator=None, as_tensor=False, n_features=1024, jacobians=False):
        """The consistent roll-out in ONE launch (SimpleGPModel.paths_rollout_device): what sample_n_step(consistent=True)
        computes step by step -- to rounding, not bit for bit -- and returns as it does, S (n_samples, n_s) and S_all
        (n, n_samples, n_s); with jacobians=True what sample_n_step_jacobians returns, (S, S_all, A_all).  x0 may also be
        (n_samples, n_s): one start per particle.  The model's valid paths are used if there are n_samples of them,
        otherwise they are drawn here.  A model with a "lin_rbf" output has no one-launch roll-out: it goes through the
        chained route of sample_n_step(consistent=True) (a single start x0 only)."""
        n_s, n_u = self.n_s, self.n_u
        assert n > 0, "The time horizon n for the multi-step sampling must be positive!"
        assert np.shape(K) == (n, n_u, n_s), "Required shape of K is ({},{},{})".format(n, n_u, n_s)
        assert np.shape(k) == (n, n_u), "Required shape of k is ({},{})".format(n, n_u)
        if not self.GP._paths_fused_rollout_supported():
            if np.ndim(x0) == 2 and np.shape(x0) == (n_samples, n_s) and np.shape(x0) != (n_s, 1):
                raise NotImplementedError("rollout_paths: one start per particle needs the roll-out in one launch, which is for "
                                          "ARD-RBF models only; a model with a lin_rbf output takes a single start x0")
            return self._consistent_rollout(x0, K, k, n, n_samples, generator, as_tensor, n_features, jacobians)
        if self.GP.paths_count()[0] != n_samples:
            self.GP.draw_paths(n_samples, n_features, generator)
        out = self.GP.paths_rollout_device(x0, K, k, jacobians=jacobians)
        S_all = out[0] if jacobians else out
        res = (S_all[n - 1], S_all) + ((out[1],) if jacobians else ())
        if as_tensor:
            return res
        out = tuple(B.to_numpy(t) for t in res[1:])
        return (out[0][n - 1].squeeze(),) + out

    def rollout_paths_diff(self, x0, K, k, n=1, n_samples=1000, generator=None, n_features=1024):
        """rollout_paths as a node of torch's autograd graph (SimpleGPModel.paths_rollout_diff_device): returns the tensors
        S (n_samples, n_s), a view of S_all[n - 1], and S_all (n, n_samples, n_s) -- the bits of rollout_paths -- and a cost
        of them can be differentiated once in those of x0, K, k that are tensors requiring a gradient (the reverse pass on
        the device, sr_gp_paths_rollout_vjp; the model and the draws get none).  The paths are drawn under rollout_paths'
        rule: the model's valid ones if there are n_samples of them.  "rbf" models only: NotImplementedError for a model
        with a "lin_rbf" output, before anything is drawn."""
        if not self.GP._paths_fused_rollout_supported():
            raise NotImplementedError("rollout_paths_diff: the reverse pass of the roll-out is for ARD-RBF models only")
        n_s, n_u = self.n_s, self.n_u
        assert n > 0, "The time horizon n for the multi-step sampling must be positive!"
        assert tuple(np.shape(K)) == (n, n_u, n_s), "Required shape of K is ({},{},{})".format(n, n_u, n_s)
        assert tuple(np.shape(k)) == (n, n_u), "Required shape of k is ({},{})".format(n, n_u)
        if self.GP.paths_count()[0] != n_samples:
            self.GP.draw_paths(n_samples, n_features, generator)
        S_all = self.GP.paths_rollout_diff_device(x0, K, k)
        return S_all[n - 1], S_all

    def inside_ellipsoid_ratio(self, S, Q, p):
        """Ratio of samples inside the ellipsoid of each time step  (sampling_models.py:82-107).

        S (n, n_samples, n_s); Q (n, n_s, n_s); p (n, n_s) -> Ratio (n,), R_bool (n, n_samples)."""
        as_t = B.is_tensor(S)
        dev = S.device if as_t else self.GP.device
        n = np.shape(S)[0]
        inside = distance_to_center_batch(B.as_dev(S, dev), B.as_dev(p, dev, (n, self.n_s)),
                                          B.as_dev(Q, dev, (n, self.n_s, self.n_s))) < 1.0
        ratio = inside.double().mean(dim=1)
        if as_t:
            return ratio, inside
        return B.to_numpy(ratio), inside.cpu().numpy()
