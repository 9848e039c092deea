"""Policy search on consistent Monte-Carlo roll-outs: the feedback gains K[i] and the feed-forward terms k[i] of the closed
loop u_i = K[i] x_i + k[i] are tuned by a torch optimiser on an expected quadratic cost plus a soft state-constraint penalty
over S posterior function samples (one plausible system per particle).  The forward is the roll-out in one launch, the
gradient its reverse pass on the device (MonteCarloSafetyVerification.rollout_paths_diff: sr_gp_paths_rollout and
sr_gp_paths_rollout_vjp); the paths are drawn once, so every iteration sees the same systems (common random numbers).

    python examples/rollout_policy_gradient.py

The model is the synthetic one of examples/consistent_rollouts.py.  Needs a GPU."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd import SimpleGPModel                                    # noqa: E402
from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification     # noqa: E402


def main(steps=15):
    rng = np.random.default_rng(0)
    n_s, n_u, N, n, S = 2, 1, 150, 8, 1024
    Z = rng.uniform(-1, 1, (N, n_s + n_u))
    Y = 0.8 * Z[:, :n_s] + 0.2 * np.sin(2.0 * Z.dot(rng.standard_normal((n_s + n_u, n_s)))) + 0.01 * rng.standard_normal((N, n_s))
    hyp = [{"lengthscale": np.array([0.7, 0.9, 1.1]), "variance": 0.5, "noise_variance": 1e-3} for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    dev = gp.device
    gp.draw_paths(S, n_features=1024, generator=torch.Generator(device=dev).manual_seed(1))
    mc = MonteCarloSafetyVerification(gp)

    x0 = np.array([[0.4], [-0.3]])
    x0_t = torch.as_tensor(x0[:, 0], device=dev)
    K = torch.zeros((n, n_u, n_s), dtype=torch.float64, device=dev, requires_grad=True)
    k = torch.zeros((n, n_u), dtype=torch.float64, device=dev, requires_grad=True)
    q = torch.tensor([1.0, 0.5], dtype=torch.float64, device=dev)                   # state weights of the quadratic cost
    r, x_max, rho = 0.05, 0.35, 10.0                                                # control weight, |x_0| <= x_max, penalty

    def cost():
        _, X = mc.rollout_paths_diff(x0, K, k, n=n, n_samples=S)                    # (n, S, n_s): x_1 .. x_n of every path
        u = torch.einsum("iqc,isc->isq", K[1:], X[:-1]) + k[1:, None, :]            # the controls at x_1 .. x_{n-1}
        u0 = K[0] @ x0_t + k[0]                                                     # ... and at the start
        quad = (q * X ** 2).sum(-1).mean(1).sum() + r * ((u ** 2).sum(-1).mean(1).sum() + (u0 ** 2).sum())
        soft = rho * (torch.relu(X[..., 0].abs() - x_max) ** 2).mean(1).sum()       # soft constraint on the first state
        return quad + soft, float((X[..., 0].abs() > x_max).double().mean())

    opt = torch.optim.Adam([K, k], lr=0.02)
    print("step   expected cost   share of (step, path) pairs outside |x_0| <= %.2f" % x_max)
    first = last = None
    for it in range(steps):
        opt.zero_grad()
        c, outside = cost()
        c.backward()                                                                # one reverse pass on the device
        opt.step()
        last = float(c.detach())
        first = last if first is None else first
        print("%4d   %.6f        %.4f" % (it, last, outside))
    with torch.no_grad():
        c, outside = cost()
    print("%4d   %.6f        %.4f" % (steps, float(c), outside))
    assert float(c) < first, "the cost did not go down"
    print("cost %.6f -> %.6f over %d steps of Adam on K (%s) and k (%s)" % (first, float(c), steps, tuple(K.shape), tuple(k.shape)))


if __name__ == "__main__":
    main()
