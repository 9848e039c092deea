"""Planning through exact moment matching: the gradient of an expected quadratic cost over H steps of
x+ = a x + b (K_i x + k_ff,i) + g([x; u]) in the feed-forward controls and the feedback gains, and one descent step.

    python examples/moment_matching_gradient.py

Needs a GPU.  Two routes to the same gradient:
  chained   every step's GP call is sr_gp_moment_match, and its backward is sr_gp_moment_match_vjp (the reverse pass in the
            Gaussian input's mean and covariance); the small closed-loop algebra between the calls is batched torch,
            differentiated by autograd: H autograd nodes;
  one call  the whole roll-out is ONE autograd node (moment_matching_rollout_diff_batch): the forward is the fused roll-out
            (sr_gp_moment_match_rollout), the backward one call of sr_gp_moment_match_rollout_vjp."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from safe_exploration_amd import SimpleGPModel                                    # noqa: E402
from safe_exploration_amd import uncertainty_propagation_casadi as up             # noqa: E402


def expected_cost(mu_all, sigma_all, target, Qc):
    """sum over the steps of E[(x - target)^T Qc (x - target)] = (mu - target)^T Qc (mu - target) + tr(Qc Sigma)"""
    e = mu_all - target
    return (e.matmul(Qc) * e).sum() + (Qc * sigma_all).sum()


def main():
    rng = np.random.default_rng(0)
    n_s, n_u, N, H, T = 2, 1, 150, 6, 4
    Z = rng.uniform(-1, 1, (N, n_s + n_u))
    Y = 0.2 * np.sin(2.0 * Z.dot(rng.standard_normal((n_s + n_u, n_s)))) + 0.01 * rng.standard_normal((N, n_s))
    hyp = [{"lengthscale": np.full(n_s + n_u, 0.8), "variance": 0.05, "noise_variance": 1e-4} for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    dev = gp.device
    a, b = 0.9 * np.eye(n_s), np.array([[0.0], [0.3]])
    mu_0 = torch.as_tensor(0.3 * rng.standard_normal((T, n_s)), device=dev)
    sigma_0 = torch.as_tensor(np.tile(np.diag([0.01, 0.02]), (T, 1, 1)), device=dev)
    k_ff = torch.as_tensor(0.1 * rng.standard_normal((T, H, n_u)), device=dev).requires_grad_(True)
    k_fb = torch.as_tensor(-0.3 * np.ones((T, H - 1, n_u, n_s)), device=dev).requires_grad_(True)
    target = torch.zeros(n_s, dtype=torch.float64, device=dev)
    Qc = torch.eye(n_s, dtype=torch.float64, device=dev)

    def cost(kff, kfb, differentiable):
        mu_all, sigma_all, _ = up.moment_matching_batch(mu_0, gp, kff, kfb, a, b, sigma_0, differentiable=differentiable)
        return expected_cost(mu_all, sigma_all, target, Qc)

    c0 = cost(k_ff, k_fb, True)
    g_ff, g_fb = torch.autograd.grad(c0, (k_ff, k_fb))
    c0 = c0.detach()
    print("expected cost of %d roll-outs over %d steps: %.6f" % (T, H, float(c0)))
    print("|d cost / d k_ff| = %.4f, |d cost / d k_fb| = %.4f" % (float(g_ff.norm()), float(g_fb.norm())))
    # the same gradient with the whole roll-out as one autograd node
    mu_all, sigma_all, _ = up.moment_matching_rollout_diff_batch(mu_0, gp, k_ff, k_fb, a, b, sigma_0)
    r_ff, r_fb = torch.autograd.grad(expected_cost(mu_all, sigma_all, target, Qc), (k_ff, k_fb))
    off = max(float((r_ff - g_ff).abs().max() / g_ff.abs().max()), float((r_fb - g_fb).abs().max() / g_fb.abs().max()))
    print("one call for the whole roll-out: the two gradients agree to %.1e of their largest element" % off)
    assert off < 1e-8
    # one descent step; the step length is a backtracking search from 1
    step = 1.0
    with torch.no_grad():
        while step > 1e-6:
            c1 = cost(k_ff - step * g_ff, k_fb - step * g_fb, False)
            if float(c1) < float(c0):
                break
            step *= 0.5
    print("after one descent step of length %.3g: %.6f (lower by %.3g)" % (step, float(c1), float(c0) - float(c1)))
    assert float(c1) < float(c0)


if __name__ == "__main__":
    main()
