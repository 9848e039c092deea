"""The objective of the reference's journal experiments on the device: generic_cost over a moment trajectory with trig_aug as the
state transformation and loss_sat as stage and terminal cost (defaultconfig_episode.py:118-164) -- the cart-pole's idx_angle = 2,
z = [2.5, 0, 0, 0, 0.5], W = diag(20, 0, 0, 0, 5) / 100 -- on a Taylor (mode 1) roll-out and on an exact moment-matching roll-out
of a batch of trajectories through a GP of the cart-pole's shape (n_s = 4, n_u = 1).

    python examples/cautious_shooting_cost.py

Needs a GPU.  The gradient of the summed objective in k_ff, k_fb is computed two ways:
  three library calls   the roll-out, utils_casadi.rollout_cost_vjp_batch (the seeds mu_all_bar, sigma_all_bar), the roll-out's
                        reverse pass (multistep_moments_vjp_batch / moment_matching_rollout_vjp_batch): no autograd graph;
  torch port            the same roll-out as one autograd node (the *_diff_batch surfaces) and the cost written in batched torch
                        fp64 (linalg.inv, det, cat and index selection), differentiated by autograd.
Prints the cost, the largest element of either gradient and their distance (of the largest element)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from safe_exploration_amd import SimpleGPModel, utils_casadi                      # noqa: E402
from safe_exploration_amd import uncertainty_propagation_casadi as prop           # noqa: E402

IDX_ANGLE = 2
Z_TARGET = np.array([2.5, 0.0, 0.0, 0.0, 0.5])
W_TARGET = np.diag([20.0, 0.0, 0.0, 0.0, 5.0]) / 100.0


def torch_cost(mu_all, sigma_all, z, W, idx, a=1.0):
    """The reference's expressions in batched torch: trig_aug (the angle dropped), loss_sat at every step, summed over the steps."""
    T, H, n_s = mu_all.shape
    m, v = mu_all.reshape(T * H, n_s), sigma_all.reshape(T * H, n_s, n_s)
    v = (v + v.transpose(1, 2)) / 2
    th, s2 = m[:, idx], v[:, idx, idx]
    e0, e1 = torch.exp(-s2 / 2), torch.exp(-2 * s2)
    ms, mc = e0 * torch.sin(th), e0 * torch.cos(th)
    ess, ecc, esc = (1 - e1 * torch.cos(2 * th)) / 2, (1 + e1 * torch.cos(2 * th)) / 2, e1 * torch.sin(2 * th) / 2
    vt = a * a * torch.stack((torch.stack((ess - ms ** 2, esc - ms * mc), dim=1), torch.stack((esc - ms * mc, ecc - mc ** 2), dim=1)), dim=1)
    C = v[:, :, idx:idx + 1] * torch.stack((a * mc, -a * ms), dim=1)[:, None, :]
    kept = [k for k in range(n_s + 2) if k != idx]
    m = torch.cat((m, (a * ms)[:, None], (a * mc)[:, None]), dim=1)[:, kept]
    v = torch.cat((torch.cat((v, C), dim=2), torch.cat((C.transpose(1, 2), vt), dim=2)), dim=1)[:, kept][:, :, kept]
    d = m - z
    G = torch.eye(z.shape[0], dtype=m.dtype, device=m.device) + v @ W
    l = 1 - torch.exp(-torch.einsum("ni,nij,nj->n", d, W @ torch.linalg.inv(G), d) / 2) / torch.sqrt(torch.linalg.det(G))
    return l.reshape(T, H).sum(dim=1)


def model(N=150, n_s=4, n_u=1, seed=0):
    rng = np.random.default_rng(seed)
    D = n_s + n_u
    Z = rng.uniform(-1, 1, (N, D))
    Y = 0.2 * np.sin(2.0 * Z.dot(rng.standard_normal((D, n_s)) / np.sqrt(D))) + 0.01 * rng.standard_normal((N, n_s))
    hyp = [{"lengthscale": rng.uniform(0.6, 1.4, D) * np.sqrt(D / 3.0), "variance": 0.05, "noise_variance": 1e-2} for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    return gp


def main(T=16, H=15):
    n_s, n_u = 4, 1
    gp = model()
    dev = gp.device
    rng = np.random.default_rng(1)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
    mu_0 = t(0.3 * rng.standard_normal((T, n_s)))
    k_ff = t(0.2 * rng.standard_normal((T, H, n_u))).requires_grad_(True)
    k_fb = t(0.3 * rng.standard_normal((T, H - 1, n_u, n_s))).requires_grad_(True)
    a, b = 0.9 * np.eye(n_s), 0.1 * rng.standard_normal((n_s, n_u))
    z, W = t(Z_TARGET), t(W_TARGET)
    worst = 0.0
    for name in ("Taylor (mode 1)", "moment matching"):
        taylor = name.startswith("Taylor")
        # three library calls, no graph
        kff, kfb = k_ff.detach(), k_fb.detach()
        if taylor:
            mu_all, sigma_all, _ = prop.multistep_moments_batch(mu_0, gp, kff, kfb, a, b, prop.TAYLOR)
        else:
            mu_all, sigma_all, _ = prop.moment_matching_rollout_batch(mu_0, gp, kff, kfb, a, b)
        cost = utils_casadi.rollout_cost_batch(mu_all, sigma_all, Z_TARGET, W_TARGET, idx_angle=IDX_ANGLE)
        mu_bar, sigma_bar, _ = utils_casadi.rollout_cost_vjp_batch(mu_all, sigma_all, Z_TARGET, W_TARGET, idx_angle=IDX_ANGLE)
        if taylor:
            g = prop.multistep_moments_vjp_batch(mu_0, gp, kff, kfb, mu_all, sigma_all, mu_bar, sigma_bar, None, a, b, prop.TAYLOR)
        else:
            g = prop.moment_matching_rollout_vjp_batch(mu_0, gp, kff, kfb, mu_all, sigma_all, mu_bar, sigma_bar, None, a, b)
        lib_grads = (g[2].reshape(k_ff.shape), g[3].reshape(k_fb.shape))
        # the torch port behind the same roll-out as one autograd node
        if taylor:
            ma, sa, _ = prop.multistep_moments_diff_batch(mu_0, gp, k_ff, k_fb, a, b, prop.TAYLOR)
        else:
            ma, sa, _ = prop.moment_matching_rollout_diff_batch(mu_0, gp, k_ff, k_fb, a, b)
        port = torch_cost(ma, sa, z, W, IDX_ANGLE)
        port_grads = torch.autograd.grad(port.sum(), [k_ff, k_fb])
        print("%s roll-out, T = %d, H = %d: cost %.6f .. %.6f (device) against the torch port: %.1e" %
              (name, T, H, float(cost.min()), float(cost.max()), float((cost - port.detach()).abs().max())))
        for what, gl, gt in zip(("k_ff", "k_fb"), lib_grads, port_grads):
            dist = float((gl - gt).abs().max() / gt.abs().max())
            worst = max(worst, dist)
            print("  d/d%s: largest element %.6e (three calls) %.6e (torch port), distance %.2e" % (what, float(gl.abs().max()),
                                                                                                  float(gt.abs().max()), dist))
    print("distance of the two gradients, of the largest element: %.3e" % worst)


if __name__ == "__main__":
    main()
