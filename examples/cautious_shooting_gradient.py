"""Cautious shooting through the Taylor-propagated moments: a few Adam steps on the feed-forward controls and feedback gains of a
batch of roll-outs of the pendulum fixture (tests/golden/reach_pend.npz), against a loss written in plain torch,

    |mu_H - target|^2  +  w sum_i sum_m relu(h_m . mu_i + k sqrt(h_m^T Sigma_i h_m) - h_vec_m)^2

the terminal distance of the mean trajectory plus a hinge on the chance constraint of every step, h x <= h_vec with the
k-sigma back-off of the CautiousMPC baseline (the performance trajectory of SafeMPC is propagated the same way).

    python examples/cautious_shooting_gradient.py

Needs a GPU: every step of the roll-out is sr_onestep_moments, its backward sr_onestep_moments_vjp (the GP derivatives at the
step's input and the reverse of the moment algebra in one launch); torch autograd chains the steps and differentiates the loss."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from safe_exploration_amd import SimpleGPModel                                    # noqa: E402
from safe_exploration_amd import uncertainty_propagation_casadi as prop           # noqa: E402


def main(steps=8):
    g = np.load(os.path.join(ROOT, "tests", "golden", "reach_pend.npz"))
    n_s, n_u = 2, 1
    hyp = [{"lengthscale": g["lengthscale"][d], "variance": float(g["signal_var"][d]),
            "noise_variance": float(g["noise_var"][d])} for d in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(g["Z"], g["Y"], opt_hyp=False)
    dev = gp.device
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
    H = 5
    mu_0 = t(g["ms_p0"])
    k_ff = t(g["ms_k_ff"][:, :H]).requires_grad_(True)
    k_fb = t(g["ms_k_fb"][:, :H - 1]).requires_grad_(True)
    h_mat, h_vec, k = t(g["h_mat"]), t(g["h_vec"]).reshape(-1), 2.0
    target = torch.zeros(n_s, dtype=torch.float64, device=dev)

    def loss_of(kff, kfb, differentiable):
        mu_all, sigma_all, _ = prop.multistep_moments_batch(mu_0, gp, kff, kfb, g["a_lin"], g["b_lin"], prop.TAYLOR,
                                                            differentiable=differentiable)
        quad = torch.einsum('mi,thij,mj->thm', h_mat, sigma_all, h_mat)
        dist = torch.einsum('mi,thi->thm', h_mat, mu_all) + k * torch.sqrt(quad) - h_vec
        return ((mu_all[:, -1] - target) ** 2).sum() + 10.0 * (torch.relu(dist) ** 2).sum()

    opt = torch.optim.Adam([k_ff, k_fb], lr=0.02)
    for i in range(steps):
        opt.zero_grad()
        loss = loss_of(k_ff, k_fb, True)
        loss.backward()
        print("step %d loss %.8f" % (i, float(loss)))
        opt.step()
    with torch.no_grad():
        print("step %d loss %.8f" % (steps, float(loss_of(k_ff, k_fb, False))))


if __name__ == "__main__":
    main()
