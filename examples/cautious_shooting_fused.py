"""The gradient of the objective of examples/cautious_shooting_gradient.py computed both ways: through the Taylor-propagated moments
of a batch of roll-outs of the pendulum fixture (tests/golden/reach_pend.npz),

    |mu_H - target|^2  +  w sum_i sum_m relu(h_m . mu_i + k sqrt(h_m^T Sigma_i h_m) - h_vec_m)^2

in the feed-forward controls and the feedback gains.

    python examples/cautious_shooting_fused.py

Needs a GPU.  The fused route: the plain one-launch roll-out (sr_multistep_moments) and ONE sr_multistep_moments_vjp call behind
it (uncertainty_propagation_casadi.multistep_moments_diff_batch): the GP derivatives at the inputs of all T * H steps in one pass,
then the reverse sweep.  The chained route: multistep_moments_batch(differentiable=True), H one-step nodes, each with a GP pass of
its own.  Prints the distance of the two gradients (of the largest element of the chained one) and the time per gradient (forward +
backward of the loss) of either route."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from safe_exploration_amd import SimpleGPModel                                    # noqa: E402
from safe_exploration_amd import uncertainty_propagation_casadi as prop           # noqa: E402


def main(reps=20):
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

    def loss_of(kff, kfb, route):
        if route == "fused":
            mu_all, sigma_all, _ = prop.multistep_moments_diff_batch(mu_0, gp, kff, kfb, g["a_lin"], g["b_lin"], prop.TAYLOR)
        else:
            mu_all, sigma_all, _ = prop.multistep_moments_batch(mu_0, gp, kff, kfb, g["a_lin"], g["b_lin"], prop.TAYLOR,
                                                                differentiable=True)
        quad = torch.einsum('mi,thij,mj->thm', h_mat, sigma_all, h_mat)
        dist = torch.einsum('mi,thi->thm', h_mat, mu_all) + k * torch.sqrt(quad) - h_vec
        return ((mu_all[:, -1] - target) ** 2).sum() + 10.0 * (torch.relu(dist) ** 2).sum()

    grads = {route: torch.autograd.grad(loss_of(k_ff, k_fb, route), [k_ff, k_fb]) for route in ("fused", "chained")}
    for name, gf, gc in zip(("k_ff", "k_fb"), grads["fused"], grads["chained"]):
        print("d/d%s: largest element %.6e (fused) %.6e (chained)" % (name, float(gf.abs().max()), float(gc.abs().max())))
    dist = max(float((gf - gc).abs().max() / gc.abs().max()) for gf, gc in zip(grads["fused"], grads["chained"]))
    for route in ("fused", "chained"):
        times = []
        for r in range(reps + 3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            torch.autograd.grad(loss_of(k_ff, k_fb, route), [k_ff, k_fb])
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        print("%s route: %.3f ms per gradient (median of %d, T = %d, H = %d)"
              % (route, 1e3 * float(np.median(times[3:])), reps, mu_0.shape[0], H))
    print("distance of the two gradients, of the largest element: %.3e" % dist)


if __name__ == "__main__":
    main()
