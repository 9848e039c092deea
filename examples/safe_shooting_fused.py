"""The shooting loop of examples/safe_shooting_gradient.py on the fused gradient: a few Adam steps on the feed-forward controls
and feedback gains of a batch of roll-outs of the pendulum fixture (tests/golden/reach_pend.npz), against

    |p_H - target|^2  +  w sum_i sum_m relu(h_m . p_i + c sqrt(h_m^T q_i h_m) - h_vec_m)^2

    python examples/safe_shooting_fused.py

Needs a GPU.  The forward of every iteration is the plain one-launch roll-out (sr_multistep_reach), its backward ONE
sr_multistep_reach_vjp call (gp_reachability.multistep_reachability_diff_batch): a batched linearisation of the GP at the inputs
of all T * H steps, then the reverse sweep.  Prints the loss per iteration and, at the end, the time per gradient (forward +
backward of the loss) of this route and of the chained one (multistep_reachability_batch(differentiable=True): H one-step nodes)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from safe_exploration_amd import SimpleGPModel                                    # noqa: E402
from safe_exploration_amd import gp_reachability as reach                         # noqa: E402


def main(steps=8, reps=20):
    g = np.load(os.path.join(ROOT, "tests", "golden", "reach_pend.npz"))
    n_s, n_u = 2, 1
    hyp = [{"lengthscale": g["lengthscale"][d], "variance": float(g["signal_var"][d]),
            "noise_variance": float(g["noise_var"][d])} for d in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(g["Z"], g["Y"], opt_hyp=False)
    dev = gp.device
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
    H = 5
    p_0 = t(g["ms_p0"])
    k_ff = t(g["ms_k_ff"][:, :H]).requires_grad_(True)
    k_fb = t(g["ms_k_fb"][:, :H - 1]).requires_grad_(True)
    h_mat, h_vec, c = t(g["h_mat"]), t(g["h_vec"]).reshape(-1), float(g["c_safety"])
    target = torch.zeros(n_s, dtype=torch.float64, device=dev)

    def loss_of(kff, kfb, route):
        if route == "fused":
            p_all, q_all = reach.multistep_reachability_diff_batch(p_0, gp, kfb, kff, g["l_mu"], g["l_sigma"], None, c,
                                                                   g["a_lin"], g["b_lin"])
        else:
            p_all, q_all = reach.multistep_reachability_batch(p_0, gp, kfb, kff, g["l_mu"], g["l_sigma"], None, c, g["a_lin"],
                                                              g["b_lin"], differentiable=route == "chained")
        quad = torch.einsum('mi,thij,mj->thm', h_mat, q_all, h_mat)
        dist = torch.einsum('mi,thi->thm', h_mat, p_all) + c * torch.sqrt(quad) - h_vec
        return ((p_all[:, -1] - target) ** 2).sum() + 10.0 * (torch.relu(dist) ** 2).sum()

    opt = torch.optim.Adam([k_ff, k_fb], lr=0.02)
    for i in range(steps):
        opt.zero_grad()
        loss = loss_of(k_ff, k_fb, "fused")
        loss.backward()
        print("step %d loss %.8f" % (i, float(loss)))
        opt.step()
    with torch.no_grad():
        print("step %d loss %.8f" % (steps, float(loss_of(k_ff, k_fb, "plain"))))

    for route in ("fused", "chained"):
        times = []
        for r in range(reps + 3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            torch.autograd.grad(loss_of(k_ff, k_fb, route), [k_ff, k_fb])
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        print("%s route: %.3f ms per gradient (median of %d, T = %d, H = %d)"
              % (route, 1e3 * float(np.median(times[3:])), reps, p_0.shape[0], H))


if __name__ == "__main__":
    main()
