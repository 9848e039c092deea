"""The shooting loop of examples/safe_shooting_fused.py on the real SafeMPC constraint set: a few Adam steps on the feed-forward
controls and feedback gains of a batch of roll-outs of the pendulum fixture (tests/golden/reach_pend.npz) against

    |p_H - target|^2  +  sum_rows (max(0, lam + rho g)^2 - lam^2) / (2 rho)

the Powell-Hestenes-Rockafellar augmented Lagrangian of the rows g <= 0 of SimpleSafeMPC.generate_safety_constraints: control
bounds on the ellipsoid of controls, the fixture's h_mat as obstacle set on every intermediate ellipsoid and (tighter) as terminal
set on the last one, with a multiplier update lam <- max(0, lam + rho g) after every step.

    python examples/safe_shooting_constrained.py

Needs a GPU.  The gradient of the Lagrangian term in k_ff, k_fb is computed both ways and printed with the largest difference:
  raw      three library calls: the roll-out (sr_multistep_reach), the constraints' reverse pass (sr_rollout_constraints_vjp) with
           the seed max(0, lam + rho g), the roll-out's reverse pass (sr_multistep_reach_vjp) with the seeds the second call
           returned -- plus the direct terms kff_bar, kfb_bar of the second call: the control rows read the gains themselves;
  autograd torch autograd through the rows written as einsums, sqrt and relu on multistep_reachability_diff_batch.
At the end the time per gradient of both."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from safe_exploration_amd import SimpleGPModel                                    # noqa: E402
from safe_exploration_amd import gp_reachability as reach                         # noqa: E402


def torch_constraints(p_all, q_all, k_ff, k_fb, ctrl_bounds, h_obs_mat, h_obs, h_safe_mat, h_safe, c):
    """The rows of rollout_constraints_batch (point start) in batched torch: einsum, sqrt, cat -- what a caller wrote before the
    library had them.  ctrl_bounds (n_u, 2), h_* tensors."""
    T, H, _ = p_all.shape
    q = (q_all + q_all.transpose(2, 3)) / 2
    r = c * torch.sqrt(torch.einsum("thja,thab,thjb->thj", k_fb, q[:, :-1], k_fb))
    r = torch.cat((torch.zeros_like(k_ff[:, :1]), r), dim=1)
    blocks = [torch.cat((k_ff + r - ctrl_bounds[:, 1], ctrl_bounds[:, 0] - k_ff + r), dim=2).reshape(T, -1)]
    for hm, hv, sl in ((h_obs_mat, h_obs, slice(0, H - 1)), (h_safe_mat, h_safe, slice(H - 1, H))):
        quad = torch.einsum("mi,thij,mj->thm", hm, q[:, sl], hm)
        blocks.append((torch.einsum("mi,thi->thm", hm, p_all[:, sl]) + c * torch.sqrt(quad) - hv).reshape(T, -1))
    return torch.cat(blocks, dim=1)


def lagrangian(g, lam, rho):
    return ((torch.relu(lam + rho * g) ** 2 - lam ** 2) / (2 * rho)).sum()


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
    T = p_0.shape[0]
    k_ff = t(g["ms_k_ff"][:, :H]).requires_grad_(True)
    k_fb = t(g["ms_k_fb"][:, :H - 1]).requires_grad_(True)
    c = float(g["c_safety"])
    bounds = np.array([[-0.15, 0.15]])
    h_mat, h_obs, h_safe = g["h_mat"], 0.25 * g["h_vec"].reshape(-1), 0.1 * g["h_vec"].reshape(-1)
    sets = (bounds, h_mat, h_obs, h_mat, h_safe, None, None, c)
    sets_t = (t(bounds), t(h_mat), t(h_obs), t(h_mat), t(h_safe), c)
    blocks, names = reach.rollout_constraint_layout(H, n_u, h_mat.shape[0], h_mat.shape[0], True)
    rho = 10.0
    lam = torch.zeros((T, len(names)), dtype=torch.float64, device=dev)
    target = torch.zeros(n_s, dtype=torch.float64, device=dev)
    roll_args = (g["l_mu"], g["l_sigma"], None, c, g["a_lin"], g["b_lin"])

    def grad_raw(kff, kfb):
        """the Lagrangian term's gradient in three calls (no autograd graph), and the rows"""
        kff, kfb = kff.detach(), kfb.detach()
        p_all, q_all = reach.multistep_reachability_batch(p_0, gp, kfb, kff, *roll_args)
        rows, worst = reach.rollout_constraints_batch(p_all, q_all, kff, kfb, *sets, return_max=True)
        pb, qb, kffb, kfbb, _, _ = reach.rollout_constraints_vjp_batch(p_all, q_all, kff, kfb, *sets, g_bar=torch.relu(lam + rho * rows))
        out = reach.multistep_reachability_vjp_batch(p_0, gp, kfb, kff, g["l_mu"], g["l_sigma"], p_all, q_all, pb, qb, None, c,
                                                     g["a_lin"], g["b_lin"])
        return out[3] + kffb, out[4].reshape(kfb.shape) + kfbb, rows, worst

    def grad_autograd(kff, kfb):
        p_all, q_all = reach.multistep_reachability_diff_batch(p_0, gp, kfb, kff, *roll_args)
        return torch.autograd.grad(lagrangian(torch_constraints(p_all, q_all, kff, kfb, *sets_t), lam, rho), [kff, kfb])

    def loss_of(kff, kfb):
        p_all, q_all = reach.multistep_reachability_diff_batch(p_0, gp, kfb, kff, *roll_args)
        rows = reach.rollout_constraints_batch(p_all, q_all, kff, kfb, *sets, differentiable=True)
        return ((p_all[:, -1] - target) ** 2).sum() + lagrangian(rows, lam, rho), rows.detach()

    opt = torch.optim.Adam([k_ff, k_fb], lr=0.02)
    for i in range(steps):
        opt.zero_grad()
        loss, rows = loss_of(k_ff, k_fb)
        loss.backward()
        viol = {k: float(rows[:, s].max()) for k, s in blocks.items()}
        print("step %d loss %.8f  largest row: control %+.4f obstacle %+.4f terminal %+.4f  feasible candidates %d / %d"
              % (i, float(loss), viol["control"], viol["obstacle"], viol["terminal"], int((rows.max(dim=1).values <= 0).sum()), T))
        opt.step()
        lam = torch.relu(lam + rho * rows)

    raw, auto = grad_raw(k_ff, k_fb), grad_autograd(k_ff, k_fb)
    worst_row = int(raw[2][0].argmax())
    print("the largest row of candidate 0 is %s (%+.4f); g_max per candidate: %s"
          % (names[worst_row], float(raw[2][0, worst_row]), np.array2string(raw[3].cpu().numpy(), precision=4)))
    for name, u, v in (("k_ff", raw[0], auto[0]), ("k_fb", raw[1], auto[1])):
        print("d Lagrangian / d %s, candidate 0, three raw calls: %s" % (name, np.array2string(u[0].reshape(-1).cpu().numpy(), precision=6)))
        print("d Lagrangian / d %s, candidate 0, torch autograd:  %s" % (name, np.array2string(v[0].reshape(-1).cpu().numpy(), precision=6)))
        print("largest difference over the batch: %.3e (largest element %.3e)" % (float((u - v).abs().max()), float(v.abs().max())))

    for name, fn in (("three raw calls", grad_raw), ("torch autograd through the einsum form", grad_autograd)):
        times = []
        for r in range(reps + 3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn(k_ff, k_fb)
            torch.cuda.synchronize(dev)
            times.append(time.perf_counter() - t0)
        print("%s: %.3f ms per gradient (median of %d, T = %d, H = %d)" % (name, 1e3 * float(np.median(times[3:])), reps, T, H))


if __name__ == "__main__":
    main()
