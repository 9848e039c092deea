"""Time of the MPC objective and its seeds: the device cost (utils_casadi.rollout_cost_batch + rollout_cost_vjp_batch, one launch
each) against the same cost written in batched torch fp64 and differentiated by autograd (examples/cautious_shooting_cost.torch_cost:
linalg.inv, det, cat, index selection), in the same run; then the same pair inside a whole gradient in k_ff, k_fb behind
uncertainty_propagation_casadi.multistep_moments_diff_batch (Taylor roll-out, one autograd node).

    python scripts/bench_rollout_cost.py [OUT]        (default OUT: profiles/r25_rollout_cost.txt)

Cart-pole regime: n_s = 4, n_u = 1, idx_angle = 2, z = [2.5, 0, 0, 0, 0.5], W = diag(20, 0, 0, 0, 5) / 100, H = 15, N = 150;
T = 1, 16, 256, 3840.  Times: host clock around synchronised batches of calls on device tensors, after a warm-up; the median of seven
batches with the fastest and the slowest batch beside it.  The two routes are timed alternately, batch by batch."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

from cautious_shooting_cost import torch_cost, model, IDX_ANGLE, Z_TARGET, W_TARGET    # noqa: E402
from safe_exploration_amd import utils_casadi as uc                                  # noqa: E402
from safe_exploration_amd import uncertainty_propagation_casadi as prop              # noqa: E402


def alternating(fns, per, warmup=5, n_batches=7):
    """us per call of each function: (median, fastest, slowest) of n_batches batches of `per` calls, the functions taking turns"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    res = [[] for _ in fns]
    for _ in range(n_batches):
        for k, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per):
                fn()
            torch.cuda.synchronize()
            res[k].append((time.perf_counter() - t0) / per * 1e6)
    return [(statistics.median(r), min(r), max(r)) for r in res]


def fmt(x):
    return "%9.1f us [%8.1f .. %8.1f]" % x


def regime(out, gp, T, H=15, per=20):
    n_s, n_u = 4, 1
    dev = gp.device
    rng = np.random.default_rng(1)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
    mu_0 = t(0.3 * rng.standard_normal((T, n_s)))
    k_ff = t(0.2 * rng.standard_normal((T, H, n_u))).requires_grad_(True)
    k_fb = t(0.3 * rng.standard_normal((T, H - 1, n_u, n_s))).requires_grad_(True)
    a, b = 0.9 * np.eye(n_s), 0.1 * rng.standard_normal((n_s, n_u))
    z, W = t(Z_TARGET), t(W_TARGET)
    mu_all, sigma_all, _ = prop.multistep_moments_batch(mu_0, gp, k_ff.detach(), k_fb.detach(), a, b, prop.TAYLOR)
    kw = dict(z=Z_TARGET, W=W_TARGET, idx_angle=IDX_ANGLE)

    def dev_forward():
        return uc.rollout_cost_batch(mu_all, sigma_all, **kw)

    def dev_seeds():
        return uc.rollout_cost_batch(mu_all, sigma_all, **kw), uc.rollout_cost_vjp_batch(mu_all, sigma_all, **kw)

    def port_forward():
        return torch_cost(mu_all, sigma_all, z, W, IDX_ANGLE)

    def port_seeds():
        m, s = mu_all.detach().requires_grad_(True), sigma_all.detach().requires_grad_(True)
        c = torch_cost(m, s, z, W, IDX_ANGLE)
        return c, torch.autograd.grad(c.sum(), [m, s])

    def roll():
        ma, sa, _ = prop.multistep_moments_diff_batch(mu_0, gp, k_ff, k_fb, a, b, prop.TAYLOR)
        return ma, sa

    def grad_dev():
        ma, sa = roll()
        return torch.autograd.grad(uc.rollout_cost_batch(ma, sa, differentiable=True, **kw).sum(), [k_ff, k_fb])

    def grad_port():
        ma, sa = roll()
        return torch.autograd.grad(torch_cost(ma, sa, z, W, IDX_ANGLE).sum(), [k_ff, k_fb])

    def grad_plain():                                       # the roll-out's gradient with a linear functional: no cost at all
        ma, sa = roll()
        return torch.autograd.grad(ma.sum() + sa.sum(), [k_ff, k_fb])

    (c_dev, g_dev), (c_port, g_port) = dev_seeds(), port_seeds()
    agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(g_dev[:2], g_port))
    whole = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(grad_dev(), grad_port()))
    t_df, t_pf = alternating((dev_forward, port_forward), per)
    t_ds, t_ps = alternating((dev_seeds, port_seeds), per)
    t_gd, t_gp, t_g0 = alternating((grad_dev, grad_port, grad_plain), max(3, per // 2))
    out.append("  T = %d, H = %d" % (T, H))
    out.append("    cost alone          device (1 launch)  %s   torch port %s   %.2f x" % (fmt(t_df), fmt(t_pf), t_pf[0] / t_df[0]))
    out.append("    cost + seeds        device (2 launches)%s   torch port %s   %.2f x" % (fmt(t_ds), fmt(t_ps), t_ps[0] / t_ds[0]))
    out.append("    whole gradient      device cost        %s   torch port %s   %.2f x" % (fmt(t_gd), fmt(t_gp), t_gp[0] / t_gd[0]))
    out.append("    the roll-out's gradient with a linear functional in place of the cost  %s" % fmt(t_g0))
    out.append("    seeds, device against port: %.1e of the largest element; whole gradient: %.1e" % (agree, whole))
    out.append("")


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r25_rollout_cost.txt")
    out = ["The cart-pole objective (trig_aug + loss_sat over H = 15 stored states) and its gradient -- time per call, 1 x MI355X",
           "(scripts/bench_rollout_cost.py; median [fastest .. slowest] of seven synchronised batches, host clock, device tensors; the",
           "routes of a row are timed alternately, batch by batch; the ratio is torch port / device)", ""]
    gp = model()
    for T in (1, 16, 256, 3840):
        regime(out, gp, T, per=20 if T < 3840 else 8)
    text = "\n".join(out) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
