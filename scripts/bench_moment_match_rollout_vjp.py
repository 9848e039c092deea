"""Time per gradient of an exact moment-matching roll-out in its controls: ONE autograd node for the whole roll-out
(uncertainty_propagation_casadi.moment_matching_rollout_diff_batch: the plain forward + one sr_gp_moment_match_rollout_vjp call)
against the chained route (moment_matching_batch(differentiable=True) + torch.autograd.grad: H forwards and H
sr_gp_moment_match_vjp nodes with batched-torch glue between them), in the same run, with the plain forward beside them.

    python scripts/bench_moment_match_rollout_vjp.py [OUT]        (default OUT: profiles/r23_moment_match_rollout_vjp.txt)
    python scripts/bench_moment_match_rollout_vjp.py --one-call N n_s n_u T
                                                                  (a warm-up and three reverse calls, for a kernel trace)

Times: host clock around synchronised batches of calls on device tensors, after a warm-up; the median of the batches with the
fastest and the slowest batch beside it."""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from reach_grad_bench import model                                                 # noqa: E402
from safe_exploration_amd import uncertainty_propagation_casadi as up              # noqa: E402


def batches(fn, per, warmup=2, n_batches=5):
    """us per call: (median, fastest, slowest) of n_batches batches of `per` calls"""
    for _ in range(warmup):
        fn()
    res = []
    for _ in range(n_batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(per):
            fn()
        torch.cuda.synchronize()
        res.append((time.perf_counter() - t0) / per * 1e6)
    return statistics.median(res), min(res), max(res)


def fmt(x):
    return "%11.1f us [%10.1f .. %10.1f]" % x


def setup(N, n_s, n_u, T, H):
    gp = model(N, n_s, n_u)
    dev = gp.device
    rng = np.random.default_rng(1)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    mu0 = t(0.3 * rng.standard_normal((T, n_s)))
    L = 0.1 * rng.standard_normal((T, n_s, n_s))
    s0 = t(np.matmul(L, np.transpose(L, (0, 2, 1))))
    kff = t(0.2 * rng.standard_normal((T, H, n_u))).requires_grad_(True)
    kfb = t(0.3 * rng.standard_normal((T, H - 1, n_u, n_s))).requires_grad_(True)
    w = t(rng.standard_normal((T, H, n_s))), t(rng.standard_normal((T, H, n_s, n_s)))
    a, b = 0.9 * np.eye(n_s), 0.1 * rng.standard_normal((n_s, n_u))
    return gp, mu0, s0, kff, kfb, w, a, b


def regime(out, name, N, n_s, n_u, T, H=15, per=10, n_batches=5):
    gp, mu0, s0, kff, kfb, (wm, ws), a, b = setup(N, n_s, n_u, T, H)

    def plain():
        return up.moment_matching_rollout_batch(mu0, gp, kff.detach(), kfb.detach(), a, b, s0)

    def fused():
        mu_all, sigma_all, _ = up.moment_matching_rollout_diff_batch(mu0, gp, kff, kfb, a, b, s0)
        return torch.autograd.grad((mu_all * wm).sum() + (sigma_all * ws).sum(), (kff, kfb))

    def chained():
        mu_all, sigma_all, _ = up.moment_matching_batch(mu0, gp, kff, kfb, a, b, s0, differentiable=True)
        return torch.autograd.grad((mu_all * wm).sum() + (sigma_all * ws).sum(), (kff, kfb))

    mu_all, sigma_all, _ = plain()

    def reverse_only():
        return up.moment_matching_rollout_vjp_batch(mu0, gp, kff.detach(), kfb.detach(), mu_all, sigma_all, wm, ws, None, a, b, s0)

    t_plain, t_fused = batches(plain, per, n_batches=n_batches), batches(fused, per, n_batches=n_batches)
    t_chain, t_rev = batches(chained, max(2, per // 2), n_batches=n_batches), batches(reverse_only, per, n_batches=n_batches)
    gf, gc = fused(), chained()
    agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(gf, gc))
    fwd = "one launch" if gp.moment_match_rollout_supported() else "per step: N > 1024"
    out.append("  %s, H = %d" % (name, H))
    out.append("    plain forward (%s)%s %s" % (fwd, " " * (26 - len(fwd)), fmt(t_plain)))
    out.append("    one-node gradient (forward + backward)      %s   %.2f x the forward" % (fmt(t_fused), t_fused[0] / t_plain[0]))
    out.append("    chained gradient  (forward + backward)      %s   %.2f x the one-node gradient" % (fmt(t_chain),
                                                                                                      t_chain[0] / t_fused[0]))
    out.append("    sr_gp_moment_match_rollout_vjp alone        %s" % fmt(t_rev))
    out.append("    one-node against chained gradient: %.1e of the largest element" % agree)
    out.append("")
    return t_chain[0] / t_fused[0]


def one_call(N, n_s, n_u, T, H=15):
    gp, mu0, s0, kff, kfb, (wm, ws), a, b = setup(N, n_s, n_u, T, H)
    mu_all, sigma_all, _ = up.moment_matching_rollout_batch(mu0, gp, kff.detach(), kfb.detach(), a, b, s0)
    for _ in range(4):
        up.moment_matching_rollout_vjp_batch(mu0, gp, kff.detach(), kfb.detach(), mu_all, sigma_all, wm, ws, None, a, b, s0)
    torch.cuda.synchronize()


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--one-call":
        return one_call(*[int(x) for x in sys.argv[2:6]])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r23_moment_match_rollout_vjp.txt")
    out = ["Gradient of an H = 15 exact moment-matching roll-out in its controls -- time per gradient, 1 x MI355X",
           "(scripts/bench_moment_match_rollout_vjp.py; median [fastest .. slowest] of five synchronised batches, host clock, device "
           "tensors)", ""]
    for T in (1, 16, 256, 3840):
        regime(out, "cart-pole regime N=150 n_out=4 D=5 T=%d" % T, 150, 4, 1, T, per=10 if T < 3840 else 2,
               n_batches=5 if T < 3840 else 3)
    for T in (1, 64):
        regime(out, "N=1000 n_out=2 D=3 T=%d" % T, 1000, 2, 1, T, per=4)
    regime(out, "N=5000 n_out=2 D=3 T=16", 5000, 2, 1, 16, per=1, n_batches=3)
    text = "\n".join(out) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
