"""Time per gradient of a reachability roll-out: the fused route (the plain one-launch forward + ONE sr_multistep_reach_vjp call,
gp_reachability.multistep_reachability_diff_batch) against the chained route (multistep_reachability_batch(differentiable=True) +
torch.autograd.grad: H one-step forwards and H sr_onestep_reach_vjp nodes), in the same run, with the plain forward beside them and
the split of the new call into its linearisation pass and its sweep.

    python scripts/bench_reach_rollout_vjp.py [OUT]        (default OUT: profiles/r22_reach_rollout_vjp.txt)

Times: host clock around synchronised batches of calls on device tensors, after a warm-up; the median of seven batches with the
fastest and the slowest batch beside it.  The split: the handle's event profile (sr_prof_get) of one profiled run of the reverse call --
SR_K_REACH_VJP is the sweep, every other id the linearisation pass -- and the time of linearize_device_batch alone on the same
T * H inputs."""
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
from safe_exploration_amd import gp_reachability as reach                          # noqa: E402
from safe_exploration_amd._lib import K_GRAM                                       # noqa: E402

K_REACH_VJP, K_COUNT = 14, 15


def batches(fn, per, warmup=5, n_batches=7):
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
    return "%9.1f us [%8.1f .. %8.1f]" % x


def regime(out, name, N, n_s, n_u, T, H=15, per=20):
    gp = model(N, n_s, n_u)
    dev = gp.device
    rng = np.random.default_rng(1)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    p0 = t(0.3 * rng.standard_normal((T, n_s)))
    kff = t(0.2 * rng.standard_normal((T, H, n_u))).requires_grad_(True)
    kfb = t(0.3 * rng.standard_normal((T, H - 1, n_u, n_s))).requires_grad_(True)
    wp, wq = t(rng.standard_normal((T, H, n_s))), t(rng.standard_normal((T, H, n_s, n_s)))
    a_np, b_np = 0.9 * np.eye(n_s), 0.1 * rng.standard_normal((n_s, n_u))
    l_np, c = np.full(n_s, 0.03), 1.7

    def plain():
        return reach.multistep_reachability_batch(p0, gp, kfb.detach(), kff.detach(), l_np, l_np, None, c, a_np, b_np)

    def fused():
        pa, qa = reach.multistep_reachability_diff_batch(p0, gp, kfb, kff, l_np, l_np, None, c, a_np, b_np)
        return torch.autograd.grad((pa * wp).sum() + (qa * wq).sum(), (kff, kfb))

    def chained():
        pa, qa = reach.multistep_reachability_batch(p0, gp, kfb, kff, l_np, l_np, None, c, a_np, b_np, differentiable=True)
        return torch.autograd.grad((pa * wp).sum() + (qa * wq).sum(), (kff, kfb))

    pa, qa = plain()

    def reverse_only():
        return reach.multistep_reachability_vjp_batch(p0, gp, kfb.detach(), kff.detach(), l_np, l_np, pa, qa, wp, wq, None, c,
                                                      a_np, b_np)

    z = torch.cat((torch.cat((p0[:, None], pa[:, :-1]), dim=1), kff.detach()), dim=2).reshape(T * H, n_s + n_u).contiguous()
    t_plain, t_fused, t_chain = batches(plain, per), batches(fused, per), batches(chained, max(3, per // 4))
    t_rev, t_lin = batches(reverse_only, per), batches(lambda: gp.linearize_device_batch(z), per)
    gf, gc = fused(), chained()
    agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(gf, gc))
    # the event profile of the reverse call alone
    reverse_only()
    torch.cuda.synchronize()
    gp.prof_enable(True)
    gp.prof_reset()
    reps = 5
    for _ in range(reps):
        reverse_only()
    torch.cuda.synchronize()
    prof = [gp.prof_get(k)[0] * 1e3 / reps for k in range(K_GRAM, K_COUNT)]
    gp.prof_enable(False)
    sweep, lin = prof[K_REACH_VJP], sum(prof) - prof[K_REACH_VJP]
    out.append("  %s, H = %d" % (name, H))
    out.append("    plain forward (one launch)            %s" % fmt(t_plain))
    out.append("    fused gradient  (forward + backward)  %s   %.2f x the forward" % (fmt(t_fused), t_fused[0] / t_plain[0]))
    out.append("    chained gradient (forward + backward) %s   %.2f x the fused gradient" % (fmt(t_chain), t_chain[0] / t_fused[0]))
    out.append("    sr_multistep_reach_vjp alone          %s   linearize_device_batch alone on its %d inputs %s"
               % (fmt(t_rev), T * H, fmt(t_lin)))
    out.append("    its kernels (event profile, per call): linearisation pass %8.1f us, sweep %8.1f us (%.0f %% of the two)"
               % (lin, sweep, 100 * sweep / max(lin + sweep, 1e-9)))
    out.append("    fused against chained gradient: %.1e of the largest element" % agree)
    out.append("")
    return t_chain[0] / t_fused[0]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r22_reach_rollout_vjp.txt")
    out = ["Gradient of an H = 15 reachability roll-out in its controls -- time per gradient, 1 x MI355X",
           "(scripts/bench_reach_rollout_vjp.py; median [fastest .. slowest] of seven synchronised batches, host clock, device tensors)",
           ""]
    for T in (1, 16, 256, 3840):
        regime(out, "cart-pole regime N=150 n_s=4 n_u=1 T=%d" % T, 150, 4, 1, T, per=20 if T < 3840 else 8)
    for T in (1, 16, 256, 3840):
        regime(out, "pendulum regime N=200 n_s=2 n_u=1 T=%d" % T, 200, 2, 1, T, per=20 if T < 3840 else 8)
    regime(out, "N=5000 n_s=2 n_u=1 T=256", 5000, 2, 1, 256, per=6)
    out.append("In neither figure of the split: the input and the eigenpair launch (parallel over the T * H queries, a few us each).")
    text = "\n".join(out) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
