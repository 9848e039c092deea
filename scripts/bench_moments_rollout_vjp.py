"""Time per gradient of a Taylor / mean-equivalent roll-out from a point: the fused route (the plain one-launch forward + ONE
sr_multistep_moments_vjp call, uncertainty_propagation_casadi.multistep_moments_diff_batch) against the chained route
(multistep_moments_batch(differentiable=True) + torch.autograd.grad: H one-step forwards and H sr_onestep_moments_vjp nodes), in the
same run, with the plain forward beside them and the split of the new call into its GP pass and its sweep.

    python scripts/bench_moments_rollout_vjp.py [OUT]        (default OUT: profiles/r24_moments_rollout_vjp.txt)

Times: host clock around synchronised batches of calls on device tensors, after a warm-up; the median of seven batches with the
fastest and the slowest batch beside it.  The split: the handle's event profile (sr_prof_get) of one profiled run of the reverse call --
SR_K_REACH_VJP is the sweep, every other id the GP pass (sr_gp_linearize_batch in mode 1, sr_gp_predict_grad in mode 2)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_reach_rollout_vjp import batches, fmt, K_REACH_VJP, K_COUNT              # noqa: E402
from reach_grad_bench import model                                                 # noqa: E402
from safe_exploration_amd import uncertainty_propagation_casadi as prop            # noqa: E402
from safe_exploration_amd._lib import K_GRAM                                       # noqa: E402

_MODELS = {}


def regime(out, name, N, n_s, n_u, T, mode, H=15, per=20):
    if (N, n_s, n_u) not in _MODELS:
        _MODELS[(N, n_s, n_u)] = model(N, n_s, n_u)
    gp = _MODELS[(N, n_s, n_u)]
    dev = gp.device
    rng = np.random.default_rng(1)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    m0 = t(0.3 * rng.standard_normal((T, n_s)))
    kff = t(0.2 * rng.standard_normal((T, H, n_u))).requires_grad_(True)
    kfb = t(0.3 * rng.standard_normal((T, H - 1, n_u, n_s))).requires_grad_(True)
    wm, ws = t(rng.standard_normal((T, H, n_s))), t(rng.standard_normal((T, H, n_s, n_s)))
    a_np, b_np = 0.9 * np.eye(n_s), 0.1 * rng.standard_normal((n_s, n_u))

    def plain():
        return prop.multistep_moments_batch(m0, gp, kff.detach(), kfb.detach(), a_np, b_np, mode)

    def fused():
        ma, sa, _ = prop.multistep_moments_diff_batch(m0, gp, kff, kfb, a_np, b_np, mode)
        return torch.autograd.grad((ma * wm).sum() + (sa * ws).sum(), (kff, kfb))

    def chained():
        ma, sa, _ = prop.multistep_moments_batch(m0, gp, kff, kfb, a_np, b_np, mode, differentiable=True)
        return torch.autograd.grad((ma * wm).sum() + (sa * ws).sum(), (kff, kfb))

    ma, sa, _ = plain()

    def reverse_only():
        return prop.multistep_moments_vjp_batch(m0, gp, kff.detach(), kfb.detach(), ma, sa, wm, ws, None, a_np, b_np, mode)

    t_plain, t_fused, t_chain = batches(plain, per), batches(fused, per), batches(chained, max(3, per // 4))
    t_rev = batches(reverse_only, per)
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
    out.append("  %s, mode %d, H = %d" % (name, mode, H))
    out.append("    plain forward (one launch)            %s" % fmt(t_plain))
    out.append("    fused gradient  (forward + backward)  %s   %.2f x the forward" % (fmt(t_fused), t_fused[0] / t_plain[0]))
    out.append("    chained gradient (forward + backward) %s   %.2f x the fused gradient" % (fmt(t_chain), t_chain[0] / t_fused[0]))
    out.append("    sr_multistep_moments_vjp alone        %s" % fmt(t_rev))
    out.append("    its kernels (event profile, per call): GP pass %8.1f us, sweep %8.1f us (%.0f %% of the two)"
               % (lin, sweep, 100 * sweep / max(lin + sweep, 1e-9)))
    out.append("    fused against chained gradient: %.1e of the largest element" % agree)
    out.append("")
    return t_chain[0] / t_fused[0]


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r24_moments_rollout_vjp.txt")
    out = ["Gradient of an H = 15 Taylor (mode 1) / mean-equivalent (mode 2) roll-out from a point in its controls -- time per gradient,",
           "1 x MI355X (scripts/bench_moments_rollout_vjp.py; median [fastest .. slowest] of seven synchronised batches, host clock,",
           "device tensors)", ""]
    for mode in (1, 2):
        for T in (1, 16, 256, 3840):
            regime(out, "cart-pole regime N=150 n_s=4 n_u=1 T=%d" % T, 150, 4, 1, T, mode, per=20 if T < 3840 else 8)
        for T in (1, 16, 256, 3840):
            regime(out, "pendulum regime N=200 n_s=2 n_u=1 T=%d" % T, 200, 2, 1, T, mode, per=20 if T < 3840 else 8)
        regime(out, "N=5000 n_s=2 n_u=1 T=256", 5000, 2, 1, 256, mode, per=6)
    out.append("In neither figure of the split: the input launch (parallel over the T * H queries, a few us).")
    text = "\n".join(out) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
