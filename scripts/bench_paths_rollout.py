"""The fused closed-loop roll-out (sr_gp_paths_rollout: MonteCarloSafetyVerification.rollout_paths) beside the chained route
it stands next to (sample_n_step(consistent=True) / sample_n_step_jacobians: one paths_step_device call per step plus the
torch glue), both in THIS process on the SAME drawn paths, tensors in and out; and one paths_step_device call for the per-step
comparison.  Milliseconds per call from torch events around --reps calls after a warm-up call, device-synchronised, measured
--rounds times: the median, and the spread (max - min) / median of those repeats beside it.

    python scripts/bench_paths_rollout.py [--H 15] [--reps 5] [--rounds 7] [--regime cartpole|big|both]

Regimes (README): cartpole N = 150, n_out = 4, D = 5, S = M = 1024; big N = 5000, n_out = 2, D = 3, S = 1024, M = 2048.
In the LAB build (SAFEREACH_LIB) SR_ROLLOUT_PATHS = 4 / 8 / 16 selects the paths per workgroup; the product has one."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

REGIMES = {"cartpole": (150, 4, 5, 1024, 1024), "big": (5000, 2, 3, 1024, 2048)}


def ev_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds_ms(fn, reps, rounds):
    v = sorted(ev_ms(fn, reps) for _ in range(rounds))
    med = v[len(v) // 2]
    return med, (v[-1] - v[0]) / med


def run(name, H, reps, rounds):
    from safe_exploration_amd import SimpleGPModel
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    N, n_out, D, S, M = REGIMES[name]
    n_u = D - n_out
    rng = np.random.default_rng(1)
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    ls = rng.uniform(0.5, 1.0, (n_out, D)) * np.sqrt(D / 3.0)
    sf2 = rng.uniform(0.8, 1.2, n_out)
    hyp = [{"lengthscale": ls[d], "variance": sf2[d], "noise_variance": 1e-2 - 1e-5 - 1e-8} for d in range(n_out)]
    gp = SimpleGPModel(n_out, n_out, n_u, kern_types=["rbf"] * n_out, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    dev = gp.device
    gp.draw_paths(S, M, torch.Generator(device=dev).manual_seed(2))
    mc = MonteCarloSafetyVerification(gp)
    K = 0.3 * rng.standard_normal((H, n_u, n_out))
    k = 0.1 * rng.standard_normal((H, n_u))
    x0 = rng.uniform(-0.5, 0.5, (n_out, 1))
    kw = dict(n=H, n_samples=S, n_features=M, as_tensor=True)
    Kt, kt = torch.as_tensor(K, device=dev), torch.as_tensor(k, device=dev)
    x0t = torch.as_tensor(x0[:, 0], device=dev)
    xs = torch.rand((S, D), dtype=torch.float64, device=dev) * 2 - 1

    calls = [
        ("chained  sample_n_step(consistent)", lambda: mc.sample_n_step(x0, K, k, consistent=True, **kw)),
        ("fused    rollout_paths", lambda: mc.rollout_paths(x0, K, k, **kw)),
        ("fused    paths_rollout_device", lambda: gp.paths_rollout_device(x0t, Kt, kt)),
        ("chained  sample_n_step_jacobians", lambda: mc.sample_n_step_jacobians(x0, K, k, **kw)),
        ("fused    rollout_paths(jacobians)", lambda: mc.rollout_paths(x0, K, k, jacobians=True, **kw)),
        ("fused    paths_rollout_device(jac)", lambda: gp.paths_rollout_device(x0t, Kt, kt, jacobians=True)),
        ("one      paths_step_device", lambda: gp.paths_step_device(xs)),
        ("one      paths_step_device(jac)", lambda: gp.paths_step_device(xs, jacobians=True)),
    ]
    print("paths_rollout %s N=%d n_out=%d D=%d S=%d M=%d H=%d  reps=%d rounds=%d  variant=%s"
          % (name, N, n_out, D, S, M, H, reps, rounds, os.environ.get("SR_ROLLOUT_PATHS", "product")), flush=True)
    ms = {}
    for label, fn in calls:
        ms[label], sp = rounds_ms(fn, reps, rounds)
        print("  %-38s %9.4f ms  spread %5.1f%%" % (label, ms[label], 100 * sp), flush=True)
    a, b = mc.sample_n_step(x0, K, k, consistent=True, **kw)[1], mc.rollout_paths(x0, K, k, **kw)[1]
    print("  max |fused - chained| / max |chained| = %.2e" % float((a - b).abs().max() / a.abs().max()))
    v = [ms[c[0]] for c in calls]
    print("  chained / fused = %.2f (states)  %.2f (with Jacobians)   fused per step = %.4f / %.4f ms against one step %.4f / %.4f ms"
          % (v[0] / v[1], v[3] / v[4], v[2] / H, v[5] / H, v[6], v[7]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--regime", default="both", choices=["cartpole", "big", "both"])
    a = ap.parse_args()
    for name in (("cartpole", "big") if a.regime == "both" else (a.regime,)):
        run(name, a.H, a.reps, a.rounds)


if __name__ == "__main__":
    main()
