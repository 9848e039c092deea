"""The fused moment-matching roll-out (sr_gp_moment_match_rollout: SimpleGPModel.moment_match_rollout_device) beside the
per-step route it stands next to (uncertainty_propagation_casadi.moment_matching_batch: H rounds of sr_gp_moment_match with
the torch algebra between them), both in THIS process on the SAME model and inputs, device tensors in and out; and one
moment_match_device call of T Gaussian inputs for the per-step comparison.  Milliseconds per call from torch events around
--reps calls after a warm-up call, device-synchronised, repeated --rounds times: the MINIMUM of the rounds, and their spread
(max - min) / min beside it.

    python scripts/bench_moment_match_rollout.py [--H 15] [--reps 3] [--rounds 7] [--regime cartpole|big|both]

Regimes: cartpole N = 150, n_out = 4, D = 5 at T = 1, 16, 256, 3840; big N = 1000, n_out = 2, D = 3 at T = 1, 64.

The bit check of sr_gp_moment_match (the forward the roll-out stands beside must keep its bits):
    python scripts/bench_moment_match_rollout.py --root <a built checkout of the parent commit> --dump-mm parent.npz
    python scripts/bench_moment_match_rollout.py --compare-mm parent.npz
``--root`` imports the package from another checkout; ``--dump-mm`` writes mu, cov, V of fixed calls, ``--compare-mm`` holds
this checkout's against them with array_equal."""
import argparse
import os
import sys

import numpy as np

REGIMES = {"cartpole": (150, 4, 5, (1, 16, 256, 3840)), "big": (1000, 2, 3, (1, 64))}


def ev_ms(fn, reps):
    import torch
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
    return v[0], (v[-1] - v[0]) / v[0]


def model(N, n_out, D, seed=1):
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(seed)
    n_u = D - n_out
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    ls = rng.uniform(0.6, 1.4, (n_out, D)) * np.sqrt(D / 3.0)
    sf2 = rng.uniform(0.5, 1.5, n_out)
    hyp = [{"lengthscale": ls[d], "variance": sf2[d], "noise_variance": 1e-2} for d in range(n_out)]
    gp = SimpleGPModel(n_out, n_out, n_u, kern_types=["rbf"] * n_out, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    return gp, rng, n_u


def run(name, H, reps, rounds):
    import torch
    from safe_exploration_amd import uncertainty_propagation_casadi as up
    N, n_out, D, Ts = REGIMES[name]
    gp, rng, n_u = model(N, n_out, D)
    dev = gp.device
    a = 0.8 * np.eye(n_out) + 0.05 * rng.standard_normal((n_out, n_out))
    b = 0.3 * rng.standard_normal((n_out, n_u))
    ta, tb = torch.as_tensor(a, device=dev), torch.as_tensor(b, device=dev)
    print("moment_match_rollout %s N=%d n_out=%d D=%d H=%d  reps=%d rounds=%d  (min of the rounds, spread (max - min) / min)"
          % (name, N, n_out, D, H, reps, rounds), flush=True)
    for T in Ts:
        t = lambda x: torch.as_tensor(x, device=dev)
        mu0 = t(0.3 * rng.standard_normal((T, n_out)))
        L = 0.15 * rng.standard_normal((T, n_out, n_out))
        s0 = t(np.matmul(L, np.transpose(L, (0, 2, 1))))
        kff, kfb = t(0.2 * rng.standard_normal((T, H, n_u))), t(0.4 * rng.standard_normal((T, H - 1, n_u, n_out)))
        m = torch.cat((mu0, kff[:, 0]), dim=1)
        G = 0.2 * rng.standard_normal((T, D, D))
        S = t(np.matmul(G, np.transpose(G, (0, 2, 1))))
        fused = lambda: gp.moment_match_rollout_device(mu0, kff, kfb, ta, tb, s0)
        chained = lambda: up.moment_matching_batch(mu0, gp, kff, kfb, a, b, s0)
        one = lambda: gp.moment_match_device(m, S)
        f, fs = rounds_ms(fused, reps, rounds)
        c, cs = rounds_ms(chained, reps, rounds)
        o, os_ = rounds_ms(one, reps, rounds)
        x, y = fused(), chained()
        err = max(float((p - q).abs().max()) for p, q in zip(x, y))
        verdict = "faster by more than the two spreads" if c / f > 1 + fs + cs else (
            "slower by more than the two spreads" if f / c > 1 + fs + cs else "within the two spreads")
        print("  T=%-5d fused %9.4f ms (spread %4.1f%%)  per-step route %9.4f ms (spread %4.1f%%)  ratio %5.2f  [%s]\n"
              "          fused per step %8.4f ms against one sr_gp_moment_match call of T inputs %8.4f ms (spread %4.1f%%)   "
              "max |fused - per-step| = %.1e"
              % (T, f, 100 * fs, c, 100 * cs, c / f, verdict, f / H, o, 100 * os_, err), flush=True)


def mm_outputs():
    """mu, cov, V of sr_gp_moment_match on fixed inputs: both README regimes, full S and points"""
    import torch
    out = {}
    for name, (N, n_out, D, _) in sorted(REGIMES.items()):
        gp, rng, _ = model(N, n_out, D, seed=7)
        m = rng.uniform(-1, 1, (33, D))
        G = 0.2 * rng.standard_normal((33, D, D))
        S = np.matmul(G, np.transpose(G, (0, 2, 1)))
        for kind, Sk in (("full", S), ("point", None)):
            for k, o in zip(("mu", "cov", "V"), gp.moment_match_device(m, Sk)):
                out["%s-%s-%s" % (name, kind, k)] = o.cpu().numpy()
        torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--H", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--regime", default="both", choices=["cartpole", "big", "both"])
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--dump-mm")
    ap.add_argument("--compare-mm")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    if a.dump_mm:
        np.savez(a.dump_mm, **mm_outputs())
        print("sr_gp_moment_match outputs of %s written to %s" % (os.path.abspath(a.root), a.dump_mm))
        return
    if a.compare_mm:
        ref, got = np.load(a.compare_mm), mm_outputs()
        same = {k: bool(np.array_equal(ref[k], got[k])) for k in sorted(got)}
        print("sr_gp_moment_match against %s: %d arrays, array_equal on %s" % (
            a.compare_mm, len(same), "ALL" if all(same.values()) else [k for k, v in same.items() if not v]))
        sys.exit(0 if all(same.values()) else 1)
    for name in (("cartpole", "big") if a.regime == "both" else (a.regime,)):
        run(name, a.H, a.reps, a.rounds)


if __name__ == "__main__":
    main()
