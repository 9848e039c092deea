"""Timings behind the exploration objective (profiles/r28_explore.txt).

    python scripts/bench_explore.py [OUT] [--parent-root PATH]

One run, everything alternating in it:
  a. sr_multistep_reach_vjp of this library against the parent commit's library (PATH: a checkout of the parent commit with its library built; left
     out when not given), each in a child process of its own, the two children started alternately twice; and sha256 of
     the outputs of both on the roll-out cases of tests/_reach_rollout_grad_ref.py with a model of this script (must be equal);
  b. sr_multistep_reach_var_vjp with seeds (w_p, w_v) against the same call with w_p only;
  c. the forward with and without gp_var_all, on the persistent and on the per-step route;
  d. exploration_cost_batch + exploration_cost_vjp_batch against the same expressions in batched torch fp64 with autograd;
  e. a whole exploration gradient (roll-out with variances, objective VJP, roll-out VJP) against the roll-out gradient of a linear
     functional (roll-out, roll-out VJP).
Cart-pole (N = 150, n_s = 4, n_u = 1) and pendulum (N = 200, n_s = 2, n_u = 1) regimes, H = 15, T = 1 / 16 / 256 / 3840.  Times: host
clock around synchronised batches of calls on device tensors after a warm-up; the median of seven batches with the fastest and the
slowest beside it."""
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

# (a child of part a. runs this file on another checkout: the parent commit's, with its own package, library and helpers)
ROOT = os.environ.get("SR_BENCH_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

REGIMES = (("cart-pole", 150, 4, 1), ("pendulum", 200, 2, 1))
TS, H = (1, 16, 256, 3840), 15


def batches(fn, per, warmup=5, n_batches=7):
    import torch
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
    return "%9.1f us [%8.1f .. %8.1f]" % tuple(x)


def setup(N, n_s, n_u, T):
    import torch
    from reach_grad_bench import model
    gp = model(N, n_s, n_u)
    rng = np.random.default_rng(1)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=gp.device)
    d = dict(p0=t(0.3 * rng.standard_normal((T, n_s))), kff=t(0.2 * rng.standard_normal((T, H, n_u))),
             kfb=t(0.3 * rng.standard_normal((T, H - 1, n_u, n_s))), wp=t(rng.standard_normal((T, H, n_s))),
             wv=t(rng.standard_normal((T, H, n_s))))
    return gp, d, (np.full(n_s, 0.03), np.full(n_s, 0.03), None, 1.7, 0.9 * np.eye(n_s), 0.1 * rng.standard_normal((n_s, n_u)))


def child():
    """times of sr_multistep_reach_vjp (p seed) per regime and T, and output hashes, of the checkout SR_BENCH_ROOT names (default: this)"""
    import _reach_rollout_grad_ref as RR
    from safe_exploration_amd import gp_reachability as reach
    out = dict(times={}, hashes={})
    for name, N, n_s, n_u in REGIMES:
        for T in TS:
            gp, d, ra = setup(N, n_s, n_u, T)
            pa, qa = reach.multistep_reachability_batch(d["p0"], gp, d["kfb"], d["kff"], *ra)
            fn = lambda: reach.multistep_reachability_vjp_batch(d["p0"], gp, d["kfb"], d["kff"], ra[0], ra[1], pa, qa, d["wp"], None, None,
                                                                ra[3], ra[4], ra[5])
            out["times"]["%s T=%d" % (name, T)] = batches(fn, 20 if T <= 256 else 5)
    # the one instance of the sweep whose register allocation lost a wavefront per SIMD to the added seed, <5, 4> (n_s = 5, n_u = 4
    # behind a 4 x 5 input transform: D = 8), timed on both checkouts too
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(4)
    Z = rng.uniform(-1, 1, (150, 8))
    Y = 0.2 * np.sin(2.0 * Z.dot(rng.standard_normal((8, 5)) / np.sqrt(8))) + 0.01 * rng.standard_normal((150, 5))
    gp54 = SimpleGPModel(5, 4, 4, kern_types=["rbf"] * 5, hyp=[{"lengthscale": rng.uniform(0.6, 1.4, 8) * np.sqrt(8 / 3.0), "variance": 0.05,
                                                               "noise_variance": 1e-2} for _ in range(5)])
    gp54.train(Z, Y, opt_hyp=False)
    tz = np.eye(5)[1:]
    for T in (256, 3840):
        _, d, ra = setup(16, 5, 4, T)
        pa, qa = reach.multistep_reachability_batch(d["p0"], gp54, d["kfb"], d["kff"], *ra, t_z_gp=tz)
        fn = lambda: reach.multistep_reachability_vjp_batch(d["p0"], gp54, d["kfb"], d["kff"], ra[0], ra[1], pa, qa, d["wp"], None, None,
                                                            ra[3], ra[4], ra[5], t_z_gp=tz)
        out["times"]["n_s=5 n_u=4 (Tz) T=%d" % T] = batches(fn, 20 if T <= 256 else 5)
    from reach_grad_bench import model
    for key, T, Hc in RR.CASES:
        n_s, n_u, tz = RR.model_dims(key)
        if tz is not None or key.startswith("sparse") or key.startswith("linmat"):
            continue
        gp = model(150, n_s, n_u, seed=3)
        x = RR.rollout_inputs(n_s, n_u, T, Hc)
        for start_q in (False, True):
            q0, k0 = (x["q"], x["k_fb0"]) if start_q else (None, None)
            pa, qa = reach.multistep_reachability_batch(x["p"], gp, x["k_fb"], x["k_ff"], x["l_mu"], x["l_sigma"], q0, x["c"], x["a"], x["b"], k0)
            g = reach.multistep_reachability_vjp_batch(x["p"], gp, x["k_fb"], x["k_ff"], x["l_mu"], x["l_sigma"], pa, qa, x["w_p"], x["w_q"],
                                                       q0, x["c"], x["a"], x["b"], k0)
            h = hashlib.sha256()
            for v in g:
                if v is not None:
                    h.update(np.ascontiguousarray(v).tobytes())
            out["hashes"]["%s T=%d H=%d %s" % (key, T, Hc, "q0" if start_q else "point")] = h.hexdigest()[:16]
    print("RESULT " + json.dumps(out))


def run_child(root):
    env = dict(os.environ)
    if root:
        env["SR_BENCH_ROOT"] = os.path.abspath(root)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env, cwd=root or ROOT, timeout=600)
    if res.returncode != 0:
        raise RuntimeError(res.stdout + res.stderr)
    return json.loads([l for l in res.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])


def main(out_path, parent_root):
    import torch
    from safe_exploration_amd import gp_reachability as reach
    # (the children run before this process opens the device)
    runs = [(tag, run_child(lib)) for _ in range(2) for tag, lib in (("parent", parent_root), ("this", None))] if parent_root else []
    out = ["# scripts/bench_explore.py on %s; us per call: median [fastest .. slowest] of seven synchronised batches, H = %d"
           % (torch.cuda.get_device_name(0), H)]
    if parent_root:
        out.append("a. sr_multistep_reach_vjp (seed on p_all), this library against the parent commit's, children started alternately 2 x")
        for key in runs[0][1]["times"]:
            row = {tag: [r["times"][key][0] for t, r in runs if t == tag] for tag in ("parent", "this")}
            out.append("   %-26s parent %s   this %s   (medians of the two children each)"
                       % (key, " / ".join("%.1f" % v for v in row["parent"]), " / ".join("%.1f" % v for v in row["this"])))
        hp, ht = runs[0][1]["hashes"], runs[1][1]["hashes"]
        same = all(hp[k] == ht[k] for k in hp) and all(r["hashes"] == (hp if t == "parent" else ht) for t, r in runs)
        out.append("   output hashes on %d roll-out cases (sha256 of the five gradients, first 16 hex digits): %s"
                   % (len(hp), "ALL EQUAL between the parent's library and this one" if same else "DIFFERENT"))
        for k in hp:
            out.append("      %-34s parent %s  this %s" % (k, hp[k], ht[k]))
    for name, N, n_s, n_u in REGIMES:
        for T in TS:
            gp, d, ra = setup(N, n_s, n_u, T)
            per = 20 if T <= 256 else 5
            vjp = lambda wp, wv: reach.multistep_reachability_vjp_batch(d["p0"], gp, d["kfb"], d["kff"], ra[0], ra[1], pa, qa, wp, None, None,
                                                                        ra[3], ra[4], ra[5], gpvar_all_bar=wv)
            fwd = lambda flag: reach.multistep_reachability_batch(d["p0"], gp, d["kfb"], d["kff"], *ra, return_gp_var=flag)
            pa, qa, var = fwd(True)
            out.append("%s T=%d (N=%d, n_s=%d)" % (name, T, N, n_s))
            tb = [batches(lambda: vjp(d["wp"], None), per), batches(lambda: vjp(d["wp"], d["wv"]), per),
                  batches(lambda: vjp(d["wp"], None), per), batches(lambda: vjp(d["wp"], d["wv"]), per)]
            out.append("   b. reverse pass, seed p_all only %s | %s   with the variance seed %s | %s" % (fmt(tb[0]), fmt(tb[2]), fmt(tb[1]), fmt(tb[3])))
            for chain in (True, False):
                gp.set_chain(chain)
                t0, t1 = batches(lambda: fwd(False), per), batches(lambda: fwd(True), per)
                out.append("   c. forward, %s route (last_chain %d): without gp_var_all %s   with %s"
                           % ("persistent" if chain else "per-step", gp.last_chain, fmt(t0), fmt(t1)))
            gp.set_chain(True)
            eps = 1e-8

            def dev_cost():
                return reach.exploration_cost_batch(var, "sqrt", eps), reach.exploration_cost_vjp_batch(var, "sqrt", eps)

            def torch_cost():
                v = var.detach().requires_grad_(True)
                c = -torch.sqrt(v.sum(dim=2) + eps).sum(dim=1)
                return c, torch.autograd.grad(c.sum(), v)

            td = [batches(dev_cost, 50), batches(torch_cost, 50), batches(dev_cost, 50), batches(torch_cost, 50)]
            out.append("   d. objective + VJP on the device %s | %s   batched torch with autograd %s | %s" % (fmt(td[0]), fmt(td[2]), fmt(td[1]), fmt(td[3])))

            def explore_grad():
                p, q, v = fwd(True)
                return vjp(None, reach.exploration_cost_vjp_batch(v, "sqrt", eps)[0])

            def linear_grad():
                fwd(False)
                return vjp(d["wp"], None)

            te = [batches(explore_grad, per), batches(linear_grad, per), batches(explore_grad, per), batches(linear_grad, per)]
            out.append("   e. whole exploration gradient %s | %s   roll-out gradient of a linear functional %s | %s"
                       % (fmt(te[0]), fmt(te[2]), fmt(te[1]), fmt(te[3])))
    text = "\n".join(out) + "\n"
    print(text)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    else:
        args = [a for a in sys.argv[1:] if not a.startswith("--")]
        plib = sys.argv[sys.argv.index("--parent-root") + 1] if "--parent-root" in sys.argv else None
        if plib in args:
            args.remove(plib)
        main(args[0] if args else os.path.join(ROOT, "profiles", "r28_explore.txt"), plib)
