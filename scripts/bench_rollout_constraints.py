"""Time of the SafeMPC constraint rows and their seeds: the device rows (gp_reachability.rollout_constraints_batch +
rollout_constraints_vjp_batch, one launch each) against the same rows written in batched torch fp64 (einsum, sqrt) and differentiated
by autograd (examples/safe_shooting_constrained.torch_constraints), in the same run; then the same pair inside a whole gradient in
k_ff, k_fb of the augmented Lagrangian: roll-out, constraints' reverse pass, roll-out's reverse pass (three raw calls) against
autograd through the einsum form on multistep_reachability_diff_batch.

    python scripts/bench_rollout_constraints.py [OUT] [--compare-lib LIB]     (default OUT: profiles/r27_rollout_constraints.txt)
    python scripts/bench_rollout_constraints.py --safety-hash LIB             (prints the hashes below for any build of the C ABI)

Cart-pole regime: n_s = 4, n_u = 1, H = 15, control bounds, m_obs = m_safe = 8, N = 150; T = 1, 16, 256, 3840.  Times: host clock
around synchronised batches of calls on device tensors, after a warm-up; the median of seven batches with the fastest and the slowest
batch beside it.  The two routes are timed alternately, batch by batch.
Last section: sha256 of sr_safety_distance's output on three shapes (its row arithmetic moved into a function the new kernel
shares); with --compare-lib the same hashes out of another build of the library (the parent commit's), computed in a process of
its own."""
import ctypes
import hashlib
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))

SAFETY_SHAPES = ((1000, 2, 4), (257, 5, 7), (4099, 12, 24))       # (T, n_s, m)


def safety_hashes(lib_path):
    """sha256 of the output of sr_safety_distance on SAFETY_SHAPES, through ctypes alone: any build with that entry will do"""
    lib = ctypes.CDLL(lib_path)
    P = ctypes.c_void_p
    lib.sr_safety_distance.restype = ctypes.c_int
    lib.sr_safety_distance.argtypes = [ctypes.c_int, ctypes.c_long, ctypes.c_int, ctypes.c_int, P, P, P, P, ctypes.c_double, P, P]
    out = []
    for T, n_s, m in SAFETY_SHAPES:
        rng = np.random.default_rng([T, n_s, m])
        A = rng.standard_normal((T, n_s, n_s)) / np.sqrt(n_s)
        host = (rng.standard_normal((T, n_s)), A @ A.transpose(0, 2, 1) + 0.01 * rng.standard_normal((T, n_s, n_s)),
                rng.standard_normal((m, n_s)), rng.standard_normal(m))
        p, q, hm, hv = [torch.as_tensor(np.ascontiguousarray(v), device="cuda:0") for v in host]
        d = torch.empty((T, m), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        rc = lib.sr_safety_distance(0, T, n_s, m, p.data_ptr(), q.data_ptr(), hm.data_ptr(), hv.data_ptr(), 1.7, d.data_ptr(), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        out.append(hashlib.sha256(d.cpu().numpy().tobytes()).hexdigest()[:16])
    return out


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
    from safe_shooting_constrained import torch_constraints, lagrangian
    from safe_exploration_amd import gp_reachability as reach
    n_s, n_u, m = 4, 1, 8
    dev = gp.device
    rng = np.random.default_rng(1)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
    p_0 = t(0.3 * rng.standard_normal((T, n_s)))
    k_ff = t(0.2 * rng.standard_normal((T, H, n_u))).requires_grad_(True)
    k_fb = t(0.3 * rng.standard_normal((T, H - 1, n_u, n_s))).requires_grad_(True)
    a, b = 0.9 * np.eye(n_s), 0.1 * rng.standard_normal((n_s, n_u))
    l_mu, l_sigma, c = np.full(n_s, 0.02), np.full(n_s, 0.02), 2.0
    bounds = np.array([[-0.25, 0.25]])
    h_obs_mat, h_obs = rng.standard_normal((m, n_s)), 0.3 + 0.3 * rng.random(m)
    h_safe_mat, h_safe = rng.standard_normal((m, n_s)), 0.1 + 0.2 * rng.random(m)
    sets = (bounds, h_obs_mat, h_obs, h_safe_mat, h_safe, None, None, c)
    sets_t = (t(bounds), t(h_obs_mat), t(h_obs), t(h_safe_mat), t(h_safe), c)
    roll_args = (l_mu, l_sigma, None, c, a, b)
    kffd, kfbd = k_ff.detach(), k_fb.detach()
    p_all, q_all = reach.multistep_reachability_batch(p_0, gp, kfbd, kffd, *roll_args)
    n_g = 2 * n_u * H + m * (H - 1) + m
    lam, rho = t(0.1 * rng.random((T, n_g))), 2.0

    def dev_forward():
        return reach.rollout_constraints_batch(p_all, q_all, kffd, kfbd, *sets)

    def dev_seeds():
        g = reach.rollout_constraints_batch(p_all, q_all, kffd, kfbd, *sets)
        return g, reach.rollout_constraints_vjp_batch(p_all, q_all, kffd, kfbd, *sets, g_bar=torch.relu(lam + rho * g))

    def port_forward():
        return torch_constraints(p_all, q_all, kffd, kfbd, *sets_t)

    def port_seeds():
        leaves = [v.detach().requires_grad_(True) for v in (p_all, q_all, k_ff, k_fb)]
        g = torch_constraints(*leaves, *sets_t)
        return g, torch.autograd.grad(lagrangian(g, lam, rho), leaves)

    def grad_raw():
        pa, qa = reach.multistep_reachability_batch(p_0, gp, kfbd, kffd, *roll_args)
        g = reach.rollout_constraints_batch(pa, qa, kffd, kfbd, *sets)
        pb, qb, kffb, kfbb, _, _ = reach.rollout_constraints_vjp_batch(pa, qa, kffd, kfbd, *sets, g_bar=torch.relu(lam + rho * g))
        r = reach.multistep_reachability_vjp_batch(p_0, gp, kfbd, kffd, l_mu, l_sigma, pa, qa, pb, qb, None, c, a, b)
        return r[3] + kffb, r[4] + kfbb

    def grad_port():
        pa, qa = reach.multistep_reachability_diff_batch(p_0, gp, k_fb, k_ff, *roll_args)
        return torch.autograd.grad(lagrangian(torch_constraints(pa, qa, k_ff, k_fb, *sets_t), lam, rho), [k_ff, k_fb])

    def grad_plain():                                       # the roll-out's gradient with a linear functional: no constraints at all
        pa, qa = reach.multistep_reachability_diff_batch(p_0, gp, k_fb, k_ff, *roll_args)
        return torch.autograd.grad(pa.sum() + qa.sum(), [k_ff, k_fb])

    (g_dev, s_dev), (g_port, s_port) = dev_seeds(), port_seeds()
    active = float((lam + rho * g_dev > 0).double().mean())
    agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(s_dev[:4], s_port))
    whole = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(grad_raw(), grad_port()))
    t_df, t_pf = alternating((dev_forward, port_forward), per)
    t_ds, t_ps = alternating((dev_seeds, port_seeds), per)
    t_gd, t_gp, t_g0 = alternating((grad_raw, grad_port, grad_plain), max(3, per // 2))
    out.append("  T = %d, H = %d (%d rows a trajectory, %.0f %% of them active)" % (T, H, n_g, 100 * active))
    out.append("    rows alone          device (1 launch)  %s   torch einsum %s   %.2f x" % (fmt(t_df), fmt(t_pf), t_pf[0] / t_df[0]))
    out.append("    rows + seeds        device (2 launches)%s   torch einsum %s   %.2f x" % (fmt(t_ds), fmt(t_ps), t_ps[0] / t_ds[0]))
    out.append("    whole gradient      three raw calls    %s   torch einsum %s   %.2f x" % (fmt(t_gd), fmt(t_gp), t_gp[0] / t_gd[0]))
    out.append("    the roll-out's gradient with a linear functional in place of the constraints  %s" % fmt(t_g0))
    out.append("    seeds, device against einsum form: %.1e of the largest element; whole gradient: %.1e" % (agree, whole))
    out.append("")


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--safety-hash"]:
        print(" ".join(safety_hashes(argv[1])))
        return
    other = None
    if "--compare-lib" in argv:
        k = argv.index("--compare-lib")
        other = argv[k + 1]
        del argv[k:k + 2]
    path = argv[0] if argv else os.path.join(ROOT, "profiles", "r27_rollout_constraints.txt")
    from cautious_shooting_cost import model
    from safe_exploration_amd._build import LIB_PATH
    out = ["The SafeMPC constraint rows (control bounds, 8 obstacle half-spaces on 14 states, 8 terminal rows; n_s = 4, n_u = 1, H = 15) and",
           "their gradient -- time per call, 1 x MI355X (scripts/bench_rollout_constraints.py; median [fastest .. slowest] of seven",
           "synchronised batches, host clock, device tensors; the routes of a row are timed alternately, batch by batch; the ratio is",
           "torch einsum / device)", ""]
    gp = model()
    for T in (1, 16, 256, 3840):
        regime(out, gp, T, per=20 if T < 3840 else 8)
    mine = safety_hashes(LIB_PATH)
    out.append("sr_safety_distance, sha256 of the output on (T, n_s, m) = %s: %s" % (", ".join(map(str, SAFETY_SHAPES)), " ".join(mine)))
    if other:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--safety-hash", other], capture_output=True, text=True, timeout=300)
        theirs = r.stdout.split()
        out.append("the same out of the parent commit's library:%s %s -- %s" % (" " * 37, " ".join(theirs) if theirs else r.stderr.strip()[-200:],
                                                                              "the same bits" if theirs == mine else "DIFFERENT"))
    text = "\n".join(out) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
