#!/usr/bin/env python3
"""Every output of the reachability, moment-propagation, moment-matching and roll-out cost entry points, dumped for a bit-for-bit
comparison of two builds of the library (a refactor of csrc/sr_capi_reach.hip, sr_capi_chain.hip or sr_capi_moment_match.hip must
not move a bit).

    python scripts/reach_bits.py SEED OUT.npz        dump (run it once under each tree, each in its own process)
    python scripts/reach_bits.py compare A.npz B.npz  np.array_equal with NaNs equal on every array; exit status 1 on a difference

Entry points: sr_onestep_reach, sr_multistep_reach and sr_multistep_moments on the per-step route (set_chain(False), H = 3),
sr_onestep_moments, sr_ellipsoid_step, sr_moment_step, the two reverse passes with the GP inside (sr_onestep_reach_vjp,
sr_onestep_moments_vjp) and the two stateless ones (sr_ellipsoid_step_vjp, sr_moment_step_vjp).  Modes 0, 1, 2; point and
ellipsoid / Gaussian starts; each seed alone and all together; a few queries that violate the bounds in mode 0.
Shapes, the smallest at which each branch is taken: (n_s, n_u) = (1, 1), (2, 1) (sr_onestep_reach through the chain kernel),
(4, 1) under a 3-row input transform, (5, 2) (the first instance with its block in LDS), (8, 4) under a transform that cuts the
model to D = 8 -- N = 70, T = 300, chunks of 64 and the default; and N = 2000, n_s = 2, T = 1000 with chunks of 64, 1000 and the
default, where the reverse passes are bounded at 768 queries and 1000 cross a pass boundary.
The reverse passes of whole roll-outs (sr_multistep_reach_vjp, sr_multistep_moments_vjp in modes 1 and 2) at the same instances and
chunks: H = 3 from a point and from an ellipsoid / a Gaussian, and H = 1 with k_fb = None from a point (the one roll-out in which
mode 1 takes sr_gp_predict_grad); a chunk of 64 makes groups of 21 trajectories, the last one short; at N = 2000 the 3000 queries
cross the pass bound three times.  sr_multistep_moments also with the chain kernel allowed.  At N = 70 only: sr_gp_moment_match and its reverse pass (points and Gaussians, each seed alone and
all together), sr_gp_moment_match_rollout and its reverse pass (one policy for all trajectories and one per trajectory),
sr_gp_moment_match on a lin_rbf model (the general route); and sr_rollout_cost / sr_rollout_cost_vjp (both losses, with and without
an angle, with and without controls).
Only calls the Python layer has had since the roll-out cost was added, so the same file runs on either tree."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H = 3
INSTANCES = [(1, 1, None), (2, 1, None), (4, 1, 3), (5, 2, None), (8, 4, 4)]          # (n_s, n_u, rows of the transform)


def model(seed, n_s, n_u, n_xin, N):
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng([seed, n_s, n_u, N])
    D = n_xin + n_u
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_s)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_s))
    hyp = [dict(lengthscale=rng.uniform(0.5, 1.5, D) * np.sqrt(D / 3.0), variance=float(rng.uniform(0.5, 1.5)), noise_variance=1e-2)
           for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_xin, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    return gp


def inputs(seed, n_s, n_u, T):
    rng = np.random.default_rng([seed, n_s, n_u, T, 1])
    A = rng.standard_normal((T, n_s, n_s))
    x = dict(p=0.3 * rng.standard_normal((T, n_s)), k_ff=0.2 * rng.standard_normal((T, n_u)),
             q=0.02 * np.einsum('tij,tkj->tik', A, A) / n_s, k_fb=0.3 * rng.standard_normal((T, n_u, n_s)),
             a=0.8 * np.eye(n_s) + 0.05 * rng.standard_normal((n_s, n_s)), b=0.1 * rng.standard_normal((n_s, n_u)),
             l_mu=rng.uniform(0.01, 0.05, n_s), l_sigma=rng.uniform(0.01, 0.05, n_s), c=2.0,
             pb=rng.standard_normal((T, n_s)), qb=rng.standard_normal((T, n_s, n_s)), vb=rng.standard_normal((T, n_s)),
             k_ff_h=0.2 * rng.standard_normal((T, H, n_u)), k_fb_h=0.3 * rng.standard_normal((T, H - 1, n_u, n_s)),
             mu=0.3 * rng.standard_normal((T, n_s)), var=rng.uniform(0.01, 0.1, (T, n_s)),
             jac=0.3 * rng.standard_normal((T, n_s, n_s + n_u)))
    x["q"][[3, T // 2, T - 1]] = 0.0                     # box half-widths that are not > 0 in mode 0 from an ellipsoid
    return x


def rollout_seeds(seed, n_s, n_u, T):
    rng = np.random.default_rng([seed, n_s, n_u, T, 2])
    return dict(pb=rng.standard_normal((T, H, n_s)), qb=rng.standard_normal((T, H, n_s, n_s)), vb=rng.standard_normal((T, H, n_s)))


def with_gp(out, tag, gp, x, tz, chunks, r):
    from safe_exploration_amd import gp_reachability as reach, uncertainty_propagation_casadi as mom
    lin = (x["l_mu"], x["l_sigma"])
    gp.set_chain(False)
    for chunk in chunks:
        gp.set_chunk(65536 if chunk is None else chunk)
        fwd = {}
        for start in ("point", "gauss"):
            g = start == "gauss"
            q, kfb = (x["q"], x["k_fb"]) if g else (None, None)
            k = "%s/chunk%s/%s/" % (tag, chunk, start)
            put = lambda name, arrs: out.update({k + name + str(i): a for i, a in enumerate(arrs) if a is not None})
            gp.set_chain(True)                           # (n_s <= 2: sr_onestep_reach tries the chain kernel)
            put("onestep_reach", reach.onestep_reachability_batch(x["p"], gp, x["k_ff"], *lin, q, kfb, x["c"], x["a"], x["b"],
                                                                  return_var=True, t_z_gp=tz))
            gp.set_chain(False)
            put("onestep_reach_per_step", reach.onestep_reachability_batch(x["p"], gp, x["k_ff"], *lin, q, kfb, x["c"], x["a"],
                                                                           x["b"], return_var=True, t_z_gp=tz))
            ra = reach.multistep_reachability_batch(x["p"], gp, x["k_fb_h"], x["k_ff_h"], *lin, q, x["c"], x["a"], x["b"], kfb,
                                                    t_z_gp=tz)
            put("multistep_reach", ra)
            # the roll-outs' reverse passes at stored states: H = 3, and one step with k_fb = None from a point
            cut = lambda arr, h: None if arr is None else np.ascontiguousarray(arr[:, :h])
            steps = (H,) if g else (H, 1)
            for h in steps:
                kfb_h = x["k_fb_h"] if h > 1 else None
                for pb, qb, s in ((r["pb"], None, "p"), (None, r["qb"], "q"), (r["pb"], r["qb"], "pq")):
                    put("multistep_reach_vjp_H%d_%s" % (h, s), reach.multistep_reachability_vjp_batch(
                        x["p"], gp, kfb_h, cut(x["k_ff_h"], h), *lin, cut(ra[0], h), cut(ra[1], h), cut(pb, h), cut(qb, h), q,
                        x["c"], x["a"], x["b"], kfb, t_z_gp=tz))
            for pb, qb, s in ((x["pb"], None, "p"), (None, x["qb"], "q"), (x["pb"], x["qb"], "pq")):
                put("onestep_reach_vjp_" + s, reach.onestep_reachability_vjp_batch(x["p"], gp, x["k_ff"], *lin, pb, qb, q, kfb,
                                                                                   x["c"], x["a"], x["b"], t_z_gp=tz))
            for mode in (1, 2):
                m = "_m%d" % mode
                put("onestep_moments" + m, mom.onestep_moments_batch(x["p"], gp, x["k_ff"], q, kfb, x["a"], x["b"], mode, tz))
                if not g:
                    fwd[mode] = mom.multistep_moments_batch(x["p"], gp, x["k_ff_h"], x["k_fb_h"], x["a"], x["b"], mode, tz)
                    put("multistep_moments" + m, fwd[mode])
                    gp.set_chain(True)                   # (small models: the persistent chain kernel)
                    put("multistep_moments_chain" + m, mom.multistep_moments_batch(x["p"], gp, x["k_ff_h"], x["k_fb_h"], x["a"],
                                                                                  x["b"], mode, tz))
                    gp.set_chain(False)
                for h in steps:                          # (the stored states: those of the roll-out from the point)
                    kfb_h = x["k_fb_h"] if h > 1 else None
                    for pb, qb, vb, s in ((r["pb"], None, None, "p"), (None, r["qb"], None, "q"), (None, None, r["vb"], "v"),
                                          (r["pb"], r["qb"], r["vb"], "pqv")):
                        put("multistep_moments_vjp%s_H%d_%s" % (m, h, s), mom.multistep_moments_vjp_batch(
                            x["p"], gp, cut(x["k_ff_h"], h), kfb_h, cut(fwd[mode][0], h), cut(fwd[mode][1], h), cut(pb, h), cut(qb, h),
                            cut(vb, h), x["a"], x["b"], mode, tz, sigma_0=q))
                for pb, qb, vb, s in ((x["pb"], None, None, "p"), (None, x["qb"], None, "q"), (None, None, x["vb"], "v"),
                                      (x["pb"], x["qb"], x["vb"], "pqv")):
                    put("onestep_moments_vjp%s_%s" % (m, s), mom.onestep_moments_vjp_batch(x["p"], gp, x["k_ff"], pb, qb, vb, q, kfb,
                                                                                          x["a"], x["b"], mode, tz))
    gp.set_chunk(65536)
    gp.set_chain(True)


def stateless(out, tag, x):
    from safe_exploration_amd import gp_reachability as reach, uncertainty_propagation_casadi as mom
    lin = (x["l_mu"], x["l_sigma"])
    for start in ("point", "gauss"):
        g = start == "gauss"
        q, kfb, jac = (x["q"], x["k_fb"], x["jac"]) if g else (None, None, None)
        k = "%s/%s/" % (tag, start)
        put = lambda name, arrs: out.update({k + name + str(i): a for i, a in enumerate(arrs) if a is not None})
        put("ellipsoid_step", reach.ellipsoid_step_batch(x["p"], x["k_ff"], x["mu"], x["var"], jac, *lin, q, kfb, x["c"], x["a"],
                                                         x["b"]))
        for pb, qb, s in ((x["pb"], None, "p"), (None, x["qb"], "q"), (x["pb"], x["qb"], "pq")):
            put("ellipsoid_step_vjp_" + s, reach.ellipsoid_step_vjp_batch(x["p"], x["k_ff"], x["mu"], x["var"], jac, *lin, pb, qb, q,
                                                                          kfb, x["c"], x["a"], x["b"]))
            for mode in (1, 2):
                put("moment_step_vjp_m%d_%s" % (mode, s), mom.moment_step_vjp_batch(x["p"], x["k_ff"], x["mu"], x["var"], jac, pb, qb,
                                                                                   q, kfb, x["a"], x["b"], mode))
        for mode in (1, 2):
            put("moment_step_m%d" % mode, mom.moment_step_batch(x["p"], x["k_ff"], x["mu"], x["var"], jac, q, kfb, x["a"], x["b"],
                                                               mode))


def lin_rbf_model(seed, n_s, n_u, N):
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng([seed, n_s, n_u, N, 3])
    D = n_s + n_u
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_s)) / np.sqrt(D))) + 0.3 * Z.dot(rng.standard_normal((D, n_s)))
    hyp = [{"prod.rbf.lengthscale": rng.uniform(0.6, 1.4, 1), "prod.rbf.variance": float(rng.uniform(0.5, 1.5)),
            "prod.linear.variances": rng.uniform(0.3, 0.9, 1), "linear.variances": rng.uniform(0.1, 0.5, D), "noise_variance": 1e-2}
           for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["lin_rbf"] * n_s, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    return gp


def moment_matching(out, tag, gp, x, tz, r, D, chunks, reverse=True):
    """sr_gp_moment_match* through the device methods of the model (tensors out: copied back)"""
    from safe_exploration_amd import _buffers as B
    T, n = x["p"].shape
    rng = np.random.default_rng([T, n, D, 4])
    A = rng.standard_normal((T, D, D))
    m, S = 0.3 * rng.standard_normal((T, D)), 0.02 * np.einsum('tij,tkj->tik', A, A) / D
    mb, cb, Vb = rng.standard_normal((T, n)), rng.standard_normal((T, n, n)), rng.standard_normal((T, n, D))
    for chunk in chunks:
        gp.set_chunk(65536 if chunk is None else chunk)
        for start, S_in, sig in (("point", None, None), ("gauss", S, x["q"])):
            k = "%s/chunk%s/%s/" % (tag, chunk, start)
            put = lambda name, arrs: out.update({k + name + str(i): B.to_numpy(a) for i, a in enumerate(arrs) if a is not None})
            put("moment_match", gp.moment_match_device(m, S_in))
            if not reverse:
                continue
            for s, seeds in (("m", (mb, None, None)), ("c", (None, cb, None)), ("V", (None, None, Vb)), ("mcV", (mb, cb, Vb))):
                put("moment_match_vjp_" + s, gp.moment_match_vjp_device(m, S_in, *seeds))
            for per_traj in (0, 1):
                kff, kfb = (x["k_ff_h"], x["k_fb_h"]) if per_traj else (x["k_ff_h"][0], x["k_fb_h"][0])
                fw = gp.moment_match_rollout_device(x["p"], kff, kfb, x["a"], x["b"], sigma0=sig, a_gp_inp_x=tz)
                put("moment_match_rollout_g%d" % per_traj, fw)
                for s, seeds in (("p", (r["pb"], None, None)), ("q", (None, r["qb"], None)), ("c", (None, None, r["qb"][::-1].copy())),
                                 ("pqc", (r["pb"], r["qb"], r["qb"][::-1].copy()))):
                    put("moment_match_rollout_vjp_g%d_%s" % (per_traj, s), gp.moment_match_rollout_vjp_device(
                        x["p"], kff, kfb, x["a"], x["b"], fw[0], fw[1], *seeds, sigma0=sig, a_gp_inp_x=tz))
    gp.set_chunk(65536)


def rollout_cost(out, tag, n_s, n_u, T):
    from safe_exploration_amd import utils_casadi as uc
    rng = np.random.default_rng([T, n_s, n_u, 5])
    A = rng.standard_normal((T, H, n_s, n_s))
    mu, sigma = 0.5 * rng.standard_normal((T, H, n_s)), 0.05 * np.einsum('thij,thkj->thik', A, A) / n_s
    u, cb = 0.3 * rng.standard_normal((T, H, n_u)), rng.standard_normal(T)
    Ru = rng.standard_normal((n_u, n_u))
    R = Ru.dot(Ru.T) + 0.1 * np.eye(n_u)
    for idx, keep in ((None, False), (0, False), (n_s - 1, True)):
        n_c = n_s if idx is None else n_s + 1 + int(keep)
        z, Wh = 0.3 * rng.standard_normal(n_c), rng.standard_normal((n_c, n_c))
        W = Wh.dot(Wh.T) / n_c
        for loss in ("sat", "quadratic"):
            for sig, us, Rs, s in ((sigma, u, R, "full"), (None, None, None, "mean")):
                k = "%s/cost/angle%s%d/%s/%s/" % (tag, idx, keep, loss, s)
                put = lambda name, arrs: out.update({k + name + str(i): a for i, a in enumerate(arrs) if a is not None})
                put("cost", uc.rollout_cost_batch(mu, sig, z, W, us, Rs, idx, 0.7, keep, loss, 0.9, 1.3, return_steps=True))
                put("cost_vjp", uc.rollout_cost_vjp_batch(mu, sig, z, W, us, Rs, idx, 0.7, keep, loss, 0.9, 1.3, cost_bar=cb))
                put("cost_vjp_ones", uc.rollout_cost_vjp_batch(mu, sig, z, W, us, Rs, idx, 0.7, keep, loss, 0.9, 1.3))


def dump(seed, path):
    out = {}
    for n_s, n_u, rows in INSTANCES:
        tz = None if rows is None else np.eye(n_s)[n_s - rows:]
        x = inputs(seed, n_s, n_u, 300)
        tag = "%dx%d" % (n_s, n_u)
        r = rollout_seeds(seed, n_s, n_u, 300)
        gp = model(seed, n_s, n_u, rows or n_s, 70)
        with_gp(out, tag + "/N70", gp, x, tz, (64, None), r)
        stateless(out, tag, x)
        moment_matching(out, tag + "/N70", gp, x, tz, r, (rows or n_s) + n_u, (64, None))
        rollout_cost(out, tag, n_s, n_u, 300)
    moment_matching(out, "2x1/N70/lin_rbf", lin_rbf_model(seed, 2, 1, 70), inputs(seed, 2, 1, 300), None, None, 3, (64, None),
                    reverse=False)
    with_gp(out, "2x1/N2000", model(seed, 2, 1, 2, 2000), inputs(seed, 2, 1, 1000), None, (64, 1000, None),
            rollout_seeds(seed, 2, 1, 1000))
    np.savez(path, **out)
    print("%d arrays, %d of them with a NaN, %.1f MB -> %s" % (len(out), sum(bool(np.isnan(a).any()) for a in out.values()),
                                                            sum(a.nbytes for a in out.values()) / 1e6, path))


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    if set(a.files) != set(b.files):
        print("the two dumps hold different arrays: %s" % sorted(set(a.files) ^ set(b.files))[:10])
        return 1
    bad = [k for k in a.files if a[k].shape != b[k].shape or not np.array_equal(a[k], b[k], equal_nan=True)]
    for k in bad[:20]:
        print("DIFFERS %s" % k)
    print("%d arrays compared (%d with a NaN, %d values), %d differ" % (len(a.files), sum(bool(np.isnan(a[k]).any()) for k in a.files),
                                                                     sum(a[k].size for k in a.files), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    dump(int(sys.argv[1]), sys.argv[2])
