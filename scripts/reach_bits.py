#!/usr/bin/env python3
"""Every output of the one-step / per-step reachability and moment entry points, dumped for a bit-for-bit comparison of two
builds of the library (a refactor of csrc/sr_capi_reach.hip must not move a bit).

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
Only calls the Python layer has had since the reverse passes were added, so the same file runs on either tree."""
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


def with_gp(out, tag, gp, x, tz, chunks):
    from safe_exploration_amd import gp_reachability as reach, uncertainty_propagation_casadi as mom
    lin = (x["l_mu"], x["l_sigma"])
    gp.set_chain(False)
    for chunk in chunks:
        gp.set_chunk(65536 if chunk is None else chunk)
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
            put("multistep_reach", reach.multistep_reachability_batch(x["p"], gp, x["k_fb_h"], x["k_ff_h"], *lin, q, x["c"], x["a"],
                                                                      x["b"], kfb, t_z_gp=tz))
            for pb, qb, s in ((x["pb"], None, "p"), (None, x["qb"], "q"), (x["pb"], x["qb"], "pq")):
                put("onestep_reach_vjp_" + s, reach.onestep_reachability_vjp_batch(x["p"], gp, x["k_ff"], *lin, pb, qb, q, kfb,
                                                                                   x["c"], x["a"], x["b"], t_z_gp=tz))
            for mode in (1, 2):
                m = "_m%d" % mode
                put("onestep_moments" + m, mom.onestep_moments_batch(x["p"], gp, x["k_ff"], q, kfb, x["a"], x["b"], mode, tz))
                if not g:
                    put("multistep_moments" + m, mom.multistep_moments_batch(x["p"], gp, x["k_ff_h"], x["k_fb_h"], x["a"], x["b"],
                                                                            mode, tz))
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


def dump(seed, path):
    out = {}
    for n_s, n_u, rows in INSTANCES:
        tz = None if rows is None else np.eye(n_s)[n_s - rows:]
        x = inputs(seed, n_s, n_u, 300)
        tag = "%dx%d" % (n_s, n_u)
        with_gp(out, tag + "/N70", model(seed, n_s, n_u, rows or n_s, 70), x, tz, (64, None))
        stateless(out, tag, x)
    with_gp(out, "2x1/N2000", model(seed, 2, 1, 2, 2000), inputs(seed, 2, 1, 1000), None, (64, 1000, None))
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
