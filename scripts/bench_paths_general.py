"""Posterior function samples of the general kernel family beside the ARD-RBF route, in ONE process: milliseconds per call of
sr_gp_paths_draw, _eval (sample_paths), _step (paths_step_device) and _step_grad (its jacobians=True form) -- and _eval_grad --
from torch events around the C entry points, each measured --rounds times (the median, and the spread (max - min) / median of
those repeats beside it), for three models on the same data and draws:

    (a) an "rbf" model on the ARD-RBF route (sr_gp_set_data);
    (b) the same model packed into the family, c0 = 1, a = b = 0, s = 1 / l (sr_gp_set_data_general): identical work, so
        (b) / (a) is what the general kernels cost;
    (c) the in-tree "lin_rbf" model (one group on input dimension 1 + ARD linear).

    python scripts/bench_paths_general.py [--shape cartpole|n5000|both] [--reps 20] [--rounds 5] [--models abc]

The shapes are those of profiles/r12_paths.txt / r13_paths_grad.txt with S = 1024 paths and M = 1024 features: the cart-pole
regime (N = 150, n_out = 4, D = 5, T = 1024) and N = 5000 (n_out = 2, D = 3, T = 4096).  For the per-kernel times run it
under a kernel trace with statistics, in a run of its own (--reps 2 --rounds 1)."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = {"cartpole": (150, 4, 5, 1024, 1024, 1024), "n5000": (5000, 2, 3, 1024, 1024, 4096)}


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


def make_model(which, Z, Y, ls, sf2, nd, rng):
    """the fitted model and its weight count's kind"""
    from safe_exploration_amd import SimpleGPModel
    n_out, D = Y.shape[1], Z.shape[1]
    noise = nd - 1e-5 - 1e-8
    if which == "a":
        hyp = [{"lengthscale": ls[d], "variance": sf2[d], "noise_variance": noise} for d in range(n_out)]
        gp = SimpleGPModel(n_out, D - 1, 1, kern_types=["rbf"] * n_out, hyp=hyp)
    elif which == "b":
        kp = np.zeros((n_out, 3 + 3 * D))
        kp[:, 1], kp[:, 2], kp[:, 3:3 + D] = sf2, 1.0, 1.0 / ls
        gp = SimpleGPModel(n_out, D - 1, 1, kern_types=["lin_rbf"] * n_out, hyp=[{"noise_variance": noise}] * n_out)
        gp._pack_kernel_params = lambda only=None: kp.copy() if only is None else kp[only:only + 1].copy()
    else:
        hyp = [{"prod.rbf.lengthscale": ls[d, 1:2], "prod.rbf.variance": sf2[d], "prod.linear.variances": np.array([0.8]),
                "linear.variances": rng.uniform(0.2, 1.0, D), "noise_variance": noise} for d in range(n_out)]
        gp = SimpleGPModel(n_out, D - 1, 1, kern_types=["lin_rbf"] * n_out, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    return gp


def run_shape(name, a):
    from safe_exploration_amd import _lib, _buffers as B
    lib, check = _lib.lib, _lib.check
    N, n_out, D, S, M, T = SHAPES[name]
    rng = np.random.default_rng(1)
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    ls = rng.uniform(0.5, 1.0, (n_out, D)) * np.sqrt(D / 3.0)
    sf2 = rng.uniform(0.8, 1.2, n_out)
    times, outs = {}, {}
    for which in a.models:
        gp = make_model(which, Z, Y, ls, sf2, 1e-2, np.random.default_rng(3))
        hd = gp._handle
        dev = hd.device
        s = B.stream_ptr(dev)
        n_w = gp.paths_weight_count(M)
        g = torch.Generator(device=dev).manual_seed(2)
        f64 = dict(dtype=torch.float64, device=dev)
        om, tau = torch.randn((M, D), generator=g, **f64), torch.rand((M,), generator=g, **f64) * (2 * np.pi)
        w_all, eps = torch.randn((n_out, S, M + D), generator=g, **f64), torch.randn((n_out, S, N), generator=g, **f64)
        x = torch.rand((T, D), generator=g, **f64) * 2 - 1
        xs = torch.rand((S, D), generator=g, **f64) * 2 - 1
        w = w_all[:, :, :n_w].contiguous()               # (a): the first M of (b)'s weights; (b)'s last D have zero amplitude
        F, Fs = torch.empty((T, S, n_out), **f64), torch.empty((S, n_out), **f64)
        J, Js = torch.empty((T, S, n_out, D), **f64), torch.empty((S, n_out, D), **f64)

        def draw():
            check(lib.sr_gp_paths_draw(hd.h, S, M, B.ptr(om), B.ptr(tau), B.ptr(w), B.ptr(eps), s))

        def evaluate():
            check(lib.sr_gp_paths_eval(hd.h, B.ptr(x), T, B.ptr(F), s))

        def step():
            check(lib.sr_gp_paths_step(hd.h, B.ptr(xs), B.ptr(Fs), None, None, None, s))

        def step_grad():
            check(lib.sr_gp_paths_step_grad(hd.h, B.ptr(xs), B.ptr(Fs), B.ptr(Js), None, None, None, s))

        def evaluate_grad():
            check(lib.sr_gp_paths_eval_grad(hd.h, B.ptr(x), T, B.ptr(F), B.ptr(J), s))

        print("paths_general (%s) %s N=%d n_out=%d D=%d S=%d M=%d T=%d n_w=%d"
              % (which, {"a": "rbf, ARD route", "b": "rbf packed into the family", "c": "in-tree lin_rbf"}[which], N, n_out, D, S, M,
                 T, n_w), flush=True)
        times[which] = {}
        for label, fn in (("draw", draw), ("eval", evaluate), ("step", step), ("step_grad", step_grad), ("eval_grad", evaluate_grad)):
            ms, sp = rounds_ms(fn, a.reps, a.rounds)
            times[which][label] = ms
            print("  %-10s %10.4f ms  spread %5.1f%%" % (label, ms, 100 * sp), flush=True)
        ks = (_lib.K_KSTAR, _lib.K_PATHS_DRAW, _lib.K_PATHS_EVAL, _lib.K_PATHS_STEP)
        check(lib.sr_prof_enable(hd.h, 1))
        prof = []
        for fn in (draw, evaluate, evaluate_grad):
            check(lib.sr_prof_reset(hd.h))
            for _ in range(a.reps):
                fn()
            torch.cuda.synchronize()
            row = []
            for kid in ks:
                t, n = ctypes.c_double(0), ctypes.c_long(0)
                check(lib.sr_prof_get(hd.h, kid, ctypes.byref(t), ctypes.byref(n)))
                row.append(t.value / a.reps)
            prof.append(row)
        check(lib.sr_prof_enable(hd.h, 0))
        print("  sr_prof per call [ms]: draw PATHS_DRAW=%.4f | eval K*=%.4f PATHS_EVAL=%.4f | eval_grad K*=%.4f PATHS_EVAL=%.4f"
              % (prof[0][1], prof[1][0], prof[1][2], prof[2][0], prof[2][2]), flush=True)
        step_grad()
        evaluate_grad()
        torch.cuda.synchronize()
        outs[which] = [t.clone() for t in (F, J, Fs, Js)]
        gp.drop_paths()
        del gp
    if "a" in times and "b" in times:
        print("  (b) / (a): " + "  ".join("%s %.2f" % (k, times["b"][k] / times["a"][k]) for k in times["a"]))
        sc = [float(t.abs().max()) for t in outs["a"]]
        print("  |(b) - (a)| / max|(a)|: " + "  ".join(
            "%s %.1e" % (k, float((u - v).abs().max()) / m) for k, u, v, m in zip(("F", "J", "F_step", "J_step"), outs["b"], outs["a"], sc)))
    if "a" in times and "c" in times:
        print("  (c) / (a): " + "  ".join("%s %.2f" % (k, times["c"][k] / times["a"][k]) for k in times["a"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["cartpole", "n5000", "both"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--models", default="abc")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_paths_general.py needs a GPU"
    for name in (("cartpole", "n5000") if a.shape == "both" else (a.shape,)):
        run_shape(name, a)


if __name__ == "__main__":
    main()
