"""Batched predictive-variance gradient (sr_gp_predict_grad) against a plain batched predict with d mu/dx, in one process
with torch events; and, at one size, against the per-row single-query loop it replaces in predict(..., jacobians=True).

    python scripts/predict_grad_bench.py [--sizes 2000x4096,5000x65536] [--reps 10] [--loop-size 2000x4096]

One line per size: ms of predict, ms of the gradient call, their ratio, and the G-product rate counted as n_out Np^2 T
flops (what DESIGN counts for the variance contraction) over the whole gradient call minus the plain predict."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def model(N, n_s=2, n_u=1, seed=0):
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(seed)
    D = n_s + n_u
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2 * Z @ rng.standard_normal((D, n_s))) + 0.05 * rng.standard_normal((N, n_s))
    hyp = [{"lengthscale": rng.uniform(0.5, 1.5, D), "variance": 1.0, "noise_variance": 1e-2} for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    return gp, rng


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2000x4096,5000x65536")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-size", default="2000x4096")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for sz in args.sizes.split(","):
        N, T = (int(v) for v in sz.split("x"))
        gp, rng = model(N)
        x = torch.from_numpy(0.4 * rng.standard_normal((T, 3))).to(dev)
        tp = timed(lambda: gp.predict_device(x, True), args.reps)
        tg = timed(lambda: gp.predict_device_grad(x), args.reps)
        Np = (N + 127) // 128 * 128
        Tp = (T + 127) // 128 * 128
        tf = 2 * Np * Np * Tp / ((tg - tp) * 1e-3) / 1e12
        print("N=%d T=%d n_out=2: predict %.3f ms, predict_grad %.3f ms, ratio %.2f; G product (n_out Np^2 T flops over "
              "the difference) %.1f TF" % (N, T, tp, tg, tg / tp, tf), flush=True)
        if sz == args.loop_size:
            xs = x.cpu().numpy()
            gp.predict(xs[:8, :2], xs[:8, 2:], True)
            t0 = time.perf_counter()
            for t in range(T):
                gp._linearize_host(xs[t])
            tl = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            gp.predict(xs[:, :2], xs[:, 2:], True)
            tb = (time.perf_counter() - t0) * 1e3
            print("N=%d T=%d: per-row host loop %.1f ms, batched predict(..., jacobians=True) from NumPy %.3f ms, "
                  "speed-up %.0fx" % (N, T, tl, tb, tl / tb), flush=True)
        del gp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
