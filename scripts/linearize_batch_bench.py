"""Batched second-order linearisation (sr_gp_linearize_batch) against the batched gradient pass it extends
(sr_gp_predict_grad), in one process with torch events; and, at one size, against the per-row single-query loop it
replaces (one linearize_predict(..., jacobians=True) per row).

    python scripts/linearize_batch_bench.py [--sizes 2000x4096,5000x65536] [--reps 10] [--loop-size 2000x4096]

One line per size: ms of predict_device_grad, ms of linearize_device_batch, their difference (the Hessian pass: KH and
KHF), and that difference as a rate over the K* slab the ARD-RBF pass reads (n_out N T 8 bytes) against the 8 TB/s of
HBM.  The kernel's own time comes from a kernel trace (rocprofv3 --kernel-trace --stats) of the same script."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from predict_grad_bench import model, timed  # noqa: E402

HBM_TBS = 8.0


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
        n_out = 2
        x = torch.from_numpy(0.4 * rng.standard_normal((T, 3))).to(dev)
        tg = timed(lambda: gp.predict_device_grad(x), args.reps)
        tl = timed(lambda: gp.linearize_device_batch(x), args.reps)
        dh = tl - tg
        gbs = n_out * N * T * 8 / (dh * 1e-3) / 1e9 if dh > 0 else float("nan")
        print("N=%d T=%d n_out=2 D=3: predict_grad %.3f ms, linearize_batch %.3f ms, ratio %.3f; Hessian pass (difference) "
              "%.3f ms = %.1f %%, K* slab %.2f GB -> %.0f GB/s = %.2f of %.0f TB/s"
              % (N, T, tg, tl, tl / tg, dh, 100 * dh / tg, n_out * N * T * 8 / 1e9, gbs, gbs / 1e3 / HBM_TBS, HBM_TBS),
              flush=True)
        if sz == args.loop_size:
            xs = x.cpu().numpy()
            gp.linearize_predict_batch(xs[:8, :2], xs[:8, 2:])
            gp.linearize_predict(xs[:1, :2], xs[:1, 2:], True)
            t0 = time.perf_counter()
            for t in range(T):
                gp.linearize_predict(xs[t:t + 1, :2], xs[t:t + 1, 2:], True)
            tloop = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            gp.linearize_predict_batch(xs[:, :2], xs[:, 2:])
            tb = (time.perf_counter() - t0) * 1e3
            print("N=%d T=%d: per-row linearize_predict(..., jacobians=True) loop %.1f ms, linearize_predict_batch from "
                  "NumPy %.3f ms, speed-up %.0fx" % (N, T, tloop, tb, tloop / tb), flush=True)
        del gp
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
