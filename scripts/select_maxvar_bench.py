"""Greedy max-variance selection, both routes of choose_datapoints_maxvar on one model: "predict" (a batched posterior over
the pool and a row append per round, one blocking read-back of the pick per round) and "downdate" (sr_gp_select_maxvar:
pivoted Cholesky downdates, one launch per round, one read-back at the end, one fit on the chosen rows).

    python scripts/select_maxvar_bench.py [--grid 2000x150,10000x500,50000x2000] [--nout 2,4] [--kernels rbf,mat52]
                                          [--reps 2] [--routes predict,downdate]

One line per (kernel, n_out, n, m): wall ms of each route (host clock around the whole call: it ends in a read-back), the
speed-up, whether the two routes picked the same rows, and the downdate route's rate over the bytes of L its rounds read
(n_out n sum_r r doubles).  Seeds: 10 fixed random rows (what the k-means seeding would hand over)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def model(kt, n, n_out, D=3, seed=0):
    from safe_exploration_amd import SimpleGPModel
    rng = np.random.default_rng(seed)
    Z = rng.uniform(-1, 1, (n, D))
    Y = np.sin(2 * Z @ rng.standard_normal((D, n_out))) + 0.05 * rng.standard_normal((n, n_out))
    hyp = [{"lengthscale": rng.uniform(0.5, 1.5, D), "variance": 1.0, "noise_variance": 1e-2} for _ in range(n_out)]
    gp = SimpleGPModel(n_out, D - 1, 1, kern_types=[kt] * n_out, hyp=hyp)
    init = [int(i) for i in rng.choice(n, 10, replace=False)]
    return gp, Z, Y, init


def timed(fn, reps):
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        t = (time.perf_counter() - t0) * 1e3
        best = t if best is None else min(best, t)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", default="2000x150,10000x500,50000x2000")
    ap.add_argument("--nout", default="2,4")
    ap.add_argument("--kernels", default="rbf,mat52")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--routes", default="predict,downdate")
    args = ap.parse_args()
    routes = args.routes.split(",")
    for kt in args.kernels.split(","):
        for n_out in (int(v) for v in args.nout.split(",")):
            for sz in args.grid.split(","):
                n, m = (int(v) for v in sz.split("x"))
                gp, Z, Y, init = model(kt, n, n_out)
                res = {}
                for route in routes:
                    gp.choose_datapoints_maxvar(Z, Y, min(m, 20), init_idx=init, route=route)        # warm-up
                    res[route] = timed(lambda: gp.choose_datapoints_maxvar(Z, Y, m, init_idx=init, route=route,
                                                                           return_index=True)[2], args.reps)
                line = "%s n_out=%d n=%d m=%d:" % (kt, n_out, n, m)
                for route in routes:
                    line += " %s %.1f ms," % (route, res[route][0])
                if len(routes) == 2:
                    line += " speed-up %.1fx, same picks %s," % (res["predict"][0] / res["downdate"][0],
                                                                 np.array_equal(res["predict"][1], res["downdate"][1]))
                if "downdate" in routes:
                    gb = n_out * n * (m - 1) * (m - 2) / 2 * 8 / 1e9
                    line += " L read %.2f GB = %.0f GB/s over the whole call" % (gb, gb / (res["downdate"][0] * 1e-3))
                print(line, flush=True)
                del gp
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
