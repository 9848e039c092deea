#!/usr/bin/env python3
"""Retiring a training point (remove_data / sr_gp_remove) against the refit of the same rows, in the same run.
Per N: retire index 0, N/2 and the last one; the steady sliding-window step (one one-point append + one retire:
update_model(n_max=N)); the parent's alternative, update_model(replace_old=True) on the N - 1 remaining rows.
Times are host wall clock around calls that end in a stream synchronisation, the median of `reps` calls (us).
Byte floor of one removal: the upper triangle of U^-1 read once and written once, 2 n_out Np^2 / 2 x 8 B, at 6.3 TB/s.
GPU box:  python scripts/remove_bench.py [N ...]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from safe_exploration_amd import SimpleGPModel, workload  # noqa: E402

HBM_BPS = 6.3e12


def wall_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0)


def main():
    sizes = [int(a) for a in sys.argv[1:]] or [1000, 5000, 20000]
    reps, extra = 7, 64
    for N in sizes:
        prob = workload.make_problem(13, N + extra, 2, 1, 8, sf2=0.01)
        Z, Y = prob["Z"], prob["Y"]
        gp = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=workload.hyp_list(prob), device="cuda:0")
        gp.append_limit = 10 ** 9
        gp.train(Z[:N], Y[:N], opt_hyp=False)
        Np = gp._handle.Np
        rows = list(range(N))
        nxt = N
        out = {"N": N, "Np": Np, "n_out": 2, "D": 3}
        # warm-up: one append + one retire (code objects, scratch, the spare buffers)
        gp.update_model(Z[nxt:nxt + 1], Y[nxt:nxt + 1], opt_hyp=False, replace_old=False)
        rows.append(nxt)
        nxt += 1
        gp.remove_data(N // 3)
        del rows[N // 3]
        for name, pos in (("first", lambda n: 0), ("middle", lambda n: n // 2), ("last", lambda n: n - 1)):
            ts = []
            for _ in range(reps):
                j = pos(len(rows))
                ts.append(wall_us(lambda: gp.remove_data(j)))
                del rows[j]
                gp.update_model(Z[nxt:nxt + 1], Y[nxt:nxt + 1], opt_hyp=False, replace_old=False)   # (N back; not timed)
                rows.append(nxt)
                nxt += 1
            out["retire_%s_us" % name] = round(statistics.median(ts), 1)
        ts = []
        for _ in range(reps):
            x1, y1 = Z[nxt:nxt + 1], Y[nxt:nxt + 1]
            ts.append(wall_us(lambda: gp.update_model(x1, y1, opt_hyp=False, replace_old=False, n_max=N, retire="oldest")))
            rows.append(nxt)
            del rows[0]
            nxt += 1
        out["window_step_us"] = round(statistics.median(ts), 1)
        assert gp._handle.N == N and gp._handle.Np == Np
        # the parent's alternative: refit of the N - 1 rows a retire leaves, same run
        ref = SimpleGPModel(2, 2, 1, kern_types=["rbf"] * 2, hyp=workload.hyp_list(prob), device="cuda:0")
        keep = np.array(rows)
        ref.train(Z[keep], Y[keep], opt_hyp=False)
        ts = [wall_us(lambda: ref.update_model(Z[keep[1:]], Y[keep[1:]], opt_hyp=False, replace_old=True)) for _ in range(3)]
        ts += [wall_us(lambda: ref.update_model(Z[keep], Y[keep], opt_hyp=False, replace_old=True))]     # (back to the N rows)
        out["refit_us"] = round(statistics.median(ts[:3]), 1)
        floor = 2 * 2 * Np * Np / 2 * 8 / HBM_BPS * 1e6
        worst = max(out["retire_first_us"], out["retire_middle_us"], out["retire_last_us"])
        out["byte_floor_us"] = round(floor, 1)
        out["floor_fraction_of_slowest_retire"] = round(floor / worst, 3)
        out["refit_over_slowest_retire"] = round(out["refit_us"] / worst, 2)
        # the model after all of it against the refit of the same rows
        x = np.hstack((prob["p"], prob["k_ff"]))
        a, b = gp.predict(x), ref.predict(x)
        out["err_mu_var"] = [float(np.abs(a[0] - b[0]).max()), float(np.abs(a[1] - b[1]).max())]
        print(json.dumps(out), flush=True)
        del gp, ref
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
