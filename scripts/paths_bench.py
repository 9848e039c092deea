"""Posterior function samples (sr_gp_paths_draw / _eval / _step) of ONE size: milliseconds per call from the handle's sr_prof
event pairs and from torch events around the C entry points, beside the same formulas in batched torch fp64 on the same
device in the same run, and -- for eval -- sr_test_gemm_tn at the padded shape (the tile's own ceiling).

    python scripts/paths_bench.py --N 150 --nout 4 --D 5 --S 1024 --M 1024 --T 1024 [--reps 5]

One process per size.  FLOP count of eval: 2 n_out Tp Sp (Mp + Np)."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    for k, v in (("N", 150), ("nout", 4), ("D", 5), ("S", 1024), ("M", 1024), ("T", 1024), ("reps", 5)):
        ap.add_argument("--" + k, type=int, default=v)
    a = ap.parse_args()
    from safe_exploration_amd import SimpleGPModel, _lib, _buffers as B
    lib, check = _lib.lib, _lib.check
    N, n_out, D, S, M, T = a.N, a.nout, a.D, a.S, a.M, a.T
    rng = np.random.default_rng(1)
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    ls = rng.uniform(0.5, 1.0, (n_out, D)) * np.sqrt(D / 3.0)
    sf2 = rng.uniform(0.8, 1.2, n_out)
    nd = 1e-2
    hyp = [{"lengthscale": ls[d], "variance": sf2[d], "noise_variance": nd - 1e-5 - 1e-8} for d in range(n_out)]
    gp = SimpleGPModel(n_out, D - 1, 1, kern_types=["rbf"] * n_out, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    hd = gp._handle
    dev = hd.device
    s = B.stream_ptr(dev)
    g = torch.Generator(device=dev).manual_seed(2)
    f64 = dict(dtype=torch.float64, device=dev)
    om, tau = torch.randn((M, D), generator=g, **f64), torch.rand((M,), generator=g, **f64) * (2 * np.pi)
    w, eps = torch.randn((n_out, S, M), generator=g, **f64), torch.randn((n_out, S, N), generator=g, **f64)
    x = torch.rand((T, D), generator=g, **f64) * 2 - 1
    xs = torch.rand((S, D), generator=g, **f64) * 2 - 1
    F = torch.empty((T, S, n_out), **f64)
    Fs = torch.empty((S, n_out), **f64)

    def draw():
        check(lib.sr_gp_paths_draw(hd.h, S, M, B.ptr(om), B.ptr(tau), B.ptr(w), B.ptr(eps), s))

    def evaluate():
        check(lib.sr_gp_paths_eval(hd.h, B.ptr(x), T, B.ptr(F), s))

    def step():
        check(lib.sr_gp_paths_step(hd.h, B.ptr(xs), B.ptr(Fs), None, None, None, s))

    # the same formulas in batched torch fp64 (dense K_y, Cholesky solve)
    tZ, tY = torch.as_tensor(Z, **f64), torch.as_tensor(Y, **f64)
    tl, tf = torch.as_tensor(ls, **f64), torch.as_tensor(sf2, **f64)

    def feat(xx):                                        # (n_out, rows, M)
        return torch.sqrt(2 * tf / M)[:, None, None] * torch.cos((xx[None] / tl[:, None, :]) @ om.T + tau)

    def kern(xa, xb):                                    # (n_out, rows a, rows b)
        return tf[:, None, None] * torch.exp(-0.5 * torch.cdist(xa[None] / tl[:, None, :], xb[None] / tl[:, None, :]) ** 2)

    Lc = torch.linalg.cholesky(kern(tZ, tZ) + nd * torch.eye(N, **f64))
    state = {}

    def t_draw():
        R = tY.T[:, :, None] - feat(tZ) @ w.transpose(1, 2) - np.sqrt(nd) * eps.transpose(1, 2)
        state["c"] = torch.cholesky_solve(R, Lc)         # (n_out, N, S)

    def t_eval():
        return (feat(x) @ w.transpose(1, 2) + kern(x, tZ) @ state["c"]).permute(1, 2, 0).contiguous()

    def t_step():
        return ((feat(xs) * w).sum(-1) + (kern(xs, tZ) * state["c"].transpose(1, 2)).sum(-1)).T.contiguous()

    draw(); evaluate(); step(); t_draw()
    torch.cuda.synchronize()
    scale = float(t_eval().abs().max())
    err_e = float((F - t_eval()).abs().max())
    err_s = float((Fs - t_step()).abs().max())
    check(lib.sr_prof_enable(hd.h, 1))
    res = {}
    for name, fn, tfn, kid in (("draw", draw, t_draw, _lib.K_PATHS_DRAW), ("eval", evaluate, t_eval, _lib.K_PATHS_EVAL),
                               ("step", step, t_step, _lib.K_PATHS_STEP)):
        check(lib.sr_prof_reset(hd.h))
        ms = ev_ms(fn, a.reps)
        t, n = ctypes.c_double(0), ctypes.c_long(0)
        check(lib.sr_prof_get(hd.h, kid, ctypes.byref(t), ctypes.byref(n)))
        res[name] = (ms, t.value / (a.reps + 1), ev_ms(tfn, a.reps))        # (ev_ms makes reps + 1 calls)
    check(lib.sr_prof_enable(hd.h, 0))
    Np, Sp, Tp, Mp = -(-N // 128) * 128, -(-S // 128) * 128, -(-T // 128) * 128, -(-M // 16) * 16
    K = -(-(Mp + Np) // 16) * 16
    A = torch.randn((K, Tp), generator=g, **f64)
    Bm = torch.randn((K, Sp), generator=g, **f64)
    C = torch.empty((n_out, Tp, Sp), **f64)

    def gemm():
        for d in range(n_out):
            check(lib.sr_test_gemm_tn(dev.index, B.ptr(A), Tp, B.ptr(Bm), Sp, B.ptr(C[d]), Sp, Tp, Sp, K, 1.0, 0.0, 0, s))
    g_ms = ev_ms(gemm, a.reps)
    flop = 2.0 * n_out * Tp * Sp * (Mp + Np)
    print("paths N=%d n_out=%d D=%d S=%d M=%d T=%d | max|F|=%.2f  |eval - torch|=%.2e  |step - torch|=%.2e" % (N, n_out, D, S, M, T, scale, err_e, err_s))
    for name in ("draw", "eval", "step"):
        ms, prof, tms = res[name]
        print("  %-4s %9.3f ms (own kernels by sr_prof %9.3f ms) | torch fp64 %9.3f ms | x%.2f" % (name, ms, prof, tms, tms / ms))
    print("  eval: %.1f TF of its %.1f GF; sr_test_gemm_tn at %d x %d x %d, %d outputs: %.3f ms = %.1f TF"
          % (flop / (res["eval"][0] * 1e-3) / 1e12, flop / 1e9, Tp, Sp, K, n_out, g_ms, flop / (g_ms * 1e-3) / 1e12), flush=True)


if __name__ == "__main__":
    main()
