"""Path Jacobians (sr_gp_paths_eval_grad / _step_grad) of ONE size beside the value calls they extend: milliseconds per call
from torch events around the C entry points, each measured --rounds times (the median, and the spread (max - min) / median of
those repeats of the same command beside it), and the handle's sr_prof sums of the kernel ids the calls count under.

    python scripts/paths_grad_bench.py --N 150 --nout 4 --D 5 --S 1024 --M 1024 --T 1024 [--reps 5] [--rounds 5]

Beside them: 2 D calls of _step (the central differences _step_grad replaces), the same step formulas in batched torch
fp64 on the same device, and (1 + D) calls of _eval (the matrix-core work of _eval_grad is (1 + D)-fold).
Copied into a checkout of a commit without the two symbols it measures _step and _eval alone: run the two checkouts
alternately, one process each, to see that the value calls did not move.  One process per size."""
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


def rounds_ms(fn, reps, rounds):
    v = sorted(ev_ms(fn, reps) for _ in range(rounds))
    med = v[len(v) // 2]
    return med, (v[-1] - v[0]) / med


def main():
    ap = argparse.ArgumentParser()
    for k, v in (("N", 150), ("nout", 4), ("D", 5), ("S", 1024), ("M", 1024), ("T", 1024), ("reps", 5), ("rounds", 5)):
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    from safe_exploration_amd import SimpleGPModel, _lib, _buffers as B
    lib, check = _lib.lib, _lib.check
    have_grad = hasattr(lib, "sr_gp_paths_eval_grad")
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
    F, Fg = torch.empty((T, S, n_out), **f64), torch.empty((T, S, n_out), **f64)
    Fs, Fsg = torch.empty((S, n_out), **f64), torch.empty((S, n_out), **f64)
    J = torch.empty((T, S, n_out, D), **f64) if have_grad else None
    Js = torch.empty((S, n_out, D), **f64)
    check(lib.sr_gp_paths_draw(hd.h, S, M, B.ptr(om), B.ptr(tau), B.ptr(w), B.ptr(eps), s))

    def evaluate():
        check(lib.sr_gp_paths_eval(hd.h, B.ptr(x), T, B.ptr(F), s))

    def step():
        check(lib.sr_gp_paths_step(hd.h, B.ptr(xs), B.ptr(Fs), None, None, None, s))

    def evaluate_grad():
        check(lib.sr_gp_paths_eval_grad(hd.h, B.ptr(x), T, B.ptr(Fg), B.ptr(J), s))

    def step_grad():
        check(lib.sr_gp_paths_step_grad(hd.h, B.ptr(xs), B.ptr(Fsg), B.ptr(Js), None, None, None, s))

    def step_2d():
        for _ in range(2 * D):
            step()

    def evaluate_1d():
        for _ in range(1 + D):
            evaluate()

    def prof(fn, kids):
        check(lib.sr_prof_enable(hd.h, 1))
        check(lib.sr_prof_reset(hd.h))
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        out = []
        for kid in kids:
            t, n = ctypes.c_double(0), ctypes.c_long(0)
            check(lib.sr_prof_get(hd.h, kid, ctypes.byref(t), ctypes.byref(n)))
            out.append(t.value / a.reps)
        check(lib.sr_prof_enable(hd.h, 0))
        return out

    head = "paths_grad%s N=%d n_out=%d D=%d S=%d M=%d T=%d" % (" [" + a.tag + "]" if a.tag else "", N, n_out, D, S, M, T)
    print(head, flush=True)

    def line(name, fn):
        ms, sp = rounds_ms(fn, a.reps, a.rounds)
        print("  %-22s %10.4f ms  spread %5.1f%%" % (name, ms, 100 * sp), flush=True)
        return ms

    t_step = line("step", step)
    t_eval = line("eval", evaluate)
    if not have_grad:
        return
    # the same step formulas in batched torch fp64 (c taken from the reference solve: dense K_y, Cholesky)
    tZ, tY = torch.as_tensor(Z, **f64), torch.as_tensor(Y, **f64)
    tl, tf = torch.as_tensor(ls, **f64), torch.as_tensor(sf2, **f64)
    amp = torch.sqrt(2 * tf / M)[:, None, None]

    def kern(xa, xb):
        return tf[:, None, None] * torch.exp(-0.5 * torch.cdist(xa[None] / tl[:, None, :], xb[None] / tl[:, None, :]) ** 2)

    Lc = torch.linalg.cholesky(kern(tZ, tZ) + nd * torch.eye(N, **f64))
    R = tY.T[:, :, None] - (amp * torch.cos((tZ[None] / tl[:, None, :]) @ om.T + tau)) @ w.transpose(1, 2) \
        - np.sqrt(nd) * eps.transpose(1, 2)
    c = torch.cholesky_solve(R, Lc)                      # (n_out, N, S)
    del Lc, R

    def t_step_grad():
        sw = -amp * torch.sin((xs[None] / tl[:, None, :]) @ om.T + tau) * w                  # (n_out, S, M)
        jf = (sw @ om) / tl[:, None, :]                                                      # (n_out, S, D)
        kc = kern(xs, tZ) * c.transpose(1, 2)                                                # (n_out, S, N)
        jk = (kc @ tZ - kc.sum(-1, keepdim=True) * xs[None]) / tl[:, None, :] ** 2
        return (jf + jk).permute(1, 0, 2).contiguous()

    step_grad(); evaluate_grad(); step(); evaluate()
    torch.cuda.synchronize()
    same_f = bool(torch.equal(F, Fg)) and bool(torch.equal(Fs, Fsg))
    err_s = float((Js - t_step_grad()).abs().max())
    print("  F bit for bit: %s   max|J_step|=%.2f   |step_grad - torch|=%.2e" % (same_f, float(Js.abs().max()), err_s))
    t_sg = line("step_grad", step_grad)
    t_s2d = line("2 D x step", step_2d)
    t_tsg = line("torch fp64 step grad", t_step_grad)
    t_eg = line("eval_grad", evaluate_grad)
    t_e1d = line("(1 + D) x eval", evaluate_1d)
    ks = (_lib.K_KSTAR, _lib.K_PATHS_EVAL, _lib.K_PATHS_STEP)
    pe, peg = prof(evaluate, ks), prof(evaluate_grad, ks)
    ps, psg = prof(step, ks), prof(step_grad, ks)
    print("  step_grad / step = %.2f   (2 D x step) / step_grad = %.2f   torch / step_grad = %.2f"
          % (t_sg / t_step, t_s2d / t_sg, t_tsg / t_sg))
    print("  eval_grad / eval = %.2f   eval_grad / ((1 + D) x eval) = %.2f" % (t_eg / t_eval, t_eg / t_e1d))
    print("  sr_prof per call [ms]: eval K*=%.4f PATHS_EVAL=%.4f | eval_grad K*=%.4f PATHS_EVAL=%.4f | step PATHS_STEP=%.4f | "
          "step_grad PATHS_STEP=%.4f" % (pe[0], pe[1], peg[0], peg[1], ps[2], psg[2]))
    # PATHS_EVAL of _eval is one feature slab + one product; of _eval_grad 1 + D of each plus D passes over K*
    print("  eval_grad's slab passes beyond (1 + D) x eval's own scope: %.4f ms of %.4f ms"
          % (peg[1] - (1 + D) * pe[1], peg[1]), flush=True)


if __name__ == "__main__":
    main()
