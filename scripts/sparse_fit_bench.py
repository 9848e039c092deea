"""Sparse GP fit (sr_gp_fit_sparse) of ONE size: milliseconds per fit, split by the handle's sr_prof counters into the
streamed part (cross-covariance panels + the accumulating fp64-MFMA product G += K_fu^T K_fu over all data rows) and the
m x m part (three factorisations, two inverse products), and the streamed product's rate.

    python scripts/sparse_fit_bench.py --m 2048 --N 200000 [--nout 2] [--D 3] [--reps 3] [--chunk 16384]

One process per size (the driver chains the sizes, each under its own time limit).  FLOP count of the streamed product:
n_out m_p (m_p + 128) / 2 N fused multiply-adds = n_out m_p (m_p + 128) N flops (upper block triangle, m_p = m padded
to 128), against the fp64 MFMA peak the
project uses (78.6 TF).  The data are generated on the device; the timed region is the C entry point alone."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from _timing import timeit  # noqa: E402

PEAK_TF = 78.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, required=True)
    ap.add_argument("--N", type=int, required=True)
    ap.add_argument("--nout", type=int, default=2)
    ap.add_argument("--D", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--check", action="store_true", help="compare mean / variance at 64 queries with the fp64 NumPy formulas")
    a = ap.parse_args()
    from safe_exploration_amd import SimpleGPModel, _lib, _buffers as B
    from safe_exploration_amd.ssm_hip.gaussian_process import _Handle, SPARSE_JITTER
    lib = _lib.lib
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    X = torch.rand((a.N, a.D), generator=gen, device=dev, dtype=torch.float64) * 2 - 1
    w = torch.rand((a.D, a.nout), generator=gen, device=dev, dtype=torch.float64) + 0.5
    Y = torch.sin(X @ w) + 0.1 * torch.randn((a.N, a.nout), generator=gen, device=dev, dtype=torch.float64)
    Zu = X[torch.randperm(a.N, generator=gen, device=dev)[:a.m]].cpu().numpy()
    # lengthscale: about m^(-1/D) of the box per inducing point and dimension (cond K_uu stays moderate: 1.5 times that makes
    # K_uu^-1 - Sigma^-1 indefinite in fp64 at m = 5000, which the fit reports as SR_ENOTPD)
    ls = 2.0 * a.m ** (-1.0 / a.D)
    hyp = [{"lengthscale": np.full(a.D, ls), "variance": 1.0, "noise_variance": 1e-2 - 1e-5} for _ in range(a.nout)]
    gp = SimpleGPModel(a.nout, a.D - 1, 1, kern_types=["rbf"] * a.nout, hyp=hyp)
    hd = _Handle(dev, a.m, a.D, a.nout)
    s = B.stream_ptr(dev)
    gp._set_data(hd, Zu, np.zeros((a.m, a.nout)), np.full(a.nout, 1e-2), dev, s)
    _lib.check(lib.sr_gp_set_chunk(hd.h, a.chunk))
    info = (ctypes.c_int * a.nout)()

    def fit():
        _lib.check(lib.sr_gp_fit_sparse(hd.h, B.ptr(X), B.ptr(Y), a.N, SPARSE_JITTER, s, info))
    fit()                                             # first touch of the workspace
    ms = timeit(fit, n=a.reps, warmup=1, batches=a.reps) / 1e3          # (the median fit)
    # split: one more fit with the per-kernel event pairs on
    _lib.check(lib.sr_prof_enable(hd.h, 1))
    _lib.check(lib.sr_prof_reset(hd.h))
    fit()
    t, n = ctypes.c_double(0), ctypes.c_long(0)
    part = {}
    for name, kid in (("panel", _lib.K_SPARSE_PANEL), ("stream_gemm", _lib.K_SPARSE_GEMM), ("gram", _lib.K_GRAM),
                      ("potrf", _lib.K_POTRF), ("gemm", _lib.K_GEMM), ("trinv", _lib.K_TRINV)):
        _lib.check(lib.sr_prof_get(hd.h, kid, ctypes.byref(t), ctypes.byref(n)))
        part[name] = (t.value, n.value)
    _lib.check(lib.sr_prof_enable(hd.h, 0))
    mp = -(-a.m // 128) * 128
    fma = a.nout * mp * (mp + 128) / 2 * float(a.N)          # (the upper block triangle has m_p (m_p + 128) / 2 entries)
    tf = 2 * fma / (part["stream_gemm"][0] * 1e-3) / 1e12 if part["stream_gemm"][0] > 0 else 0.0
    streamed = part["panel"][0] + part["stream_gemm"][0]
    dense = sum(part[k][0] for k in ("gram", "potrf", "gemm", "trinv"))
    print("sparse_fit m=%d N=%d n_out=%d D=%d chunk=%d: %.2f ms/fit | streamed %.2f ms (panel %.2f, MFMA product %.2f = %.1f TF, "
          "%.0f %% of %.1f) | m x m %.2f ms (potrf %.2f, gemm %.2f, trinv %.2f) | launches %d"
          % (a.m, a.N, a.nout, a.D, a.chunk, ms, streamed, part["panel"][0], part["stream_gemm"][0], tf, 100 * tf / PEAK_TF,
             PEAK_TF, dense, part["potrf"][0], part["gemm"][0], part["trinv"][0], sum(v[1] for v in part.values())), flush=True)
    if a.check:
        import scipy.linalg as sla
        Xh, Yh = X.cpu().numpy(), Y.cpu().numpy()
        xq = np.random.default_rng(2).uniform(-1, 1, (64, a.D))

        def k(A, Bm):
            A, Bm = A / ls, Bm / ls
            return np.exp(-0.5 * np.maximum((A * A).sum(1)[:, None] + (Bm * Bm).sum(1)[None, :] - 2 * A @ Bm.T, 0))
        Kuu, Kuf, ks = k(Zu, Zu) + SPARSE_JITTER * np.eye(a.m), k(Zu, Xh), k(xq, Zu)
        Li = sla.solve_triangular(np.linalg.cholesky(Kuu), np.eye(a.m), lower=True)
        Si = sla.solve_triangular(np.linalg.cholesky(Kuu + Kuf @ Kuf.T / 1e-2), np.eye(a.m), lower=True)
        M = Li.T @ Li - Si.T @ Si
        beta = Si.T @ (Si @ (Kuf @ Yh[:, 0])) / 1e-2
        mu, var = B.empty((64, a.nout), dev), B.empty((64, a.nout), dev)
        _lib.check(lib.sr_gp_predict(hd.h, B.ptr(B.as_dev(xq, dev)), 64, B.ptr(mu), B.ptr(var), None, s))
        torch.cuda.synchronize()
        print("  check against fp64 NumPy (output 0): cond K_uu %.1e, max |d mu| %.2e (|beta|_1 %.1e), max |d var| %.2e"
              % (np.linalg.cond(Kuu), np.abs(mu.cpu().numpy()[:, 0] - ks @ beta).max(), np.abs(beta).sum(),
                 np.abs(var.cpu().numpy()[:, 0] - (1.0 - ((ks @ M) * ks).sum(1))).max()), flush=True)


if __name__ == "__main__":
    main()
