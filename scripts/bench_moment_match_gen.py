"""Time per call of sr_gp_moment_match on the general-family route (csrc/sr_moment_match_gen.hip) beside the ARD-RBF route
(csrc/sr_moment_match.hip) in the same run, at the shapes of profiles/r10_moment_match.txt:
  * a dense general-family model (every entry of s, a, b and c0 non-zero) and the in-tree lin_rbf structure on the new route,
  * the SAME closed form in batched torch fp64 (``torch_mm_gen``: the separated form the kernels evaluate, chunked to fit memory),
  * the a = 0, b = 0, c0 = 1 model -- the plain ARD-RBF kernel -- on both routes (what the family's extra terms cost).
Device events, warmed up.  Every shape runs in a child process of its own under a time limit; the first step that fails or runs
out of time ends the run (nothing is tried again).

    python scripts/bench_moment_match_gen.py [OUTPUT_FILE]"""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((150, 4, 5, 256, 20, 3), (150, 4, 5, 3840, 5, 2), (5000, 2, 3, 64, 3, 1))      # N, n_out, D, T, calls, torch calls
STEP_TIMEOUT = 240


def torch_mm_gen(kp, Z, alpha, Kinv, m, S, budget=2 ** 26):
    """kp (n, 3 + 3 D) packed [0, v, c0, s, a, b]; Z (N, D); alpha (n, N); Kinv (n, N, N); m (T, D); S (T, D, D)
    -> mu (T, n), cov (T, n, n) (diagonal not clipped), V (T, n, D)"""
    n, N, D, T = kp.shape[0], Z.shape[0], Z.shape[1], m.shape[0]
    f = dict(dtype=torch.float64, device=Z.device)
    v, c0, s, av, bv = kp[:, 1], kp[:, 2], kp[:, 3:3 + D].abs(), kp[:, 3 + D:3 + 2 * D], kp[:, 3 + 2 * D:]
    eye = torch.eye(D, **f)
    KZ = Kinv.matmul(Z)                                                 # per call: (n, N, D), (n, D, D), (n, D)
    ZKZ = Z.t().matmul(KZ)
    bzal = bv * alpha.matmul(Z)
    mu, cov, V = torch.empty((T, n), **f), torch.empty((T, n, n), **f), torch.empty((T, n, D), **f)
    Tc = max(1, min(T, budget // (N * N)))
    for t0 in range(0, T, Tc):
        mm, SS = m[t0:t0 + Tc], S[t0:t0 + Tc]
        nt = len(mm)
        nu = Z[None] - mm[:, None, :]                                   # (Tc, N, D)
        g0, h2, Fp = [], [], []
        for a in range(n):
            d = s[a]
            Lc = torch.linalg.cholesky(eye + d[None, :, None] * SS * d[None, None, :])
            W = torch.linalg.solve_triangular(Lc, torch.diag(d).expand(nt, D, D), upper=False)
            T1 = W.matmul(SS)
            clog = -torch.log(torch.diagonal(Lc, dim1=1, dim2=2)).sum(1)
            az, kap = Z * av[a], bv[a] * KZ[a]
            y = nu.matmul(W.transpose(1, 2))
            tt, tk, sk = az.matmul(T1.transpose(1, 2)), kap.matmul(T1.transpose(1, 2)), kap.matmul(SS)
            c = c0[a] + mm.matmul(az.t()) + (y * tt).sum(2)
            q = v[a] * torch.exp(clog[:, None] - 0.5 * (y * y).sum(2))
            fk = c * (mm.matmul(kap.t()) + (y * tk).sum(2)) - (tt * tk).sum(2) + (az[None] * sk).sum(2)
            wq = alpha[a][None] * q
            g0.append((wq * c).sum(1))
            h2.append((q * fk).sum(1))
            g1 = ((wq * c)[:, :, None] * nu).sum(1)
            g2 = wq.matmul(az)
            x = W.matmul(g1[:, :, None]) - T1.matmul(g2[:, :, None])
            V[t0:t0 + Tc, a] = W.transpose(1, 2).matmul(x).squeeze(2) + g2 + bzal[a]
            Fp.append(SS.matmul(g2[:, :, None]).squeeze(2) + T1.transpose(1, 2).matmul(x).squeeze(2))
            mu[t0:t0 + Tc, a] = g0[a] + mm.matmul(bzal[a])
        SM = SS + mm[:, :, None] * mm[:, None, :]
        for a in range(n):
            for b in range(a, n):
                la, lb = s[a] ** 2, s[b] ** 2
                r = torch.sqrt(la + lb)
                C = eye + r[None, :, None] * SS * r[None, None, :]
                Y = torch.linalg.solve(C, r[None, :, None] * SS)
                rs = torch.where(r != 0, r, torch.ones_like(r))
                woodbury = SS - (SS * r[None, None, :]).matmul(Y)
                Mr = torch.where((r != 0)[None, None, :], Y.transpose(1, 2) / rs[None, None, :],
                                 torch.where((r != 0)[None, :, None], Y / rs[None, :, None], woodbury))
                M = 0.5 * (Mr + Mr.transpose(1, 2))
                clog = -0.5 * torch.linalg.slogdet(C)[1]
                aza, azb = Z * av[a], Z * av[b]
                mi, kv = (la * nu).matmul(M), aza.matmul(M)              # (Tc, N, D): M Li_a nu_i, M az_i
                mj = (lb * nu).matmul(M)
                si = clog[:, None] - 0.5 * (la * nu * (nu - mi)).sum(2)
                sj = -0.5 * (lb * nu * (nu - mj)).sum(2)
                pa = c0[a] + (aza[None] * (mm[:, None, :] + mi)).sum(2)
                pb = c0[b] + (azb[None] * (mm[:, None, :] + mj)).sum(2)
                nuT = nu.transpose(1, 2)
                E = si[:, :, None] + sj[:, None, :] + (lb * mi).matmul(nuT)
                term = torch.exp(E) * ((pa[:, :, None] + (lb * kv).matmul(nuT)) * (pb[:, None, :] + mi.matmul(azb.t()))
                                       + kv.matmul(azb.t()))
                sm = torch.einsum("i,tij,j->t", alpha[a], term, alpha[b])
                if a == b:
                    sm = sm - (term * Kinv[a][None]).sum((1, 2))
                val = (v[a] * v[b] * sm - g0[a] * g0[b] + Fp[a].matmul(bzal[b]) + Fp[b].matmul(bzal[a])
                       + torch.einsum("d,tde,e->t", bzal[a], SS, bzal[b]))
                if a == b:
                    val = (val + c0[a] * v[a] - 2.0 * h2[a] + ((av[a] * v[a] + bv[a])[None] * torch.diagonal(SM, dim1=1, dim2=2)).sum(1)
                           - torch.einsum("d,tde,e,de->t", bv[a], SM, bv[a], ZKZ[a]))
                cov[t0:t0 + Tc, a, b] = val
                cov[t0:t0 + Tc, b, a] = val
    return mu, cov, V


def packed(rng, D, n_out, kind):
    kp = np.zeros((n_out, 3 + 3 * D))
    kp[:, 1], kp[:, 2] = 1.0, (1.0 if kind == "rbf" else (0.0 if kind == "lin_rbf" else 0.7))
    kp[:, 3:3 + D] = 1.0 / (rng.uniform(0.6, 1.4, (n_out, D)) * np.sqrt(D / 3.0))
    if kind == "dense":
        kp[:, 3 + D:3 + 2 * D], kp[:, 3 + 2 * D:] = rng.uniform(0.2, 0.8, (n_out, D)) / D, rng.uniform(0.1, 0.5, (n_out, D)) / D
    if kind == "lin_rbf":
        kp[:, 3:3 + D] *= (np.arange(D) == 1)
        kp[:, 3 + D + 1], kp[:, 3 + 2 * D:] = 0.5, rng.uniform(0.1, 0.5, (n_out, D)) / D
    return kp


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def general_model(kp, noise, Zh, Yh, dev):
    """a model on the general-family route with these packed parameters"""
    from safe_exploration_amd import SimpleGPModel
    n_out, D = kp.shape[0], Zh.shape[1]
    gp = SimpleGPModel(n_out, D - 1, 1, kern_types=["lin_rbf"] * n_out, hyp=[{"noise_variance": noise}] * n_out, device=dev)
    gp._pack_kernel_params = lambda only=None: kp if only is None else kp[only:only + 1]
    gp.train(Zh, Yh, opt_hyp=False)
    return gp


def step(k):
    from safe_exploration_amd import SimpleGPModel
    N, n_out, D, T, reps, treps = SHAPES[k]
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(N + T)
    Zh = rng.uniform(-1, 1, (N, D))
    Yh = np.sin(2 * Zh.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.05 * rng.standard_normal((N, n_out))
    m = torch.as_tensor(Zh[rng.integers(0, N, T)] + 0.2 * rng.standard_normal((T, D)), device=dev)
    g = torch.as_tensor(0.25 * rng.standard_normal((T, D, 2)) / np.sqrt(D), device=dev)
    S = g.matmul(g.transpose(1, 2))
    kps = {kind: packed(rng, D, n_out, kind) for kind in ("rbf", "dense", "lin_rbf")}
    hyp = [{"lengthscale": 1.0 / kps["rbf"][o, 3:3 + D], "variance": 1.0, "noise_variance": 1e-2} for o in range(n_out)]
    rbf = SimpleGPModel(n_out, D - 1, 1, kern_types=["rbf"] * n_out, hyp=hyp, device=dev)
    rbf.train(Zh, Yh, opt_hyp=False)
    rbf.inv_K_device()
    torch.cuda.synchronize()
    base = timed(lambda: rbf.moment_match_device(m, S), 2, reps)
    ref = rbf.moment_match_device(m, S)
    line = "N=%d n_out=%d D=%d T=%d: ARD-RBF route %.3f ms" % (N, n_out, D, T, base)
    Z = torch.as_tensor(Zh, device=dev)
    for kind in ("rbf", "dense", "lin_rbf"):
        gp = general_model(kps[kind], 1e-2, Zh, Yh, dev)
        gp.inv_K_device()
        torch.cuda.synchronize()
        ms = timed(lambda: gp.moment_match_device(m, S), 2, reps)
        got = gp.moment_match_device(m, S)
        line += "; %s on the general route %.3f ms (x%.2f)" % ("a=0 b=0 c0=1" if kind == "rbf" else kind, ms, ms / base)
        if kind == "rbf":
            line += " max|general - ARD-RBF| mu %.1e cov %.1e V %.1e" % tuple(float((x - y).abs().max()) for x, y in zip(got, ref))
        if kind == "dense":
            args = (torch.as_tensor(kps[kind], device=dev), Z, gp.export_alpha(), gp.inv_K_device(), m, S)
            tref = torch_mm_gen(*args)
            tms = timed(lambda: torch_mm_gen(*args), 1, treps)
            line += " torch fp64 %.3f ms (x%.1f of the kernels) max|kernels - torch| mu %.1e cov %.1e V %.1e" % (
                (tms, tms / ms) + tuple(float((x - y).abs().max()) for x, y in zip(got, tref)))
    print(line, flush=True)


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
    for k in range(len(SHAPES)):
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(k)], capture_output=True, text=True,
                                 timeout=STEP_TIMEOUT)
        except subprocess.TimeoutExpired:
            print("step %d ran out of time (%d s): stopping" % (k, STEP_TIMEOUT), flush=True)
            return 1
        print(res.stdout, end="", flush=True)
        if res.returncode != 0:
            print(res.stderr[-2000:], flush=True)
            print("step %d failed with status %d: stopping" % (k, res.returncode), flush=True)
            return 1
        if out:
            out.write(res.stdout)
            out.flush()
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        step(int(sys.argv[2]))
    else:
        sys.exit(main())
