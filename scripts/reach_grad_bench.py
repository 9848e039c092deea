"""Times of the reverse pass of one reachability step (sr_onestep_reach_vjp) and of a full backward through a differentiable
H = 15 roll-out, each beside (a) the forward call, (b) torch autograd through a batched torch-fp64 port of the step fed by
linearize_device_batch (the GP enters the port by its second-order expansion at z, so autograd returns the same gradient),
(c) the 2 (n_u + n_u n_s) forward calls of central differences in the controls of one step, run back to back.

    python scripts/reach_grad_bench.py [OUT]        (default OUT: profiles/r15_reach_grad.txt)

One run measures every side; times are medians of five batches (scripts/_timing.timeit)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from _timing import timeit                                                         # noqa: E402
from safe_exploration_amd import SimpleGPModel, gp_reachability as reach          # noqa: E402


def model(N, n_s, n_u, seed=0):
    rng = np.random.default_rng(seed)
    D = n_s + n_u
    Z = rng.uniform(-1, 1, (N, D))
    Y = 0.2 * np.sin(2.0 * Z.dot(rng.standard_normal((D, n_s)) / np.sqrt(D))) + 0.01 * rng.standard_normal((N, n_s))
    hyp = [{"lengthscale": rng.uniform(0.6, 1.4, D) * np.sqrt(D / 3.0), "variance": 0.05, "noise_variance": 1e-2}
           for _ in range(n_s)]
    gp = SimpleGPModel(n_s, n_s, n_u, kern_types=["rbf"] * n_s, hyp=hyp)
    gp.train(Z, Y, opt_hyp=False)
    return gp


def torch_step(p, q, u, k, lin, z0, a, b, l_mu, l_sigma, c):
    """the ellipsoid step of T queries in batched torch; the GP by its expansion (mu, var, jac_mu, jac_var, hess_mu) at z0"""
    mu0, var0, jm, jv, hm = lin
    n_s = p.shape[1]
    q = (q + q.transpose(1, 2)) / 2                      # as the device reads it (eigvalsh alone would read one triangle)
    dz = torch.cat((p, u), dim=1) - z0
    mu = mu0 + torch.einsum('tad,td->ta', jm, dz)
    var = var0 + torch.einsum('tad,td->ta', jv, dz)
    jac = jm + torch.einsum('tade,te->tad', hm, dz)
    p1 = p @ a.T + u @ b.T + mu
    h = a + jac[:, :, :n_s] + (jac[:, :, n_s:] + b) @ k
    q0 = h @ q @ h.transpose(1, 2)
    l = torch.linalg.cholesky(torch.eye(n_s, dtype=q.dtype, device=q.device) + k.transpose(1, 2) @ k)
    r2 = torch.linalg.eigvalsh(l.transpose(1, 2) @ q @ l)[:, -1:]
    d_s = n_s * (c * (torch.sqrt(var) + l_sigma * torch.sqrt(r2))) ** 2
    d_m = n_s * (l_mu * r2) ** 2
    c1 = torch.sqrt(d_s.sum(1, keepdim=True) / d_m.sum(1, keepdim=True))
    d_l = (1 + 1 / c1) * d_s + (1 + c1) * d_m
    c2 = torch.sqrt(d_l.sum(1) / torch.diagonal(q0, dim1=1, dim2=2).sum(1))[:, None, None]
    return p1, (1 + c2) * q0 + torch.diag_embed((1 + 1 / c2[:, :, 0]) * d_l)


def regime(out, name, N, n_s, n_u, T, H=15, n=100):
    gp = model(N, n_s, n_u)
    dev = gp.device
    rng = np.random.default_rng(1)
    t = lambda x: torch.as_tensor(np.ascontiguousarray(x), device=dev)
    A = rng.standard_normal((T, n_s, n_s))
    p, u = t(0.3 * rng.standard_normal((T, n_s))), t(0.2 * rng.standard_normal((T, n_u)))
    q, k = t(0.02 * np.einsum('tij,tkj->tik', A, A) / n_s), t(0.3 * rng.standard_normal((T, n_u, n_s)))
    pb, qb = t(rng.standard_normal((T, n_s))), t(rng.standard_normal((T, n_s, n_s)))
    a_np, b_np = 0.9 * np.eye(n_s), 0.1 * rng.standard_normal((n_s, n_u))
    l_np, c = np.full(n_s, 0.03), 1.7
    a, b, l = t(a_np), t(b_np), t(l_np)
    z0 = torch.cat((p, u), dim=1)
    fwd = timeit(lambda: reach.onestep_reachability_batch(p, gp, u, l_np, l_np, q, k, c, a_np, b_np), n=n)
    rev = timeit(lambda: reach.onestep_reachability_vjp_batch(p, gp, u, l_np, l_np, pb, qb, q, k, c, a_np, b_np), n=n)
    lin_t = timeit(lambda: gp.linearize_device_batch(z0), n=n)

    def torch_route():
        lin = gp.linearize_device_batch(z0)
        leaves = [x.detach().requires_grad_(True) for x in (p, q, u, k)]
        p1, q1 = torch_step(leaves[0], leaves[1], leaves[2], leaves[3], lin, z0, a, b, l, l, c)
        return torch.autograd.grad((p1 * pb).sum() + (q1 * qb).sum(), leaves)

    tor = timeit(torch_route, n=max(5, n // 10))
    got = reach.onestep_reachability_vjp_batch(p, gp, u, l_np, l_np, pb, qb, q, k, c, a_np, b_np)
    agree = max(float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, torch_route()))
    n_fd = 2 * (n_u + n_u * n_s)

    def central_differences():
        for _ in range(n_fd):
            reach.onestep_reachability_batch(p, gp, u, l_np, l_np, q, k, c, a_np, b_np)

    fd = timeit(central_differences, n=max(5, n // 10))
    out.append("  %-34s fwd %8.1f us   vjp %8.1f us (%.2f fwd)   linearize_batch %8.1f us (%.0f %% of vjp)   torch port %9.1f us "
               "(%.1f vjp)   %d fwd calls of central differences %9.1f us (%.1f vjp)   vjp vs torch %.1e"
               % (name, fwd, rev, rev / fwd, lin_t, 100 * lin_t / rev, tor, tor / rev, n_fd, fd, fd / rev, agree))
    # roll-out of H steps: forward alone (the library's own route), and forward + backward of the differentiable roll-out
    Tr = T
    p0 = p
    kff = t(0.2 * rng.standard_normal((Tr, H, n_u))).requires_grad_(True)
    kfb = t(0.3 * rng.standard_normal((Tr, H - 1, n_u, n_s))).requires_grad_(True)
    wp, wq = t(rng.standard_normal((Tr, H, n_s))), t(rng.standard_normal((Tr, H, n_s, n_s)))
    roll = timeit(lambda: reach.multistep_reachability_batch(p0, gp, kfb.detach(), kff.detach(), l_np, l_np, None, c, a_np, b_np),
                  n=max(10, n // 5), warmup=3)

    def diff_roll():
        pa, qa = reach.multistep_reachability_batch(p0, gp, kfb, kff, l_np, l_np, None, c, a_np, b_np, differentiable=True)
        return torch.autograd.grad((pa * wp).sum() + (qa * wq).sum(), (kff, kfb))

    both = timeit(diff_roll, n=max(10, n // 5), warmup=3)
    n_fd_roll = 2 * H * (n_u + n_u * n_s)
    out.append("  %-34s roll-out H=%d of %d: forward %8.1f us   differentiable forward + backward %9.1f us (%.1f fwd)   "
               "central differences in its controls: %d forward roll-outs (%.1f ms at the forward's time, not run)"
               % ("", H, Tr, roll, both, both / roll, n_fd_roll, n_fd_roll * roll / 1e3))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r15_reach_grad.txt")
    out = ["sr_onestep_reach_vjp and the backward of a differentiable roll-out -- time per call, 1 x MI355X",
           "(scripts/reach_grad_bench.py; medians of five batches, host clock around synchronised batches of calls on device tensors)",
           ""]
    regime(out, "cart-pole N=150 n_s=4 n_u=1 T=256", 150, 4, 1, 256)
    regime(out, "cart-pole N=150 n_s=4 n_u=1 T=3840", 150, 4, 1, 3840)
    regime(out, "N=5000 n_s=2 n_u=1 T=4096", 5000, 2, 1, 4096, n=20)
    text = "\n".join(out) + "\n"
    print(text)
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
