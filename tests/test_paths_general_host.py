"""Posterior function samples of the general kernel family with the RBF radial part: the NumPy reference the GPU tests
compare with (tests/_paths_gen_ref.py) has the properties the algebra promises, and sr_gp_paths_weight_count is part of the
C-ABI (declared, exported, bound).  Runs without a GPU.

Bars: the Gram matrix of M = 4 10^5 features against k, every entry within 5 sqrt(k(x,x) k(y,y) / M) (a Monte-Carlo mean of
M terms, each bounded by 2 sqrt(k(x,x) k(y,y)) in the group it belongs to: five standard errors; fixed seed); the Jacobians
against central differences with h = 1e-5 within 1e-6 max|J| (truncation h^2 f''' / 6 ~ 1e-9 max|J| at these lengthscales,
rounding 1e-16 |f| / h ~ 1e-11 |f|); an "rbf" output packed into the family against tests/_paths_ref.py: the features bit for
bit where 1 / l is exact, the paths within that reference's own rule max(20 e0, 1e-12 scale sqrt(N + M)).

On the parent commit the module does not import (tests/_paths_gen_ref.py is new with it); of its tests only
test_weight_count_exported_declared_bound depends on the library's change, the others hold the new NumPy reference."""
import ctypes
import os
import re
import subprocess

import numpy as np

from oracle import oracle_np as orc
import _paths_ref as pr
import _paths_gen_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kp(D, rows):
    """rows of (v, c0, s, a, b) -> packed parameters with kappa id 0"""
    kp = np.zeros((len(rows), 3 + 3 * D))
    for o, (v, c0, s, a, b) in enumerate(rows):
        kp[o, 1], kp[o, 2] = v, c0
        kp[o, 3:3 + D], kp[o, 3 + D:3 + 2 * D], kp[o, 3 + 2 * D:] = s, a, b
    return kp


# D = 3, two outputs whose active sets differ: groups {0, 2} and {2, 3} -> the handle's groups are [0, 2, 3]; one s_j = 0
KP3 = _kp(3, [(0.9, 0.7, [1.3, 0.8, 0.0], [0.0, 0.6, 0.0], [0.2, 0.0, 0.4]),
              (1.2, 0.0, [0.5, 1.1, 0.9], [0.0, 0.3, 0.8], [0.0, 0.5, 0.1])])


def test_groups_and_weight_count():
    assert gr.groups(KP3) == [0, 2, 3] and gr.weight_count(KP3, 100) == 303
    assert gr.groups(KP3[1:]) == [2, 3] and gr.weight_count(KP3[1], 7) == 17
    lin_rbf = _kp(4, [(1.0, 0.0, [0, 2.0, 0, 0], [0, 0.5, 0, 0], [0.1, 0.2, 0.3, 0.4])])
    assert gr.groups(lin_rbf) == [2] and gr.weight_count(lin_rbf, 64) == 68
    assert gr.groups(_kp(2, [(1.0, 0.0, [1, 1], [0, 0], [1, 1])])) == []


def test_feature_gram_matrix_tends_to_the_kernel():
    M, D = 400000, 3
    rng = np.random.default_rng(21)
    kp = KP3[:1].copy()
    kp[0, 3 + D] = 0.9                                    # a_1 too: two active groups beside c0 would be three; keep c0 = 0
    kp[0, 2] = 0.0
    assert gr.groups(kp) == [1, 2]
    omega, tau = rng.standard_normal((M, D)), rng.uniform(0, 2 * np.pi, M)
    x = rng.uniform(-1.5, 1.5, (6, D))
    P = gr.features(x, omega, tau, kp[0], gr.groups(kp))
    assert P.shape == (6, 2 * M + D)
    k = gr.kernel(x, x, kp[0])
    bound = 5.0 * np.sqrt(np.outer(np.diag(k), np.diag(k)) / M)
    err = np.abs(P.dot(P.T) - k)
    print("gram: max err %.3e, max err / bound %.3f" % (err.max(), (err / bound).max()))
    assert np.all(err <= bound)
    # the check can tell: without the groups' amplitudes the Gram matrix is that of another kernel
    Q = gr.features(x, omega, tau, kp[0], [])
    assert np.any(np.abs(Q.dot(Q.T) - k) > bound)


def _tiny(seed, N, M, S, kp):
    rng = np.random.default_rng(seed)
    D, n_out = (kp.shape[1] - 3) // 3, kp.shape[0]
    Z = rng.uniform(-1, 1, (N, D))
    Y = np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)))) + 0.05 * rng.standard_normal((N, n_out))
    n_w = gr.weight_count(kp, M)
    return dict(Z=Z, Y=Y, kp=kp, nd=np.full(n_out, 1e-2), omega=rng.standard_normal((M, D)), tau=rng.uniform(0, 2 * np.pi, M),
                w=rng.standard_normal((n_out, S, n_w)), eps=rng.standard_normal((n_out, S, N)), rng=rng)


def test_jacobians_against_central_differences():
    p = _tiny(3, 30, 20, 4, KP3)
    c = gr.coeffs(p["Z"], p["Y"], p["kp"], p["nd"], p["omega"], p["tau"], p["w"], p["eps"])
    args = (p["Z"], p["kp"], p["omega"], p["tau"], p["w"], c)
    x = p["rng"].uniform(-1.2, 1.2, (5, 3))
    xs = p["rng"].uniform(-1.2, 1.2, (4, 3))
    h = 1e-5
    for fn, gfn, q in ((gr.evaluate, gr.evaluate_grad, x), (gr.step, gr.step_grad, xs)):
        J = gfn(q, *args)
        fd = np.empty_like(J)
        for j in range(3):
            e = np.zeros(3)
            e[j] = h
            fd[..., j] = (fn(q + e, *args) - fn(q - e, *args)) / (2 * h)
        err = np.abs(J - fd).max()
        print("%s: max|J| %.3e, |J - fd| %.3e" % (gfn.__name__, np.abs(J).max(), err))
        assert err <= 1e-6 * np.abs(J).max()
    # the step is the diagonal of the evaluation
    np.testing.assert_allclose(gr.step(xs, *args), gr.evaluate(xs, *args)[np.arange(4), np.arange(4)], rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(gr.step_grad(xs, *args), gr.evaluate_grad(xs, *args)[np.arange(4), np.arange(4)], rtol=1e-12,
                               atol=1e-12)


def test_packed_rbf_output_equals_the_ard_reference():
    N, M, S, D = 40, 24, 3, 3
    rng = np.random.default_rng(4)
    sf2 = np.array([1.1, 0.8])
    for ls, exact in ((np.array([[0.5, 1.0, 2.0], [0.25, 0.5, 1.0]]), True), (rng.uniform(0.5, 1.0, (2, D)), False)):
        kp = _kp(D, [(sf2[d], 1.0, 1.0 / ls[d], np.zeros(D), np.zeros(D)) for d in range(2)])
        assert gr.groups(kp) == [0] and gr.weight_count(kp, M) == M + D
        p = _tiny(5, N, M, S, kp)
        x = p["rng"].uniform(-1.2, 1.2, (9, D))
        for d in range(2):
            P = gr.features(x, p["omega"], p["tau"], kp[d], [0])
            Pa = pr.features(x, p["omega"], p["tau"], ls[d], sf2[d])
            assert np.all(P[:, M:] == 0.0)
            if exact:
                np.testing.assert_array_equal(P[:, :M], Pa)
            else:
                np.testing.assert_allclose(P[:, :M], Pa, rtol=0, atol=1e-14)
        noise_var = p["nd"] - orc.GPY_JITTER
        wa = np.ascontiguousarray(p["w"][:, :, :M])
        ca = {r: pr.coeffs(p["Z"], p["Y"], ls, sf2, noise_var, p["omega"], p["tau"], wa, p["eps"], r) for r in ("chol", "lu")}
        Fa = {r: pr.evaluate(x, p["Z"], ls, sf2, p["omega"], p["tau"], wa, ca[r]) for r in ca}
        c = gr.coeffs(p["Z"], p["Y"], kp, p["nd"], p["omega"], p["tau"], p["w"], p["eps"])
        F = gr.evaluate(x, p["Z"], kp, p["omega"], p["tau"], p["w"], c)
        e0, scale = np.abs(Fa["chol"] - Fa["lu"]).max(), np.abs(Fa["chol"]).max()
        assert np.abs(F - Fa["chol"]).max() <= max(20 * e0, 1e-12 * scale * np.sqrt(N + M))


def test_zero_draws_give_the_posterior_mean(lib_built):
    """the in-tree "lin_rbf" and a mixed "rbf" / "lin_rbf" model, packed as the model class packs them"""
    from safe_exploration_amd import SimpleGPModel
    D, N = 3, 40
    rng = np.random.default_rng(6)
    for kts in (["lin_rbf", "lin_rbf"], ["rbf", "lin_rbf"]):
        hyp = [orc.make_hyp(kt, rng, D) for kt in kts]
        gp = SimpleGPModel(2, 2, 1, kern_types=kts, hyp=[dict(h, noise_variance=1e-2) for h in hyp])
        kp = gp._pack_kernel_params()
        assert gr.groups(kp) == ([2] if kts[0] == "lin_rbf" else [0, 2])
        p = _tiny(7, N, 16, 3, kp)
        x = p["rng"].uniform(-1.2, 1.2, (11, D))
        for d in range(2):
            np.testing.assert_allclose(gr.kernel(x, p["Z"], kp[d]), orc.kernel_matrix(kts[d], gp.hyp[d], x, p["Z"]), rtol=1e-13,
                                       atol=1e-15)
        beta, inv_K = orc.gp_fit_k(p["Z"], p["Y"], kts, gp.hyp, p["nd"] - orc.GPY_JITTER)
        mu = orc.gp_predict_k(x, p["Z"], beta, inv_K, kts, gp.hyp)[0]
        for route in ("chol", "lu"):
            c = gr.coeffs(p["Z"], p["Y"], kp, p["nd"], p["omega"], p["tau"], 0 * p["w"], 0 * p["eps"], route)
            F = gr.evaluate(x, p["Z"], kp, p["omega"], p["tau"], 0 * p["w"], c)
            for s in range(3):
                np.testing.assert_allclose(F[:, s, :], mu, rtol=1e-9, atol=1e-9 * np.abs(mu).max())
    assert gp._handle is None


def test_weight_count_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT sr_gp_paths_weight_count$", out, re.M), "libsafereach.so does not export sr_gp_paths_weight_count"
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    assert re.search(r"int sr_gp_paths_weight_count\(sr_gp_t h, int M, int\* n_w\);", hdr)
    doc = hdr[hdr.index("posterior FUNCTION samples"):hdr.index("int sr_gp_paths_draw(")]
    for word in ("sr_gp_paths_weight_count", "n_w = G M + D", "sqrt(a_l) x_l", "SR_EINVAL at the draw"):
        assert word in doc, word
    assert "general kernels" not in doc[doc.index("Out of scope"):]
    from safe_exploration_amd import _lib, SimpleGPModel
    assert _lib.SIGNATURES["sr_gp_paths_weight_count"] == (ctypes.c_int, [_lib._H, _lib._I, _lib._PI])
    assert hasattr(_lib.lib, "sr_gp_paths_weight_count") and callable(SimpleGPModel.paths_weight_count)
