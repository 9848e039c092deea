"""The fused moment-matching roll-out (sr_gp_moment_match_rollout), the part that needs no GPU.

1. The two independent references the tree has -- ``_mm_ref.propagate`` (NumPy, the textbook closed form) and
   ``_mm_grad_ref.propagate_torch`` (its torch port with ``torch.linalg``) -- are held against each other on the very inputs of
   tests/test_gpu_moment_match_rollout.py (tests/_mm_rollout_cases.py; the model fitted in NumPy; for the sparse case the exact
   model on its inducing rows stands in).  Their disagreement must stay within ONE TENTH of every bar the GPU test uses: end to
   end rtol 1e-8, atol 1e-12 (the cases the GPU test holds end to end); per step, from the same state, mu+ rtol 1e-10 +
   1e-12 sigma_f |alpha|_1, Sigma+ and Cov rtol 1e-8 + 1e-9 max sf2 (every case).
   Observed shares of the bar (worst element): end to end at most 2.6e-2 (width-4; start-point-shared 2.5e-2, cartpole
   8.1e-4), per step at most 9.4e-3 (size-1024, Cov).  At noise 1e-2 the starts-and-gains models and the cart-pole shape
   reached 0.14 - 0.39 end to end (|alpha|_1 grows as 1 / noise against the mean's atol of 1e-12): those cases have noise 5e-2.
2. The entry is part of the C-ABI: declared in the header with its contract, exported by the cross-compiled library, bound in
   _lib.py; the Python surface has the agreed signatures; an untrained model raises before any device is touched; the
   per-step route keeps its parameter lists.

Every test here fails on the parent commit: the cases module, the symbol and the two functions do not exist there."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import _mm_ref as R
import _mm_grad_ref as GR
import _mm_rollout_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _share(got, ref, bar):
    return float(np.max(np.abs(np.asarray(got) - np.asarray(ref)) / bar))


@pytest.mark.parametrize("name", sorted(C.SPECS))
def test_references_agree_within_a_tenth_of_the_bars(name):
    import torch
    c = C.build(name)
    arrs = C.host_arrays(c)
    t = lambda x: None if x is None else torch.as_tensor(np.asarray(x, dtype=np.float64))
    model = tuple(t(x) for x in arrs)
    tz = C.tz_of(c)
    worst_e2e = worst_step = 0.0
    for tr in range(min(c["T"], 4)):                     # (cartpole-8 repeats the cart-pole model: four of its eight)
        kff, kfb = C.gains(c, tr)
        s0 = None if c["sigma0"] is None else c["sigma0"][tr]
        ref = R.propagate(*arrs, c["mu0"][tr], kff, kfb, c["a"], c["b"], s0, tz)
        tor = GR.propagate_torch(model, t(c["mu0"][tr]), t(kff), t(kfb), t(c["a"]), t(c["b"]), t(s0), t(tz))
        if c["e2e"]:
            worst_e2e = max([worst_e2e] + [_share(y.numpy(), x, C.e2e_bar(x)) for x, y in zip(ref, tor)])
        # per step, both from the NumPy reference's state
        mu, sig = c["mu0"][tr], s0
        for i in range(c["H"]):
            K = None if i == 0 else kfb[i - 1]
            rm, rs, rc = R.step(*arrs, mu, sig, kff[i], K, c["a"], c["b"], tz)
            tm, ts, tc = GR.step_torch(model, t(mu), t(sig), t(kff[i]), t(K), t(c["a"]), t(c["b"]), t(tz))
            bm, bs = C.step_bars(arrs, rm, rs)
            _, bc = C.step_bars(arrs, rm, rc)
            worst_step = max(worst_step, _share(tm.numpy(), rm, bm), _share(ts.numpy(), rs, bs), _share(tc.numpy(), rc, bc))
            mu, sig = rm, rs
    print("references %s: end to end %.1e of the bar, per step %.1e" % (name, worst_e2e, worst_step))
    assert worst_e2e <= 0.1 and worst_step <= 0.1, (name, worst_e2e, worst_step)


DECL = (r"int sr_gp_moment_match_rollout\(sr_gp_t h, long T, int H, int n_x_in, int gains_per_traj,\s+"
        r"const double\* mu0, const double\* sigma0, const double\* k_ff, const double\* k_fb,\s+"
        r"const double\* a, const double\* b, const double\* tz, const double\* inv_k,\s+"
        r"double\* mu_all, double\* sigma_all, double\* cov_all, void\* stream\);")


def test_rollout_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT sr_gp_moment_match_rollout$", out, re.M), "libsafereach.so does not export the entry"
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    m = re.search(DECL, hdr)
    assert m, "include/safereach.h does not declare sr_gp_moment_match_rollout as agreed"
    head = hdr[:m.start()].rstrip()
    assert head.endswith("*/")
    doc = head[head.rindex("/*"):]
    assert doc.startswith("/* sr_gp_moment_match_rollout:")
    for word in ("gains_per_traj", "k_fb [T x] (H - 1) x n_u x n_s", "mu_all T x H x n_s", "cov_all", "exactly symmetric",
                 "SR_EINVAL", "SR_ESTATE", "SR_EUNSUPPORTED", "N > 1024", "per-step route", "sr_gp_set_chunk", "`stream`"):
        assert word in doc, word
    from safe_exploration_amd import _lib
    P, I, L, H = _lib._P, _lib._I, _lib._L, _lib._H
    assert hasattr(_lib.lib, "sr_gp_moment_match_rollout")
    assert _lib.SIGNATURES["sr_gp_moment_match_rollout"] == (ctypes.c_int, [H, L, I, I, I] + [P] * 12)


def test_python_surface(lib_built):
    from safe_exploration_amd import SimpleGPModel, uncertainty_propagation_casadi as up
    sig = inspect.signature(SimpleGPModel.moment_match_rollout_device)
    assert list(sig.parameters) == ["self", "mu0", "k_ff", "k_fb", "a", "b", "sigma0", "a_gp_inp_x", "with_cov"]
    assert [sig.parameters[n].default for n in ("sigma0", "a_gp_inp_x", "with_cov")] == [None, None, True]
    sig = inspect.signature(up.moment_matching_rollout_batch)
    batch = inspect.signature(up.moment_matching_batch)
    assert list(sig.parameters) == [n for n in batch.parameters if n != "differentiable"]
    assert all(sig.parameters[n].default == batch.parameters[n].default for n in sig.parameters)
    assert "moment_matching_batch" in up.moment_matching_rollout_batch.__doc__
    # the per-step route is what it was
    assert list(batch.parameters) == ["mu_0", "ssm", "k_ff", "k_fb", "a", "b", "sigma_0", "a_gp_inp_x", "differentiable"]
    assert list(inspect.signature(up._mm_step).parameters) == ["ssm", "mu", "sigma", "kff", "K", "ta", "tb", "tz",
                                                               "differentiable"]
    assert list(inspect.signature(up.multi_step_moment_matching).parameters) == [
        "mu_0", "ssm", "k_ff", "k_fb", "sigma_0", "a", "b", "a_gp_inp_x"]


def test_untrained_model_raises_before_any_device(lib_built):
    from safe_exploration_amd import SimpleGPModel, uncertainty_propagation_casadi as up
    gp = SimpleGPModel(2, 2, 1)
    kff, kfb = np.zeros((1, 3, 1)), np.zeros((1, 2, 1, 2))
    with pytest.raises(RuntimeError):
        gp.moment_match_rollout_device(np.zeros((1, 2)), kff, kfb, np.eye(2), np.zeros((2, 1)))
    with pytest.raises(RuntimeError):
        up.moment_matching_rollout_batch(np.zeros((1, 2)), gp, kff, kfb)
    assert gp._handle is None
