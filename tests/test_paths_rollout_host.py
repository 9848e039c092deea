"""The fused closed-loop roll-out of the posterior function samples (sr_gp_paths_rollout) is part of the C-ABI: declared in
the header with its contract paragraph, exported by the cross-compiled library, bound in _lib.py; the Python surface
(SimpleGPModel.paths_rollout_device, MonteCarloSafetyVerification.rollout_paths) has the agreed signatures, an untrained model
raises before any device is touched, and sample_n_step keeps its parameter list.  Runs without a GPU.

Every test here fails on the parent commit: the symbol and the two methods do not exist there."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DECL = (r"int sr_gp_paths_rollout\(sr_gp_t h, const double\* x0, int x0_per_path, int H, const double\* k_fb, "
        r"const double\* k_ff,\s+double\* X_all, double\* A_all, void\* stream\);")


def test_rollout_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT sr_gp_paths_rollout$", out, re.M), "libsafereach.so does not export sr_gp_paths_rollout"
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    m = re.search(DECL, hdr)
    assert m, "include/safereach.h does not declare sr_gp_paths_rollout"
    # the contract paragraph: the comment that ends right in front of the declaration, at most eight lines
    head = hdr[:m.start()].rstrip()
    assert head.endswith("*/")
    doc = head[head.rindex("/*"):]
    assert doc.startswith("/* sr_gp_paths_rollout:") and doc.count("\n") + 1 <= 8
    for word in ("x0_per_path", "k_fb H x n_u x n_s", "X_all H x S x n_s", "A_all", "J_x + J_u k_fb[i]", "SR_EINVAL", "SR_ESTATE",
                 "SR_EUNSUPPORTED", "`stream`"):
        assert word in doc, word
    from safe_exploration_amd import _lib
    P, I, H = _lib._P, _lib._I, _lib._H
    assert hasattr(_lib.lib, "sr_gp_paths_rollout")
    assert _lib.SIGNATURES["sr_gp_paths_rollout"] == (ctypes.c_int, [H, P, I, I, P, P, P, P, P])


def test_python_surface(lib_built):
    from safe_exploration_amd import SimpleGPModel
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    sig = inspect.signature(SimpleGPModel.paths_rollout_device)
    assert list(sig.parameters) == ["self", "x0", "K", "k", "jacobians"]
    assert sig.parameters["jacobians"].default is False
    sig = inspect.signature(MonteCarloSafetyVerification.rollout_paths)
    assert list(sig.parameters) == ["self", "x0", "K", "k", "n", "n_samples", "generator", "as_tensor", "n_features", "jacobians"]
    assert [sig.parameters[n].default for n in ("n", "n_samples", "generator", "as_tensor", "n_features", "jacobians")] == \
        [1, 1000, None, False, 1024, False]
    # the route it stands beside is what it was (tests/test_paths_host.py, tests/test_paths_grad_host.py pin the same lists)
    assert list(inspect.signature(MonteCarloSafetyVerification.sample_n_step).parameters) == [
        "self", "x0", "K", "k", "n", "n_samples", "eps", "generator", "as_tensor", "consistent", "n_features"]
    assert list(inspect.signature(MonteCarloSafetyVerification.sample_n_step_jacobians).parameters) == [
        "self", "x0", "K", "k", "n", "n_samples", "generator", "as_tensor", "consistent", "n_features"]
    assert list(inspect.signature(SimpleGPModel.paths_step_device).parameters) == ["self", "x_s", "k_fb", "k_ff", "jacobians"]


def test_untrained_model_raises_before_any_device(lib_built):
    from safe_exploration_amd import SimpleGPModel
    from safe_exploration_amd.sampling_models import MonteCarloSafetyVerification
    gp = SimpleGPModel(2, 2, 1)
    K, k = np.zeros((3, 1, 2)), np.zeros((3, 1))
    with pytest.raises(RuntimeError):
        gp.paths_rollout_device(np.zeros(2), K, k)
    with pytest.raises(RuntimeError):
        gp.paths_rollout_device(np.zeros(2), K, k, jacobians=True)
    with pytest.raises(RuntimeError):
        MonteCarloSafetyVerification(gp).rollout_paths(np.zeros((2, 1)), K, k, n=3, n_samples=8)
    assert gp._handle is None
