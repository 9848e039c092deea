"""The batched predictive-variance gradient (sr_gp_predict_grad) is part of the C-ABI: declared in the header, exported by
the cross-compiled library, bound in _lib.py.  Runs without a GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_predict_grad_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT sr_gp_predict_grad$", out, re.M), "libsafereach.so does not export sr_gp_predict_grad"
    # the main-loop test entry lives in the lab build only
    assert "sr_test_gemm_nt" not in out
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    assert re.search(r"int sr_gp_predict_grad\(sr_gp_t h, const double\* Xq, long T, double\* mu, double\* var, "
                     r"double\* jac_mu,\s+double\* jac_var, void\* stream\);", hdr)
    from safe_exploration_amd import _lib
    assert "sr_gp_predict_grad" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sr_gp_predict_grad"][1]) == 8
