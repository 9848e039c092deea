"""The batched second-order linearisation (sr_gp_linearize_batch) is part of the C-ABI: declared in the header with the
documented signature, exported by the cross-compiled library, bound in _lib.py with all nine arguments.  Runs without
a GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_linearize_batch_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT sr_gp_linearize_batch$", out, re.M), "libsafereach.so does not export sr_gp_linearize_batch"
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    assert re.search(r"int sr_gp_linearize_batch\(sr_gp_t h, const double\* Xq, long T, double\* mu, double\* var,\s+"
                     r"double\* jac_mu, double\* jac_var, double\* hess_mu, void\* stream\);", hdr)
    from safe_exploration_amd import _lib
    assert "sr_gp_linearize_batch" in _lib.SIGNATURES
    restype, args = _lib.SIGNATURES["sr_gp_linearize_batch"]
    assert len(args) == 9
    assert args == _lib.SIGNATURES["sr_gp_predict_grad"][1][:7] + [_lib.SIGNATURES["sr_gp_predict_grad"][1][7]] * 2
