"""The greedy max-variance selection by pivoted Cholesky downdates (sr_gp_select_maxvar) is part of the C-ABI: declared in
the header with the documented signature, exported by the cross-compiled library, bound in _lib.py with all nine
arguments; and choose_datapoints_maxvar takes route= / return_scores= with the argument checks that need no device.
Runs without a GPU."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_maxvar_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT sr_gp_select_maxvar$", out, re.M), "libsafereach.so does not export sr_gp_select_maxvar"
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    assert re.search(r"int sr_gp_select_maxvar\(sr_gp_t h, const double\* X, long n, int m, const int\* init_idx, int k,"
                     r"\s+int\* idx, double\* score, void\* stream\);", hdr)
    from safe_exploration_amd import _lib
    assert "sr_gp_select_maxvar" in _lib.SIGNATURES
    restype, args = _lib.SIGNATURES["sr_gp_select_maxvar"]
    assert restype is ctypes.c_int
    assert len(args) == 9
    assert args == [_lib._H, _lib._P, _lib._L, _lib._I, _lib._P, _lib._I, _lib._P, _lib._P, _lib._P]


def test_choose_datapoints_route_arguments(lib_built):
    from safe_exploration_amd import SimpleGPModel
    params = inspect.signature(SimpleGPModel.choose_datapoints_maxvar).parameters
    assert params["route"].default is None and params["return_scores"].default is False
    gp = SimpleGPModel(2, 2, 1)
    assert gp._select_route == "predict"                   # the default stays the predict route
    with pytest.raises(ValueError):
        gp.set_select_route("bogus")
    gp.set_select_route("downdate")
    assert gp._select_route == "downdate" and SimpleGPModel(2, 2, 1)._select_route == "predict"
    rng = np.random.default_rng(0)
    x, y = rng.uniform(-1, 1, (20, 3)), rng.standard_normal((20, 2))
    with pytest.raises(ValueError):
        gp.choose_datapoints_maxvar(x, y, 5, init_idx=[0, 1], route="bogus")
    with pytest.raises(ValueError):
        gp.choose_datapoints_maxvar(x, y, 5, init_idx=[0, 1], route="predict", return_scores=True)
    for bad in ([0, 0], [0, 20], [-1, 3]):                 # checked before anything touches a device
        with pytest.raises(ValueError):
            gp.choose_datapoints_maxvar(x, y, 5, init_idx=bad, route="downdate")
    # no more rows than m: everything, no selection and no scores
    xs, ys, idx, sc = gp.choose_datapoints_maxvar(x, y, 20, route="downdate", return_index=True, return_scores=True)
    np.testing.assert_array_equal(xs, x)
    np.testing.assert_array_equal(idx, np.arange(20))
    assert sc is None
