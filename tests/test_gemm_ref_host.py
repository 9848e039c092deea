"""The test entries of the TN GEMM family (sr_test_gemm_tn_ex, _upper_ex, _splitk, _jobs) are exported, declared and bound,
and refuse bad arguments with SR_EINVAL before they touch a device; the NumPy reference the GPU tests compare with
(tests/_gemm_ref.py) agrees with a direct evaluation under explicit masks.  Runs without a GPU.

The products here are evaluated in np.longdouble, as integers or by np.einsum, and in fp64 only at 128 x 128 x 16: none of
these starts the worker threads of the BLAS, which keep spinning for a while after a product and would count against a
later test that measures the CPU time of the process (test_host_logic.py: sr_wait_flag gives the core away)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _gemm_ref as gr

L = np.longdouble                            # 64-bit mantissa: exact on this data as well, and no BLAS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRIES = ("sr_test_gemm_tn_ex", "sr_test_gemm_tn_upper_ex", "sr_test_gemm_tn_splitk", "sr_test_gemm_tn_jobs")


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_reference_matches_masked_einsum(mode):
    """256 x 384 x 256: the block-wise reference against one einsum over DENSE integer operands with the mode's mask written out
    element by element (the operands are not shaped here: the masks alone must carry the semantics)."""
    M, N, K = 256, 384, 256
    rng = np.random.default_rng(40 + mode)
    A, B, C0 = gr.integers(rng, (K, M)), gr.integers(rng, (K, N)), gr.integers(rng, (M, N))
    alpha, beta = -0.5, 2.0
    gr.assert_exact(K, alpha, beta)
    k, m, n = np.arange(K)[:, None, None], np.arange(M)[None, :, None], np.arange(N)[None, None, :]
    m0, n0 = m // 128 * 128, n // 128 * 128
    keep = {0: k >= 0, 1: k >= 0, 2: k >= n0, 3: k < m0 + 128, 4: k >= m0}[mode]
    keep = np.broadcast_to(keep, (K, M, N))
    want = alpha * np.einsum("km,kn,kmn->mn", A, B, keep.astype(np.float64)) + beta * C0
    if mode == 1:
        lower = (n0 < m0)[0]
        want[lower] = C0[lower]
        assert not gr.written_blocks(M, N, mode)[lower].any() and gr.written_blocks(M, N, mode)[~lower].all()
    else:
        assert gr.written_blocks(M, N, mode).all()
    got = gr.gemm_tn(A, B, C0, alpha, beta, mode, dtype=L).astype(np.float64)
    np.testing.assert_array_equal(got, want)
    # the k ranges differ from the full one wherever the mode says so (the comparison above can tell a wrong range)
    if mode in (2, 3, 4):
        assert not np.array_equal(got, gr.gemm_tn(A, B, C0, alpha, beta, 0, dtype=L).astype(np.float64))


@pytest.mark.parametrize("mode", [2, 3, 4])
def test_shaped_operands_and_poison(mode):
    """Shaped operands: the mode's product equals the dense product (that is what the structure is for), the poisoned variant
    gives the reference of the zero variant, and the structure is element-wise inside the diagonal blocks."""
    M, N, K = 256, 384, 256
    rng = np.random.default_rng(50 + mode)
    Az, Bz = gr.operands(rng, M, N, K, mode, "Z")
    rng = np.random.default_rng(50 + mode)
    Ap, Bp = gr.operands(rng, M, N, K, mode, "P")
    X, Xp = (Bz, Bp) if mode == 2 else (Az, Ap)
    assert np.isnan(Xp).any() and not np.isnan(X).any()
    np.testing.assert_array_equal(np.nan_to_num(Xp, nan=0.0), X)
    k, w = np.arange(K)[:, None], np.arange(X.shape[1])[None, :]
    zero = (k > w) if mode == 3 else (k < w)                 # element-wise triangular as a whole
    assert (X[zero] == 0).all() and (X[~zero] != 0).all()
    assert np.isnan(Xp[(k // 128 > w // 128) if mode == 3 else (k // 128 < w // 128)]).all()
    C0 = gr.integers(rng, (M, N))
    Ai, Bi = Az.astype(np.int64), Bz.astype(np.int64)
    ref = gr.gemm_tn(Az, Bz, C0, 1.0, -1.0, mode, dtype=L).astype(np.float64)
    np.testing.assert_array_equal(ref, Ai.T @ Bi - C0)
    np.testing.assert_array_equal(gr.gemm_tn(Ap, Bp, C0, 1.0, -1.0, mode, dtype=L).astype(np.float64), ref)
    # a 64-granular k range (the job-table kernel on 64 x 64 tiles) sees the same numbers: what it skips in addition is zero
    if mode == 2:
        np.testing.assert_array_equal(Ai[64:, :].T @ Bi[64:, 64:128], ref[:, 64:128] + C0[:, 64:128])
    elif mode == 3:
        np.testing.assert_array_equal(Ai[:64, :64].T @ Bi[:64, :], ref[:64, :] + C0[:64, :])


def test_exactness_condition():
    gr.assert_exact(2048, gr.ALPHAS, gr.ALPHAS)
    with pytest.raises(AssertionError):
        gr.assert_exact(2 ** 33, 2.0, 0.0)                   # 2^33 * 10^6 * 2 > 2^53
    with pytest.raises(AssertionError):
        gr.assert_exact(16, 0.3, 0.0)                        # not one of ALPHAS: products would round
    # beta == 0 overwrites: a NaN prefill does not reach the result
    rng = np.random.default_rng(7)
    A, B = gr.integers(rng, (16, 128)), gr.integers(rng, (16, 128))
    exact = 2 * (A.astype(np.int64).T @ B.astype(np.int64))
    np.testing.assert_array_equal(gr.gemm_tn(A, B, np.full((128, 128), np.nan), 2.0, 0.0, 0), exact)        # (the fp64 path)
    np.testing.assert_array_equal(gr.gemm_tn(A, B, None, 2.0, 0.0, 0, dtype=L).astype(np.float64), exact)
    # the worst case of the data really is exact: all operands at the bound, summed one by one and by the BLAS
    K = 4096
    a = np.full((K, 1), -1000.0)
    b = np.full((K, 1), 1000.0)
    s = 0.0
    for i in range(K):
        s += a[i, 0] * b[i, 0]
    assert s == (a.T @ b)[0, 0] == -1e6 * K


def test_error_bound_and_windows():
    rng = np.random.default_rng(9)
    A, B = gr.operands(rng, 128, 128, 16, 0, real=True)
    C0 = rng.standard_normal((128, 128))
    exact = gr.gemm_tn(A, B, C0, -0.5, 2.0, 0, dtype=L)
    err = np.abs((-0.5 * (A.T @ B) + 2.0 * C0) - exact).astype(np.float64)
    bound = gr.error_bound(A, B, C0, -0.5, 2.0)
    assert (err <= bound).all() and bound.min() > 0
    X = gr.integers(rng, (5, 6))
    buf = gr.embed(X, ld=10, fill=np.nan, extra_rows=1)
    assert buf.size == gr.flat_len(6, 10)
    np.testing.assert_array_equal(gr.window(buf, 5, 6, 10), X)
    assert np.isnan(buf).sum() == buf.size - 30 and buf[gr.OFFSET] == X[0, 0] and buf[gr.OFFSET + 10] == X[1, 0]
    mask = np.zeros(buf.size, dtype=bool)                    # a window of a mask (one byte per element)
    gr.window(mask, 5, 6, 10)[...] = True
    assert mask.sum() == 30 and mask[gr.OFFSET] and mask[gr.OFFSET + 45] and not mask[gr.OFFSET + 46]
    assert gr.same_bits(np.array([np.nan, 1.0]), np.array([np.nan, 1.0])) and not gr.same_bits(np.array([0.0]), np.array([-0.0]))


# ------------------------------------------------------------------ the entries
def test_entries_exported_declared_bound(lib_built):
    so = os.path.join(ROOT, "safe_exploration_amd", "libsafereach.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    with open(os.path.join(ROOT, "include", "safereach.h")) as f:
        hdr = f.read()
    from safe_exploration_amd import _lib
    for name in ENTRIES + ("sr_test_gemm_tn", "sr_test_gemm_tn_upper"):
        assert re.search(r"\bT %s$" % name, out, re.M), "libsafereach.so does not export %s" % name
        assert re.search(r"^int %s\(int device, " % name, hdr, re.M), "include/safereach.h does not declare %s" % name
        assert hasattr(_lib.lib, name) and _lib.SIGNATURES[name][0] is ctypes.c_int
    P, I, L, D = _lib._P, _lib._I, _lib._L, _lib._D
    assert _lib.SIGNATURES["sr_test_gemm_tn_ex"][1] == [I, P, L, P, L, P, L, I, I, I, D, D, I, I, I, L, L, L, P]
    assert _lib.SIGNATURES["sr_test_gemm_tn_upper_ex"][1] == [I, P, L, P, L, P, L, I, I, I, D, D, I, I, I, L, L, L, P]
    assert _lib.SIGNATURES["sr_test_gemm_tn_splitk"][1] == [I, P, L, P, L, P, I, I, I, I, D, I, P, L, P]
    assert _lib.SIGNATURES["sr_test_gemm_tn_jobs"][1] == [I, P, L, P, L, P, L, P, L, L, P, I, I, I, L, D, I, I, L, L, L, L, P]
    # the old entries keep their signatures (scripts use them)
    assert _lib.SIGNATURES["sr_test_gemm_tn"][1] == [I, P, L, P, L, P, L, I, I, I, D, D, I, P]
    assert _lib.SIGNATURES["sr_test_gemm_tn_upper"][1] == [I, P, L, P, L, P, L, I, I, I, D, D, I, P]
    assert re.search(r"typedef struct sr_gemm_job \{ long a, b, c, ct; int M, N, K, pad; \} sr_gemm_job;", hdr)


class Job(ctypes.Structure):
    _fields_ = [("a", ctypes.c_long), ("b", ctypes.c_long), ("c", ctypes.c_long), ("ct", ctypes.c_long),
                ("M", ctypes.c_int), ("N", ctypes.c_int), ("K", ctypes.c_int), ("pad", ctypes.c_int)]


# Pointers that are never dereferenced: every call below must be refused by the argument checks, which come before the
# device is selected (no GPU here: a call that got past them would answer SR_EHIP, not SR_EINVAL).
_PTR = ctypes.c_void_p(1 << 20)
_ODD = ctypes.c_void_p((1 << 20) + 8)


def _refused(rc, word):
    from safe_exploration_amd import _lib
    assert rc == _lib.SR_EINVAL, "code %d: %s" % (rc, _lib.last_error())
    assert word in _lib.last_error(), _lib.last_error()


def test_plain_and_upper_entries_refuse_bad_arguments(lib_built):
    from safe_exploration_amd._lib import lib
    for f, name, mo in ((lib.sr_test_gemm_tn_ex, "sr_test_gemm_tn_ex", 0), (lib.sr_test_gemm_tn_upper_ex, "sr_test_gemm_tn_upper_ex", 0)):
        def call(A=_PTR, lda=136, B=_PTR, ldb=264, C=_PTR, ldc=264, M=128, N=256, K=32, mo=mo, prio=0, n=1, sA=0, sB=0, sC=0):
            return f(0, A, lda, B, ldb, C, ldc, M, N, K, 1.0, 0.0, mo, prio, n, sA, sB, sC, None)
        _refused(call(A=None), name + ": NULL")
        _refused(call(B=None), "NULL")
        _refused(call(C=None), "NULL")
        _refused(call(M=100), "M=100")
        _refused(call(N=192), "N=192")
        _refused(call(K=24), "K=24")
        _refused(call(K=0), "K=0")
        _refused(call(lda=137), "lda=137")                   # odd
        _refused(call(ldb=265), "ldb=265")
        _refused(call(lda=126), "lda=126")                   # below M
        _refused(call(ldc=255), "ldc=255")                   # below N (odd or even: C is stored element-wise)
        _refused(call(ldc=254), "ldc=254")
        _refused(call(A=_ODD), "aligned")
        _refused(call(n=0), "n=0")
        _refused(call(n=2, sA=33, sB=64, sC=1 << 16), "batch")
        _refused(call(n=2, sA=64, sB=64, sC=100), "overlap")
    _refused(lib.sr_test_gemm_tn_ex(0, _PTR, 136, _PTR, 264, _PTR, 264, 128, 256, 32, 1.0, 0.0, 5, 0, 1, 0, 0, 0, None), "mode=5")
    _refused(lib.sr_test_gemm_tn_upper_ex(0, _PTR, 264, _PTR, 136, _PTR, 136, 256, 128, 32, 1.0, 0.0, 0, 0, 1, 0, 0, 0, None),
             "M=256 N=128")                                  # the upper form needs M <= N
    _refused(lib.sr_test_gemm_tn_upper_ex(0, _PTR, 136, _PTR, 264, _PTR, 264, 128, 256, 32, 1.0, 0.0, 2, 0, 1, 0, 0, 0, None),
             "order=2")


def test_splitk_entry_refuses_bad_arguments(lib_built):
    from safe_exploration_amd._lib import lib

    def call(A=_PTR, lda=264, B=_PTR, ldb=136, C=_PTR, M=256, N=128, K=640, ks=256, mode=0, part=_PTR, part_len=3 * 256 * 128):
        return lib.sr_test_gemm_tn_splitk(0, A, lda, B, ldb, C, M, N, K, ks, 1.0, mode, part, part_len, None)
    _refused(call(M=100), "M=100")
    _refused(call(lda=265), "lda=265")
    _refused(call(ldb=120), "ldb=120")
    _refused(call(ks=100), "ks=100")
    _refused(call(ks=0), "ks=0")
    _refused(call(part=None), "part NULL")
    _refused(call(C=None), "NULL")
    _refused(call(part_len=3 * 256 * 128 - 1), "3 slices")   # ceil(640 / 256) = 3
    _refused(call(ks=128, part_len=4 * 256 * 128), "5 slices")
    _refused(call(mode=7), "mode=7")


def test_jobs_entry_refuses_bad_arguments(lib_built):
    from safe_exploration_amd._lib import lib
    ld = 392
    ok = dict(a=0, b=0, c=0, ct=0, M=256, N=384, K=128, pad=0)
    lens = dict(lenA=127 * ld + 256, lenB=127 * ld + 384, lenC=255 * ld + 384, lenCT=383 * ld + 256)

    def call(job=None, njobs=1, ld=ld, maxM=256, maxN=384, tiles128=6, mode=2, n=1, sA=0, sB=0, sC=0, sCT=0, CT=_PTR, A=_PTR,
             jobs=True, **kw):
        ln = dict(lens, **{k: v for k, v in kw.items() if k in lens})
        arr = (Job * 1)(Job(**dict(ok, **(job or {}))))
        return lib.sr_test_gemm_tn_jobs(0, A, ln["lenA"], _PTR, ln["lenB"], _PTR, ln["lenC"], CT, ln["lenCT"], ld,
                                        ctypes.cast(arr, ctypes.c_void_p) if jobs else None, njobs, maxM, maxN, tiles128, 1.0, mode,
                                        n, sA, sB, sC, sCT, None)
    _refused(call(A=None), "NULL")
    _refused(call(jobs=False), "NULL")
    _refused(call(ld=393), "ld=393")
    _refused(call(mode=0), "mode=0")
    _refused(call(mode=4), "mode=4")
    _refused(call(njobs=0), "njobs=0")
    _refused(call(maxM=200), "maxM=200")
    _refused(call(job=dict(M=100)), "M=100")
    _refused(call(job=dict(K=24)), "K=24")
    _refused(call(job=dict(M=384)), "M=384")                 # beyond maxM
    _refused(call(job=dict(a=1)), "even")
    _refused(call(job=dict(a=-2)), "past")
    # a job whose extent passes its buffer: each operand and each result in turn, by one double
    for key in lens:
        _refused(call(**{key: lens[key] - 1}), "past")
    _refused(call(job=dict(c=2)), "past")
    _refused(call(job=dict(N=384), ld=256, maxN=384), "past")            # a row of C is wider than ld
    # ... for every batch member: the second one of two starts a stride further
    _refused(call(n=2, sA=64), "past")
    _refused(call(n=2, sCT=2), "past")
    _refused(call(n=2, sB=31), "batch")
