"""NumPy reference of the TN GEMM family of csrc/sr_gemm.hip (plain, upper-triangle, split-K and job-table kernels) and
the data its tests run on.  No GPU, no torch.

    C[m][n] (op)= alpha * sum_k A[k][m] B[k][n] + beta * C[m][n],   A: K x M, B: K x N (k-major), C: M x N

Modes, as csrc/sr_common.h words them, at the granularity of 128-blocks (m0, n0 = first row / column of the 128-block):
    0  all tiles
    1  only the blocks with n0 >= m0 are written (upper block triangle); the others keep what they held
    2  B block-lower-triangular (B[k][n] == 0 for k < n0): k starts at n0
    3  A block-upper-triangular (A[k][m] == 0 for k >= m0 + 128): k ends at min(K, m0 + 128)
    4  A block-lower-triangular (A[k][m] == 0 for k < m0): k starts at m0
The reference walks exactly these k ranges, so it never looks at what a mode skips either.

EXACT DATA: operands and C0 are integers of [-1000, 1000] stored as fp64, alpha and beta come from ALPHAS.  Every partial sum
of alpha A^T B + beta C0 is then a multiple of 1/2 below 2^53 in magnitude, whatever the order of summation: fp64
arithmetic (fused or not) makes no rounding error, `A.T @ B` is the exact answer and a device result must EQUAL it.

TRIANGULAR OPERANDS are element-wise triangular inside their diagonal 128-blocks (a 64 x 64 workgroup tile skips half a
diagonal block that a 128 x 128 tile reads: with zeros there both agree), non-zero everywhere on the kept side, and in the
128-blocks wholly on the skipped side zero (variant "Z") or NaN (variant "P": the result is the same only if nothing reads
what the mode says is skipped).
"""
import numpy as np

BLOCK = 128
VMAX = 1000
ALPHAS = (1.0, -1.0, -0.5, 2.0, 0.0)


def assert_exact(K, alphas, betas):
    """The condition under which every partial sum is exact in fp64."""
    alphas, betas = np.atleast_1d(alphas), np.atleast_1d(betas)
    assert all(float(a) in ALPHAS for a in alphas) and all(float(b) in ALPHAS for b in betas), "alpha, beta outside ALPHAS"
    assert K * VMAX ** 2 * np.abs(alphas).max() + VMAX * np.abs(betas).max() < 2 ** 53, "partial sums may round"


def integers(rng, shape, nonzero=False):
    v = rng.integers(-VMAX, VMAX + 1, size=shape)
    if nonzero:
        v[v == 0] = VMAX
    return v.astype(np.float64)


def shape_operand(X, kind, variant):
    """X (K x W, k-major) -> a copy with the structure a mode promises.  kind "lower": X[k][w] == 0 for k < w0 (modes 2 and
    4), "upper": X[k][w] == 0 for k >= w0 + 128 (mode 3); element-wise inside the diagonal 128-blocks; the 128-blocks wholly
    on the skipped side hold 0 (variant "Z") or NaN ("P")."""
    assert kind in ("lower", "upper") and variant in ("Z", "P")
    K, W = X.shape
    k, w = np.arange(K)[:, None], np.arange(W)[None, :]
    kb, wb = k // BLOCK, w // BLOCK
    skipped_block = (kb < wb) if kind == "lower" else (kb > wb)
    skipped_elem = (kb == wb) & ((k < w) if kind == "lower" else (k > w))
    out = X.copy()
    out[skipped_elem] = 0.0
    out[skipped_block] = 0.0 if variant == "Z" else np.nan
    return out


def operands(rng, M, N, K, mode, variant="Z", real=False):
    """(A, B) for a product in `mode`: integers (real: standard normal), shaped for the mode."""
    if real:
        A, B = rng.standard_normal((K, M)), rng.standard_normal((K, N))
    else:
        A, B = integers(rng, (K, M), nonzero=True), integers(rng, (K, N), nonzero=True)
    if mode == 2:
        B = shape_operand(B, "lower", variant)
    elif mode == 3:
        A = shape_operand(A, "upper", variant)
    elif mode == 4:
        A = shape_operand(A, "lower", variant)
    else:
        assert mode in (0, 1)
    return A, B


def k_range(mode, m0, n0, K):
    """k range of the 128-block at (m0, n0)."""
    k_beg = n0 if mode == 2 else (m0 if mode == 4 else 0)
    k_end = min(K, m0 + BLOCK) if mode == 3 else K
    return k_beg, max(k_end, k_beg)


def gemm_tn(A, B, C0, alpha, beta, mode, dtype=np.float64):
    """The product in `mode`; C0 may be None with beta == 0.  dtype: the arithmetic (np.longdouble for real-valued data)."""
    K, M = A.shape
    N = B.shape[1]
    assert B.shape[0] == K and M % BLOCK == 0 and N % BLOCK == 0 and mode in (0, 1, 2, 3, 4)
    assert beta == 0 or C0 is not None
    out = np.full((M, N), np.nan, dtype=dtype) if C0 is None else np.array(C0, dtype=dtype)
    alpha, beta = dtype(alpha), dtype(beta)
    for m0 in range(0, M, BLOCK):
        for n0 in range(0, N, BLOCK):
            if mode == 1 and n0 < m0:
                continue
            kb, ke = k_range(mode, m0, n0, K)
            prod = A[kb:ke, m0:m0 + BLOCK].astype(dtype).T @ B[kb:ke, n0:n0 + BLOCK].astype(dtype)
            blk = alpha * prod
            if beta != 0:                       # beta == 0 overwrites (C0 may hold NaN)
                blk = blk + beta * out[m0:m0 + BLOCK, n0:n0 + BLOCK]
            out[m0:m0 + BLOCK, n0:n0 + BLOCK] = blk
    return out


def written_blocks(M, N, mode):
    """Boolean M x N: the elements a product in `mode` writes (mode 1 leaves the blocks n0 < m0 alone)."""
    m, n = np.arange(M)[:, None] // BLOCK, np.arange(N)[None, :] // BLOCK
    return (n >= m) if mode == 1 else np.ones((M, N), dtype=bool)


def error_bound(A, B, C0, alpha, beta):
    """|device - exact| <= (K + 2) 2^-53 (|alpha| |A|^T |B| + |beta| |C0|) element-wise: K fused multiply-adds and the two
    operations of the epilogue, each with a relative error of 2^-53 at most, in any order of summation.  Operands in their
    "Z" form (a skipped term is a zero term)."""
    K = A.shape[0]
    b = abs(alpha) * (np.abs(A).T @ np.abs(B))
    if C0 is not None and beta != 0:
        b = b + abs(beta) * np.abs(C0)
    return (K + 2) * 2.0 ** -53 * b


# ---- operands and results as windows of wider allocations -------------------------------------------------------------------
OFFSET = 128     # doubles in front of a window ("128 columns into a wider allocation")
TAIL = 256       # doubles behind it


def flat_len(rows, ld, offset=OFFSET, tail=TAIL):
    return offset + rows * ld + tail


def window(buf, rows, cols, ld, offset=OFFSET):
    """Writable rows x cols view with row stride ld that starts `offset` elements into the flat array buf (any dtype)."""
    assert buf.ndim == 1 and offset + (rows - 1) * ld + cols <= buf.size and cols <= ld
    return np.lib.stride_tricks.as_strided(buf[offset:], shape=(rows, cols), strides=(buf.itemsize * ld, buf.itemsize))


def embed(X, ld, fill=np.nan, extra_rows=0, offset=OFFSET, tail=TAIL):
    """Flat allocation filled with `fill` (a scalar, or an array of the allocation's length) that holds X as a window."""
    rows, cols = X.shape
    n = flat_len(rows + extra_rows, ld, offset, tail)
    buf = np.full(n, fill, dtype=np.float64) if np.isscalar(fill) else np.array(fill, dtype=np.float64).reshape(n)
    window(buf, rows, cols, ld, offset)[...] = X
    return buf


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.int64), b.view(np.int64)))
