"""The fp64 MFMA TN GEMM family of csrc/sr_gemm.hip, one product at a time, against the exact reference of tests/_gemm_ref.py:
the plain kernel on both workgroup tiles at every k-tile count that picks another branch of the main loops
(csrc/sr_mfma_tile.h), all five modes, the upper-triangle kernel in both tile orders, the split-K form and the job table with
its transposed second output.

Integer data (see _gemm_ref): the device result must EQUAL the reference, for every order of accumulation -- no tolerance.
Operands and results are windows of wider allocations, with leading dimensions that differ from the widths and from each
other; operand padding holds NaN; everything a call must not write is compared bit for bit with what it held before; "P"
operands hold NaN wherever a mode says the kernel does not read.  Every product runs twice and must give the same bits.
One real-valued case per kernel is held to the a-priori error bound of the fp64 dot product (section E).

Which tile a shape takes is decided by the size rules of sr_gemm.hip, restated here (use_tile64*): a case that is meant for
one tile asserts the rule first, so a change of the thresholds fails loudly instead of testing the other tile."""
import ctypes

import numpy as np
import pytest

import _gemm_ref as gr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(lib_built):
    import torch
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"


# ---- the size rules of sr_gemm.hip, restated -------------------------------------------------------------------------------
def use_tile64(tiles128, K):                 # sr_use_tile64: plain kernel (and the upper kernel with prio)
    if K >= 768 and tiles128 >= 256:
        return False
    return tiles128 < 1024


def use_tile64_bulk(tiles128):               # sr_use_tile64_bulk: upper kernel without prio
    return tiles128 < 192


def use_tile64_jobs(tiles128):               # sr_use_tile64_jobs
    return tiles128 < 1024


JOBS_SUPERTILE_GRID = 16384                  # sr_launch_gemm_tn_jobs: super-tiles from this many 128 x 128 tiles of the grid on


def upper_tiles128(M, N, n=1):
    tm, tn = M // 128, N // 128
    return (tm * tn - tm * (tm - 1) // 2) * n


# ---- device plumbing -------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


def _up(buf):
    from safe_exploration_amd import _buffers as B
    return B.as_dev(buf, _dev())


def _at(t, off):
    return ctypes.c_void_p(t.data_ptr() + 8 * off)


def _twice(d0, launch):
    """Run launch(dC) on two fresh device copies of d0; both results must have the same bits.  Returns the first as NumPy."""
    import torch
    from safe_exploration_amd import _buffers as B
    outs = []
    for _ in range(2):
        d = d0.clone()
        launch(d)
        torch.cuda.synchronize()
        outs.append(d)
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64)), "two runs of one product differ"
    return B.to_numpy(outs[0])


def _stream():
    from safe_exploration_amd import _buffers as B
    return B.stream_ptr(_dev())


# ---- a product (or a batch of them) as windows of flat allocations -----------------------------------------------------------
class Case(object):
    """n products M x N x K in `mode`: flat host buffers bufA, bufB (NaN outside the operands), bufC (integers where beta != 0,
    NaN where beta == 0: beta == 0 must overwrite, not scale), the expected contents of the C allocation after the call, and
    the mask of what the call must leave alone."""

    def __init__(self, seed, M, N, K, alpha, beta, mode, variant="Z", n=1, wide=True, real=False, c_contig=False):
        rng = np.random.default_rng(seed)
        if not real:
            gr.assert_exact(K, alpha, beta)
        self.M, self.N, self.K, self.alpha, self.beta, self.mode, self.n, self.real = M, N, K, alpha, beta, mode, n, real
        self.lda, self.ldb, self.ldc = (M + 24, N + 40, N + 8) if wide else (M, N, N)
        if c_contig:
            self.ldc = N
        self.off = gr.OFFSET if wide else 0
        self.sA, self.sB, self.sC = K * self.lda + 48, K * self.ldb + 80, (M + 2) * self.ldc + 18     # (two rows behind M)
        tail = gr.TAIL
        self.bufA = np.full(self.off + n * self.sA + tail, np.nan)
        self.bufB = np.full(self.off + n * self.sB + tail, np.nan)
        nC = self.off + n * self.sC + tail
        if beta != 0:
            self.bufC = rng.standard_normal(nC) if real else gr.integers(rng, nC)
        else:
            self.bufC = np.full(nC, np.nan)
        self.expect = self.bufC.copy()
        self.untouched = np.ones(nC, dtype=bool)
        self.Az, self.Bz, self.C0 = [], [], []
        for z in range(n):
            A, Bm = gr.operands(rng, M, N, K, mode, variant, real)
            gr.window(self.bufA, K, M, self.lda, self.off + z * self.sA)[...] = A
            gr.window(self.bufB, K, N, self.ldb, self.off + z * self.sB)[...] = Bm
            Az, Bz = np.nan_to_num(A, nan=0.0), np.nan_to_num(Bm, nan=0.0)      # the reference of P is the reference of Z
            C0 = self.cwin(self.bufC, z).copy()
            self.Az.append(Az), self.Bz.append(Bz), self.C0.append(C0)
            if not real:
                self.cwin(self.expect, z)[...] = gr.gemm_tn(Az, Bz, C0, alpha, beta, mode)
            self.cwin(self.untouched, z)[...] = ~gr.written_blocks(M, N, mode)

    def cwin(self, buf, z=0):
        return gr.window(buf, self.M, self.N, self.ldc, self.off + z * self.sC)

    def check(self, got):
        """Exact equality everywhere (NaN prefill included), and the bits of everything the call must leave alone."""
        assert gr.same_bits(got[self.untouched], self.bufC[self.untouched]), "the call wrote outside its tiles"
        np.testing.assert_array_equal(got, self.expect)
        assert not np.isnan(got[~self.untouched]).any()


def run_plain(c, prio=0):
    from safe_exploration_amd._lib import lib, check
    dA, dB, s = _up(c.bufA), _up(c.bufB), _stream()

    def launch(dC):
        check(lib.sr_test_gemm_tn_ex(0, _at(dA, c.off), c.lda, _at(dB, c.off), c.ldb, _at(dC, c.off), c.ldc, c.M, c.N, c.K,
                                     c.alpha, c.beta, c.mode, prio, c.n, c.sA, c.sB, c.sC, s))
    return _twice(_up(c.bufC), launch)


def run_upper(c, order, prio=0):
    from safe_exploration_amd._lib import lib, check
    dA, dB, s = _up(c.bufA), _up(c.bufB), _stream()

    def launch(dC):
        check(lib.sr_test_gemm_tn_upper_ex(0, _at(dA, c.off), c.lda, _at(dB, c.off), c.ldb, _at(dC, c.off), c.ldc, c.M, c.N,
                                           c.K, c.alpha, c.beta, order, prio, c.n, c.sA, c.sB, c.sC, s))
    return _twice(_up(c.bufC), launch)


# ================================================================== A. plain kernel
@pytest.mark.parametrize("kt", [1, 2, 3, 4, 5, 6, 7, 8, 9])
def test_plain_tile64_every_ktile_count(kt):
    """srt64::mainloop_tn_pipe: the prologue issues npro = min(kt, 4) tiles and waits by npro; a step waits by the tiles behind
    it (>= 3, 2, 1, 0) and issues the tile four ahead from 4 behind on.  kt = 1 .. 9: every npro, every residue of kt mod 4 below
    and above the four stages, and the second trip of the four-step loop."""
    M, N, K = 128, 256, 16 * kt
    assert use_tile64(M // 128 * (N // 128), K)
    c = Case(100 + kt, M, N, K, -0.5, 2.0, 0)
    c.check(run_plain(c))


@pytest.mark.parametrize("variant", ["Z", "P"])
@pytest.mark.parametrize("M,N,K,mode", [(384, 384, 384, 1), (384, 384, 384, 2), (384, 384, 384, 3), (384, 384, 384, 4),
                                        (256, 512, 512, 1), (256, 512, 512, 2), (256, 512, 512, 3), (256, 512, 512, 4),
                                        (384, 128, 256, 3)])
def test_plain_tile64_modes(M, N, K, mode, variant):
    """Modes 1 - 4 on the 64-tile (k ranges at 128-block granularity: both 64-tiles of a block row / column take the block's
    range); (384, 128, 256, 3): the clamp min(K, m0 + 128) with m0 + 128 > K.  Mode 1 has dense operands in either variant."""
    assert use_tile64(M // 128 * (N // 128), K)
    alpha, beta = ((1.0, -1.0) if variant == "Z" else (2.0, 0.0)) if mode != 1 else ((-1.0, 1.0) if variant == "Z" else (1.0, 0.0))
    c = Case(200 + 10 * mode + M // 128, M, N, K, alpha, beta, mode, variant)
    c.check(run_plain(c))


@pytest.mark.parametrize("K", [768, 784])
def test_plain_tile128_long_k(K):
    """2048 x 2048: 256 tiles with K >= 768 take the 128-tile: 48 k-tiles (pairs only) and 49 (odd: one tile on stage 1 first)."""
    M = N = 2048
    assert not use_tile64(M // 128 * (N // 128), K)
    c = Case(300 + K, M, N, K, -0.5, 2.0, 0)
    c.check(run_plain(c))


@pytest.mark.parametrize("K", [16, 32, 48])
def test_plain_tile128_short_k(K):
    """4096 x 4096 = 1024 tiles: the 128-tile at nt = 1, 2, 3 k-tiles -- the three prologue shapes of the paired loop (one tile;
    one pair, both DMAs in the prologue; odd start whose successor's DMA goes out under the first tile).  Contiguous
    operands at offset zero (134 MB of C)."""
    M = N = 4096
    assert not use_tile64(M // 128 * (N // 128), K)
    c = Case(310 + K, M, N, K, 2.0, 0.0, 0, wide=False)
    c.check(run_plain(c))


@pytest.mark.parametrize("variant", ["Z", "P"])
@pytest.mark.parametrize("mode", [2, 3, 4])
def test_plain_tile128_modes(mode, variant):
    """Triangular k ranges on the 128-tile (K = 2048 >= 768, 256 tiles): 1 .. 16 blocks of eight k-tiles per tile."""
    M = N = K = 2048
    assert not use_tile64(M // 128 * (N // 128), K)
    c = Case(320 + mode, M, N, K, 1.0, -1.0, mode, variant)
    c.check(run_plain(c))


@pytest.mark.parametrize("M,N,K,n", [(256, 256, 80, 3), (2048, 2048, 768, 2)])
def test_plain_batch(M, N, K, n):
    """Batch members at strides that are not the matrix size (Case: K lda + 48, K ldb + 80, (M + 2) ldc + 18): the small one on
    the 64-tile with 5 k-tiles, the big one on the 128-tile (the rule counts the tiles of the whole batch)."""
    assert use_tile64(M // 128 * (N // 128) * n, K) == (M == 256)
    c = Case(400 + n, M, N, K, -0.5, 2.0, 0, n=n)
    c.check(run_plain(c))


@pytest.mark.parametrize("M,N,K", [(256, 384, 112), (2048, 2048, 784)])
def test_plain_prio_same_bits(M, N, K):
    """prio = 1 raises the wavefront priority and nothing else: same tile (same rule), same bits."""
    assert use_tile64(M // 128 * (N // 128), K) == (M == 256)
    c = Case(500 + M, M, N, K, -1.0, 1.0, 0)
    g0, g1 = run_plain(c, prio=0), run_plain(c, prio=1)
    c.check(g0)
    assert gr.same_bits(g0, g1)


# ================================================================== B. upper-triangle kernel
def check_upper(c, got, t64):
    """Blocks right of and on the diagonal: the reference; blocks below it: untouched (Case.check, mode 1).  With the 64-tile the
    lower-left 64 x 64 quarter of a diagonal block is unspecified -- the launcher says untouched, nothing reads it: it may
    hold its prefill or the reference, as a whole.  With the 128-tile it is part of the tile: the reference."""
    got = got.copy()
    if t64:
        for z in range(c.n):
            g, e, p = c.cwin(got, z), c.cwin(c.expect, z), c.cwin(c.bufC, z)
            u = c.cwin(c.untouched, z)
            for m0 in range(0, c.M, 128):
                q = (slice(m0 + 64, m0 + 128), slice(m0, m0 + 64))
                assert gr.same_bits(g[q], p[q]) or np.array_equal(g[q], e[q]), "diagonal block at %d: quarter is neither" % m0
                g[q] = e[q]
                assert not u[q].any()
    c.check(got)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("K", [48, 128])
def test_upper_tile64(K, order):
    """384 x 640 (12 tiles: 64-tile), rectangular M < N.  order 0: the linear index -> (m, n) of sr_upper_index on a 6 x 10 grid
    of 64-tiles; order 1: one 8 x 8 super-tile row (2 super-tiles), most workgroups guarded out.  alpha = -1, beta = 1 as the
    trailing update calls it, and alpha = 1, beta = 0 over NaN."""
    M, N = 384, 640
    assert use_tile64_bulk(upper_tiles128(M, N))
    for alpha, beta in ((-1.0, 1.0), (1.0, 0.0)):
        c = Case(600 + K + order, M, N, K, alpha, beta, 1)
        check_upper(c, run_upper(c, order), True)


def test_upper_tile64_batch_and_prio():
    """Two members on the 64-tile (24 tiles in all); prio = 1 takes the plain rule (64-tile here too) and gives the same bits."""
    M, N, K = 384, 640, 80
    assert use_tile64_bulk(upper_tiles128(M, N, 2)) and use_tile64(upper_tiles128(M, N, 2), K)
    c = Case(650, M, N, K, -1.0, 1.0, 1, n=2)
    g0 = run_upper(c, 1)
    check_upper(c, g0, True)
    check_upper(c, run_upper(c, 0), True)
    assert gr.same_bits(run_upper(c, 1, prio=1), g0)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("K", [16, 48, 128])
@pytest.mark.parametrize("M,N", [(2560, 2560), (1920, 2560)])
def test_upper_tile128(M, N, K, order):
    """210 and 195 tiles (>= 192: the 128-tile) at 1, 3 and 8 k-tiles -- the paired loop's small odd and even counts at its
    second call site -- in both orders; (1920, 2560): 15 x 20 tiles, two super-tile rows of which the second is cut at M."""
    assert not use_tile64_bulk(upper_tiles128(M, N))
    for alpha, beta in ((-1.0, 1.0), (1.0, 0.0)):
        c = Case(700 + K + order + M // 128, M, N, K, alpha, beta, 1)
        check_upper(c, run_upper(c, order), False)


# ================================================================== C. split-K
def run_splitk(c, ks, part_tail=gr.TAIL):
    """C (contiguous M x N) through part (NaN on entry, exactly ceil(K / ks) M N doubles + a guard).  Returns C's allocation."""
    import torch
    from safe_exploration_amd._lib import lib, check
    from safe_exploration_amd import _buffers as B
    assert c.ldc == c.N and c.n == 1
    nsl = -(-c.K // ks)
    plen = nsl * c.M * c.N
    dA, dB, s = _up(c.bufA), _up(c.bufB), _stream()
    parts = []

    def launch(dC):
        part = torch.full((plen + part_tail,), float("nan"), dtype=torch.float64, device=_dev())
        check(lib.sr_test_gemm_tn_splitk(0, _at(dA, c.off), c.lda, _at(dB, c.off), c.ldb, _at(dC, c.off), c.M, c.N, c.K, ks,
                                         c.alpha, c.mode, _at(part, 0), plen, s))
        parts.append(part)
    got = _twice(_up(c.bufC), launch)
    for part in parts:
        p = B.to_numpy(part)
        assert np.isnan(p[plen:]).all(), "split-K wrote behind its slices"
        assert not np.isnan(p[:plen]).any(), "a slice (an empty one?) was not written"
    return got


@pytest.mark.parametrize("ks", [128, 256, 384, 640, 1024])
@pytest.mark.parametrize("M,N,K,mode,variant", [(640, 128, 640, 0, "Z"), (640, 128, 640, 3, "Z"), (640, 128, 640, 3, "P"),
                                                (640, 128, 640, 4, "Z"), (640, 128, 640, 4, "P"), (128, 128, 640, 0, "Z")])
def test_splitk(M, N, K, mode, variant, ks):
    """The shapes of the row append.  ks = 128 .. 1024: five full slices; a short last slice (640 = 2 x 256 + 128, 384 + 256); one
    slice; ks > K; and with modes 3 / 4 slices that the mode's k range cuts or leaves empty (they must write zeros: part
    holds NaN).  Equality with the one reference for every ks: the result does not depend on the slicing."""
    c = Case(800 + mode + M // 128, M, N, K, -0.5 if mode else 2.0, 0.0, mode, variant, c_contig=True)
    c.check(run_splitk(c, ks))


# ================================================================== D. job table
class Job(ctypes.Structure):
    _fields_ = [("a", ctypes.c_long), ("b", ctypes.c_long), ("c", ctypes.c_long), ("ct", ctypes.c_long),
                ("M", ctypes.c_int), ("N", ctypes.c_int), ("K", ctypes.c_int), ("pad", ctypes.c_int)]


JOB_SHAPES = [(128, 128, 128), (256, 128, 256), (128, 384, 384), (384, 384, 384), (256, 256, 512)]       # (M, N, K)
JOB_LD = 520                                 # wider than any job
# column offsets of the jobs' rectangles in their canvases: operands even (16-byte pieces), results odd too
JOB_COL = dict(a=[0, 8, 136, 24, 2], b=[4, 130, 16, 120, 200], c=[3, 131, 17, 121, 201], ct=[5, 9, 137, 25, 1])


class JobCase(object):
    """The list as rectangles stacked (three rows apart) in four canvases of width JOB_LD, n batch members a stride apart.
    alias: the CT rectangles live in A's allocation, below the operands, as the inversion keeps W^T in the buffer it reads."""

    def __init__(self, seed, mode, variant, n=1, real=False, alias=False, alpha=-1.0):
        rng = np.random.default_rng(seed)
        self.mode, self.n, self.alpha, self.alias, ld = mode, n, alpha, alias, JOB_LD
        dims = dict(a=[(K, M) for M, N, K in JOB_SHAPES], b=[(K, N) for M, N, K in JOB_SHAPES],
                    c=[(M, N) for M, N, K in JOB_SHAPES], ct=[(N, M) for M, N, K in JOB_SHAPES])
        self.offs, rows = {}, {}
        for key in ("a", "b", "c", "ct"):
            r, self.offs[key] = 1, []
            for (h, w), col in zip(dims[key], JOB_COL[key]):
                assert col + w <= ld
                self.offs[key].append(r * ld + col)
                r += h + 3
            rows[key] = r
        if alias:                            # CT below the operands of A
            self.offs["ct"] = [o + rows["a"] * ld for o in self.offs["ct"]]
            rows["a"] += rows["ct"]
        self.stride = {k: rows[k] * ld + 64 for k in rows}
        self.len = {k: (n - 1) * self.stride[k] + rows[k] * ld for k in rows}       # what the entry is told
        self.buf = {k: np.full(gr.OFFSET + self.len[k] + gr.TAIL, np.nan) for k in rows}
        self.expect = {k: self.buf[k].copy() for k in ("c", "ct")}
        self.data = []
        for z in range(n):
            for j, (M, N, K) in enumerate(JOB_SHAPES):
                if not real:
                    gr.assert_exact(K, alpha, 0.0)
                A, Bm = gr.operands(rng, M, N, K, mode, variant, real)
                self.win("a", z, j, self.buf["a"])[...] = A
                self.win("b", z, j, self.buf["b"])[...] = Bm
                Az, Bz = np.nan_to_num(A, nan=0.0), np.nan_to_num(Bm, nan=0.0)
                self.data.append((z, j, Az, Bz))
                if not real:
                    ref = gr.gemm_tn(Az, Bz, None, alpha, 0.0, mode)
                    self.win("c", z, j, self.expect["c"])[...] = ref
                    if not alias:
                        self.win("ct", z, j, self.expect["ct"])[...] = ref.T
        if alias:                            # expected contents of A's allocation: the operands as they were + the CT rectangles
            self.expect["a"] = self.buf["a"].copy()
            for z, j, Az, Bz in self.data:
                self.win("ct", z, j, self.expect["a"])[...] = gr.gemm_tn(Az, Bz, None, alpha, 0.0, mode).T
        self.jobs = (Job * len(JOB_SHAPES))(*[Job(self.offs["a"][j], self.offs["b"][j], self.offs["c"][j], self.offs["ct"][j],
                                                  M, N, K, 0) for j, (M, N, K) in enumerate(JOB_SHAPES)])

    def win(self, key, z, j, buf):
        M, N, K = JOB_SHAPES[j]
        h, w = dict(a=(K, M), b=(K, N), c=(M, N), ct=(N, M))[key]
        skey = "a" if (key == "ct" and self.alias) else key
        return gr.window(buf, h, w, JOB_LD, gr.OFFSET + z * self.stride[skey] + self.offs[key][j])

    def run(self, with_ct, tiles128, maxM=384, maxN=384):
        """Returns the allocations of C and CT (alias: of A; None without CT) after the call."""
        from safe_exploration_amd._lib import lib, check
        from safe_exploration_amd import _buffers as B
        import torch
        dB, s, o = _up(self.buf["b"]), _stream(), gr.OFFSET
        dA0, dCT0 = _up(self.buf["a"]), _up(self.buf["ct"])
        outs = []
        for _ in range(2):
            dA, dC, dCT = dA0.clone(), _up(self.buf["c"]), dCT0.clone()
            ct, lct, sct = (dA, self.len["a"], self.stride["a"]) if self.alias else (dCT, self.len["ct"], self.stride["ct"])
            check(lib.sr_test_gemm_tn_jobs(0, _at(dA, o), self.len["a"], _at(dB, o), self.len["b"], _at(dC, o), self.len["c"],
                                           _at(ct, o) if with_ct else None, lct if with_ct else 0, JOB_LD,
                                           ctypes.cast(self.jobs, ctypes.c_void_p), len(JOB_SHAPES), maxM, maxN, tiles128, self.alpha,
                                           self.mode, self.n, self.stride["a"], self.stride["b"], self.stride["c"], sct, s))
            torch.cuda.synchronize()
            outs.append((B.to_numpy(dC), B.to_numpy(ct)))
        assert gr.same_bits(outs[0][0], outs[1][0]) and gr.same_bits(outs[0][1], outs[1][1]), "two runs of one list differ"
        return outs[0]

    def check(self, gotC, gotCT, with_ct):
        """C, CT and everything between the rectangles: the reference or the NaN prefill, exactly."""
        np.testing.assert_array_equal(gotC, self.expect["c"])
        key = "a" if self.alias else "ct"
        np.testing.assert_array_equal(gotCT, self.expect[key] if with_ct else self.buf[key])
        for z, j, Az, Bz in self.data:
            assert not np.isnan(self.win("c", z, j, gotC)).any()
            if with_ct:
                assert not np.isnan(self.win("ct", z, j, gotCT)).any()


@pytest.mark.parametrize("variant", ["Z", "P"])
@pytest.mark.parametrize("tiles128", [1, 4096])
@pytest.mark.parametrize("with_ct", [False, True])
@pytest.mark.parametrize("mode", [2, 3])
def test_jobs(mode, with_ct, tiles128, variant):
    """Five jobs of different shapes at scattered offsets, two batch members, on the 64-tile (tiles128 = 1: k ranges at 64
    granularity, CT in one pass) and on the 128-tile (4096: CT in two passes of 64 rows); the plain grid (3 x 3 tiles of 128)."""
    assert use_tile64_jobs(tiles128 * 2) == (tiles128 == 1)
    assert (384 // 128) ** 2 < JOBS_SUPERTILE_GRID
    jc = JobCase(900 + mode, mode, variant, n=2)
    gotC, gotCT = jc.run(with_ct, tiles128)
    jc.check(gotC, gotCT, with_ct)


@pytest.mark.parametrize("mode", [2, 3])
def test_jobs_supertile_grid(mode):
    """maxM = maxN = 16384 with the 128-tile: a grid of 128 x 128 tiles -- the threshold of the super-tile mapping itself -- over
    the same five small jobs: nearly every workgroup is guarded out, the rest reach their tiles through stf / sts."""
    assert not use_tile64_jobs(4096) and (16384 // 128) ** 2 >= JOBS_SUPERTILE_GRID
    jc = JobCase(920 + mode, mode, "P", n=1)
    gotC, gotCT = jc.run(True, 4096, maxM=16384, maxN=16384)
    jc.check(gotC, gotCT, True)


@pytest.mark.parametrize("tiles128", [1, 4096])
def test_jobs_ct_in_the_operand_buffer(tiles128):
    """Mode 3 with CT's base pointer == A's, as the inversion calls it: the CT rectangles lie in A's allocation outside every
    job's operand.  Afterwards A's allocation holds the operands unchanged (bit for bit, the NaN of the skipped blocks and of
    the padding included) and the transposed results."""
    jc = JobCase(940, 3, "P", n=2, alias=True)
    gotC, gotA = jc.run(True, tiles128)
    jc.check(gotC, gotA, True)
    keep = np.ones(gotA.size, dtype=bool)
    for z, j, Az, Bz in jc.data:
        jc.win("ct", z, j, keep)[...] = False
    assert gr.same_bits(gotA[keep], jc.buf["a"][keep]), "the call changed what it reads"


# ================================================================== E. real-valued data against the a-priori bound
def _ratio(name, got, exact, bound):
    err = np.abs(got.astype(np.longdouble) - exact).astype(np.float64)
    assert (bound > 0).all()
    r = float((err / bound).max())
    print("gemm family, real data: %-28s max |err| / bound = %.4f   (max |err| = %.3e)" % (name, r, err.max()))
    assert r <= 1.0, "%s: error %.3e x the a-priori bound" % (name, r)
    return r


def test_real_data_within_the_dot_product_bound():
    """Standard-normal data, one mid-size shape per kernel, against an np.longdouble product.  The bound is a priori:
    |err| <= (K + 2) 2^-53 (|alpha| |A|^T |B| + |beta| |C0|) element-wise -- K fused multiply-adds and the two operations of the
    epilogue, each within 2^-53 relative, in any order (split-K: its slices' sums pass through fewer roundings than that).
    Measured on an MI355X (profiles/r14_gemm_family.txt): see there; the assertion is ratio <= 1."""
    L = np.longdouble
    # plain, 64-tile, 25 k-tiles
    c = Case(1000, 256, 384, 400, -0.5, 2.0, 0, real=True)
    got = c.cwin(run_plain(c))
    _ratio("plain 256x384x400", got, gr.gemm_tn(c.Az[0], c.Bz[0], c.C0[0], -0.5, 2.0, 0, dtype=L),
           gr.error_bound(c.Az[0], c.Bz[0], c.C0[0], -0.5, 2.0))
    # plain, 128-tile, 49 k-tiles
    c = Case(1001, 2048, 2048, 784, -0.5, 2.0, 0, real=True)
    assert not use_tile64(256, 784)
    got = c.cwin(run_plain(c))[:256, 1792:]
    Az, Bz, C0 = c.Az[0][:, :256], c.Bz[0][:, 1792:], c.C0[0][:256, 1792:]
    _ratio("plain 2048x2048x784 (corner)", got, gr.gemm_tn(Az, Bz, C0, -0.5, 2.0, 0, dtype=L), gr.error_bound(Az, Bz, C0, -0.5, 2.0))
    # upper, 64-tile
    c = Case(1002, 384, 640, 128, -1.0, 1.0, 1, real=True)
    got = c.cwin(run_upper(c, 1))
    w = gr.written_blocks(384, 640, 1)
    exact = gr.gemm_tn(c.Az[0], c.Bz[0], c.C0[0], -1.0, 1.0, 1, dtype=L)
    bound = gr.error_bound(c.Az[0], c.Bz[0], c.C0[0], -1.0, 1.0)
    for m0 in range(0, 384, 128):            # (the unspecified quarters of the diagonal blocks)
        w[m0 + 64:m0 + 128, m0:m0 + 64] = False
    _ratio("upper 384x640x128", got[w], exact[w], bound[w])
    # split-K, mode 3
    c = Case(1003, 640, 128, 640, -0.5, 0.0, 3, real=True, c_contig=True)
    got = c.cwin(run_splitk(c, 256))
    _ratio("split-K 640x128x640 ks=256", got, gr.gemm_tn(c.Az[0], c.Bz[0], None, -0.5, 0.0, 3, dtype=L),
           gr.error_bound(c.Az[0], c.Bz[0], None, -0.5, 0.0))
    # job table, mode 2, with CT, 64-tile
    jc = JobCase(1004, 2, "Z", n=1, real=True, alpha=-1.0)
    gotC, gotCT = jc.run(True, 1)
    worst = 0.0
    for z, j, Az, Bz in jc.data:
        exact, bound = gr.gemm_tn(Az, Bz, None, -1.0, 0.0, 2, dtype=L), gr.error_bound(Az, Bz, None, -1.0, 0.0)
        g = jc.win("c", z, j, gotC)
        assert gr.same_bits(jc.win("ct", z, j, gotCT), g.T)
        worst = max(worst, _ratio("jobs %dx%dx%d" % JOB_SHAPES[j], g, exact, bound))
    assert worst <= 1.0
