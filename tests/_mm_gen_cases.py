"""The inputs of the general-family moment-matching tests -- TEST infrastructure, shared by the GPU test (which runs them on
the device) and the host test (which measures the fp64 rounding floor of the reference on exactly these inputs).

A case is (Z, Y, kp, noise, m, S): data, the packed parameters [kappa id = 0, v, c0, s[D], a[D], b[D]] per output, the noise
variances and T Gaussian inputs.  ``corner`` names the parameter corner:
  dense    every entry of s, a, b and c0 non-zero, the outputs' parameters differ
  s1       s zero except on input dimension 1 (the RBF factor sees one dimension)
  a0       a = 0, c0 = 1: v exp(.) + sum b x z; with b0 as well (``rbf``) it is the plain ARD-RBF kernel
  b0       b = 0
  c00      c0 = 0
  lin_rbf  the in-tree kernel: c0 = 0, s and a on input dimension 1 only, b dense"""
import zlib

import numpy as np

CORNERS = ("dense", "s1", "a0", "b0", "c00", "lin_rbf")
WIDTHS = (1, 2, 3, 4, 5, 8, 9, 12)               # DT = 4: D = 1 .. 4; DT = 8: 5, 8; DT = 12: 9, 12
MMX_IT, MMX_JT = 64, 256                         # tiles of the double-sum kernel (csrc/sr_moment_match_gen.hip)
SIZES = (1, 2, MMX_IT - 1, MMX_IT, MMX_IT + 1, MMX_JT - 1, MMX_JT, MMX_JT + 1, 300)
S_KINDS = ("zero", "rank1", "full")


def seed(*key):
    return zlib.crc32("/".join(str(k) for k in key).encode())


def packed(rng, D, n_out, corner="dense"):
    kp = np.zeros((n_out, 3 + 3 * D))
    for o in range(n_out):
        v, c0 = rng.uniform(0.5, 1.5), rng.uniform(0.4, 1.0)
        s = 1.0 / (rng.uniform(0.6, 1.4, D) * np.sqrt(D / 3.0))
        a, b = rng.uniform(0.2, 0.8, D) / D, rng.uniform(0.1, 0.5, D) / D
        if corner in ("s1", "lin_rbf") and D > 1:
            keep = s[1]
            s[:] = 0.0
            s[1] = keep
        if corner in ("a0", "rbf"):
            a[:], c0 = 0.0, 1.0
        if corner in ("b0", "rbf"):
            b[:] = 0.0
        if corner in ("c00", "lin_rbf"):
            c0 = 0.0
        if corner == "lin_rbf" and D > 1:
            keep = a[1] * D
            a[:] = 0.0
            a[1] = keep
        kp[o, 1], kp[o, 2] = v, c0
        kp[o, 3:3 + D], kp[o, 3 + D:3 + 2 * D], kp[o, 3 + 2 * D:] = s, a, b
    return kp


def problem(key, N, D, n_out, corner="dense", noise=1e-2, shift=0.0):
    """Z (N, D) in [-1, 1]^D + shift, Y (N, n_out) a smooth function with a linear part, kp, noise (n_out,)"""
    rng = np.random.default_rng(seed(*key))
    Z = rng.uniform(-1, 1, (N, D)) + shift
    Y = (np.sin(2.0 * Z.dot(rng.standard_normal((D, n_out)) / np.sqrt(D))) + 0.3 * Z.dot(rng.standard_normal((D, n_out)))
         + 0.05 * rng.standard_normal((N, n_out)))
    return Z, Y, packed(rng, D, n_out, corner), np.full(n_out, noise)


def inputs(key, Z, T, kind):
    """T means near the data and their covariances: all zero (None), rank 1 (singular), or full rank (standard deviations
    ~0.2); kind "same": the full-rank input of row 0 in every row"""
    rng = np.random.default_rng(seed(*key))
    D = Z.shape[1]
    m = Z[rng.integers(0, Z.shape[0], T)] + 0.2 * rng.standard_normal((T, D))
    if kind == "zero":
        return m, None
    g = 0.25 * rng.standard_normal((T, D, 1 if kind == "rank1" else D)) / np.sqrt(D)
    S = np.matmul(g, np.transpose(g, (0, 2, 1)))
    if kind == "same":
        m, S = np.repeat(m[:1], T, axis=0), np.repeat(S[:1], T, axis=0)
    return m, S


def width_case(D, kind):
    Z, Y, kp, noise = problem(("width", D), 130, D, 2)
    return (Z, Y, kp, noise) + inputs(("width-q", D, kind), Z, 5, kind)


def size_case(N, kind):
    Z, Y, kp, noise = problem(("size", N), N, 3, 2)
    return (Z, Y, kp, noise) + inputs(("size-q", N, kind), Z, 3, kind)


def outputs_case(n_out):
    Z, Y, kp, noise = problem(("outputs",), 40, 3, 3)
    return (Z, Y[:, :n_out], kp[:n_out], noise[:n_out]) + inputs(("outputs-q",), Z, 3, "full")


def kinds_case(kind):
    Z, Y, kp, noise = problem(("kinds",), 90, 3, 2, corner="lin_rbf")
    return (Z, Y, kp, noise) + inputs(("kinds-q", kind), Z, 4, kind)


SHIFT, SHIFT_NOISE = 5.0, 1e-2


def corner_case(corner, shift=0.0):
    Z, Y, kp, noise = problem(("corner", corner), 70, 3, 2, corner=corner, noise=SHIFT_NOISE if shift else 1e-2, shift=shift)
    return (Z, Y, kp, noise) + inputs(("corner-q", corner), Z, 3, "full")


def all_cases():
    """(tag, case) of every comparison against the closed form in the GPU test"""
    for D in WIDTHS:
        for kind in S_KINDS:
            yield "width D=%d %s" % (D, kind), width_case(D, kind)
    for N in SIZES:
        for kind in ("full", "zero"):
            yield "size N=%d %s" % (N, kind), size_case(N, kind)
    for n_out in (1, 3):
        yield "outputs n_out=%d" % n_out, outputs_case(n_out)
    for kind in S_KINDS + ("same",):
        yield "kinds %s" % kind, kinds_case(kind)
    for corner in ("s1", "a0", "rbf", "b0", "c00", "lin_rbf"):
        yield "corner %s" % corner, corner_case(corner)
    yield "shift +%g" % SHIFT, corner_case("dense", SHIFT)
