"""The width lists of tests/test_gpu_widths.py follow the sources: the route thresholds and the padded-width ladder are
read from the HIP sources (the ladder from its one definition in sr_dispatch.h), and every edge and edge + 1 must be in the lists of the group that tests that route.  If a
threshold moves and the matrix does not, this fails on the CPU.  Runs without a GPU."""
import os
import re

import test_gpu_widths as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "safe_exploration_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(src, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\b" % name, src, re.M)
    assert m, "#define %s not found" % name
    return int(m.group(1))


LADDER = (r"D\s*<=\s*(\d+)\s*\?\s*\1\s*:\s*\(?\s*[\w>.-]*D\s*<=\s*(\d+)\s*\?\s*\2\s*:\s*\(?\s*"
          r"[\w>.-]*D\s*<=\s*(\d+)\s*\?\s*\3\s*:\s*(\d+)")


def _ladders(names):
    """every padded-width ladder `D <= a ? a : (D <= b ? b : (... : z))` of these sources, as (a, b, ..., z)"""
    return [tuple(int(g) for g in m.groups()) for name in names for m in re.finditer(LADDER, _read(name))]


def test_thresholds_mirrored():
    common = _read("sr_common.h")
    assert W.SR_STREAM_FUSED_MAX_D == _define(common, "SR_STREAM_FUSED_MAX_D")
    assert W.SR_LIN_FUSED_MAX_D == _define(common, "SR_LIN_FUSED_MAX_D")
    assert W.SR_GRAD_MAX_D == _define(_read("sr_predict_grad.hip"), "SR_GRAD_MAX_D")
    assert max(W.DT_LADDER) == _define(common, "SR_MAX_D")
    # the padded width is defined once (sr_width_bucket in sr_dispatch.h); the second-order route takes it from there in three
    # places (accumulator count, final kernel, streamed linearize) and picks its kernels from the same list
    assert _ladders(["sr_dispatch.h"]) == [W.DT_LADDER]
    assert "sr_width_bucket" in re.search(r"[^\n]*D <= 3 \?[^\n]*", _read("sr_dispatch.h")).group(0)
    users = ("sr_capi_posterior.hip", "sr_linearize.hip")
    assert _ladders(users) == [], "hand-written padded-width ladder beside sr_width_bucket"
    assert sum(len(re.findall(r"\bsr_width_bucket\(", _read(n))) for n in users) >= 3, "padded width not taken from sr_width_bucket"
    picks = [tuple(int(w) for w in m.group(1).split(",")) for m in re.finditer(r"sr_pick_le<([\d, ]+)>", _read("sr_linearize.hip"))]
    assert len(picks) >= 2 and set(picks) == {W.DT_LADDER}, picks
    # K0 (the one-launch pass) and its second-order form
    m = re.search(r"sr_gp_small_wanted\(.*?\{(.*?)\n\}", common, re.S)
    assert m and re.search(r"D\s*<=\s*%d\s*;" % W.K0_MAX_D, m.group(1)), "K0 width limit moved"
    m = re.search(r"sr_gp_small_lin_wanted\(.*?\{(.*?)\n\}", common, re.S)
    assert m and re.search(r"!general\s*\|\|\s*D\s*<=\s*%d" % W.K0_GENERAL_LIN_MAX_D, m.group(1)), \
        "general K0 LIN width limit moved"


def _has_edges(widths, edges, what):
    for e in edges:
        for d in (e, e + 1):
            if d <= max(W.DT_LADDER):
                assert d in widths, "%s: width %d (edge %d) not tested" % (what, d, e)


def test_width_lists_hold_every_edge():
    ladder_edges = W.DT_LADDER[:-1]
    # single query, second order: every DT edge, the one-launch streamed linearize, K0 (RBF and general)
    _has_edges(W.LIN_WIDTHS, ladder_edges + (W.SR_LIN_FUSED_MAX_D, W.K0_MAX_D, W.K0_GENERAL_LIN_MAX_D), "linearize")
    assert max(W.DT_LADDER) in W.LIN_WIDTHS
    # batched posterior: every DT edge; the one-launch streamed predict's K* edge (route asserted)
    _has_edges(W.BATCH_WIDTHS, ladder_edges + (W.SR_STREAM_FUSED_MAX_D,), "batched posterior")
    _has_edges(W.STREAM_EDGE_WIDTHS, (W.SR_STREAM_FUSED_MAX_D,), "one streamed query")
    _has_edges(W.KSTAR2_WIDTHS, (W.DT_LADDER[1],), "two queries per thread")
    assert max(W.DT_LADDER) in W.BATCH_WIDTHS
    # batched variance gradient: every compiled DT edge up to SR_GRAD_MAX_D, and the fall-back beyond it
    _has_edges(W.GRAD_WIDTHS, [e for e in ladder_edges if e < W.SR_GRAD_MAX_D], "predict_grad")
    assert W.SR_GRAD_MAX_D in W.GRAD_WIDTHS and W.SR_GRAD_MAX_D + 1 in W.GRAD_FALLBACK_WIDTHS
    assert max(W.GRAD_WIDTHS) == W.SR_GRAD_MAX_D and min(W.GRAD_FALLBACK_WIDTHS) > W.SR_GRAD_MAX_D


def test_case_lists_cover_every_width():
    """the covering designs: every width of a group meets every kernel and every N of the group"""
    for cases, widths, ns, kts in ((W.LIN_CASES, W.LIN_WIDTHS, W.LIN_NS, W.LIN_KERNELS),
                                   (W.GRAD_CASES, W.GRAD_WIDTHS, W.GRAD_NS, W.GRAD_KERNELS)):
        for D in widths:
            assert {c[2] for c in cases if c[1] == D} == set(ns), D
            assert {c[0] for c in cases if c[1] == D} == set(kts), D
    assert {c[1] for c in W.BATCH_CASES if c[0] == "rbf"} == set(W.BATCH_WIDTHS)
    for D in W.BATCH_WIDTHS:
        assert {c[2] for c in W.BATCH_CASES if c[1] == D} == set(W.BATCH_NS), D
    assert {c[3] for c in W.GRAD_CASES} == {1, 3}
