"""Every threshold of the convolution dispatcher from both sides (tests/dispatch_cases.py), down to 1 x 1 images: one
launch per case through ctx.conv2d_nhwc with the profiler on.

    row      the profiler row is the one tests/dispatch_statement.py names (not asserted when a KOCR_* developer switch
             other than KOCR_SPLIT reroutes the layer: tests/test_fallback_paths_gpu.py runs this file on those kernels);
    values   every output element within the bound the project states for the row that actually ran
             (tests/layer_bounds.family):  k ((T|x| conv |w|) |pre_a| + |pre_b|) + 2^-36 max|x| (1 conv |w|) |pre_a|,
             k = 5e-6 with T = +-3 columns at the layer's dilation for the Winograd rows, 1.5e-6 for the direct split
             kernels, Cin k^2 2^-24 for the fp32 MFMA kernel -- against a float64 convolution of the same float32 inputs;
    shape    exactly (n, h, w, cout);
    batch    image 0 alone gives the same bits as inside its batch wherever the statement names the same row for n = 1
             (the fp16 modes scale per image and flattened tiles span images: what the 256-pixel rule protects);
    control  in f16x1 mode the same check fails on every one-piece F(4,3) row (conv_w4q*).
"""
import os

import numpy as np
import pytest

from tests import dispatch_cases as dc
from tests.dispatch_statement import row as stated_row

pytestmark = pytest.mark.gpu


def _switches_set():
    return any(k.startswith("KOCR_") and k != "KOCR_SPLIT" for k in os.environ)


def _launch(ctx, case, images=None):
    """(output, the convolution's profiler row) of one launch of the case (or of its first `images` images)"""
    p = dc.problem(case)
    x = p["x"] if images is None else p["x"][:images]
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        got = ctx.conv2d_nhwc(x, p["w"], dilation=case[6], pre_a=p["pre_a"], pre_b=p["pre_b"], relu=True)
        rows = ctx.profile_report()
    finally:
        ctx.profile_enable(False)
    conv = sorted(k for k in rows if k.startswith("conv"))
    assert len(conv) == 1, f"{case}: one convolution launch expected, profiler rows {sorted(rows)}"
    return got, conv[0]


def _judge(ctx, case, label):
    """runs the case; asserts row, shape and batch independence; returns (max err / stated bound, the row that ran)"""
    n, h, w, cin, cout, k, dil = case
    mode = ctx.get_split_mode()
    got, ran = _launch(ctx, case)
    want_row = stated_row(n, h, w, cin, cout, k, dil, mode)
    if not _switches_set():
        assert ran == want_row, f"{label} {case}: ran on {ran}, the dispatch statement says {want_row}"
    assert got.shape == (n, h, w, cout) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - dc.problem(case)["want"])
    ratio = float((err / np.maximum(dc.allowed(case, ran), 1e-300)).max())
    print(f"{label} {dc.case_id(case)}: {ran}, max err / stated bound = {ratio:.3f}")
    if n > 1 and stated_row(1, h, w, cin, cout, k, dil, mode) == want_row:
        alone, ran1 = _launch(ctx, case, images=1)
        if ran1 == ran:  # (a developer switch may split what the statement keeps together)
            d = float(np.abs(alone.astype(np.float64) - got[:1]).max())
            assert np.array_equal(alone.view(np.uint32), got[:1].view(np.uint32)), \
                f"{label} {case}: image 0 alone differs from image 0 in the batch by up to {d:.3g} ({ran})"
    return ratio, ran


@pytest.mark.parametrize("case", dc.DEFAULT_CASES, ids=[dc.case_id(c) for c in dc.DEFAULT_CASES])
def test_fp32_class_at_dispatch_edge(ctx, case):
    """the context's own arithmetic (fp16x2 unless the environment says otherwise)"""
    ratio, ran = _judge(ctx, case, "default")
    assert ratio <= 1.0, f"{case} on {ran}: max err / stated bound = {ratio:.3f}"


@pytest.mark.parametrize("case", dc.BF16X3_CASES, ids=[dc.case_id(c) for c in dc.BF16X3_CASES])
def test_fp32_class_at_dispatch_edge_bf16x3(ctx, case):
    """the exact split, set on the context: where the fp16-only arrangements send their shapes"""
    prev = ctx.get_split_mode()
    ctx.set_split_mode("bf16x3")
    try:
        ratio, ran = _judge(ctx, case, "bf16x3")
    finally:
        ctx.set_split_mode(prev)
    assert ratio <= 1.0, f"{case} on {ran}: max err / stated bound = {ratio:.3f}"


def test_fp32_class_edge_checker_rejects_the_f16x1_mode(ctx):
    """Negative control: with one fp16 piece (2^-12 relative) the check above must fail on every case that runs a one-piece
    F(4,3) row -- and hold on the ragged grids, which exist with two pieces only and stay fp32-class in this mode."""
    prev = ctx.get_split_mode()
    ctx.set_split_mode("f16x1")
    try:
        seen = {c: _judge(ctx, c, "f16x1") for c in dc.F16X1_CASES}
    finally:
        ctx.set_split_mode(prev)
    one_piece = {c: r for c, (r, ran) in seen.items() if ran.startswith("conv_w4q")}
    print(f"one-piece F(4,3) rows, max err / stated bound: {one_piece}")
    if not _switches_set():
        assert len(one_piece) >= 3, seen
    assert all(r > 1.0 for r in one_piece.values()), one_piece
    two_piece = {c: r for c, (r, ran) in seen.items() if not ran.startswith("conv_w4q")}
    assert all(r <= 1.0 for r in two_piece.values()), two_piece
