"""The arithmetic modes of the wide convolutions (include/kocr.h KOCR_SPLIT_*) against fp64.

bf16x3: exact 3-way bf16 split, 6 products, every wide layer.  f16x2 (the default since round 4): the Winograd F(4,3)
layers whose images tile as 4 x 64 / 8 x 32 pixels run on the fp16 cores (csrc/conv_w43h.hip): round-to-nearest 2-way
fp16 split, 3 products, inputs scaled by an exact power of two PER IMAGE (from the max |x| slot the producer tracked or a
reduction on demand), weights per output channel; every other layer runs the bf16x3 kernels.  Stated bounds, elementwise,
S = |x| conv |w| in fp64, max|x| taken per image:

    bf16x3:  |err| <= 1e-6 * S
    f16x2 :  |err| <= 1e-6 * S + 2^-36 * max|x| * (1 conv |w|)

The second term is the fp16 low piece going subnormal for elements more than 2^16 below their image's maximum (their
absolute error stays <= 2^-38 max|x|); on tensors of ordinary dynamic range it is far below the first.

f16x1 (KOCR_SPLIT_F16X1, opt-in REDUCED PRECISION fast mode): one fp16 piece per operand, one product -- relative operand
error 2^-12.  Stated tolerance (SURVEY 8(f).4 "re-stated tolerance"):  |err| <= 1e-3 * S + 2^-24 * max|x| * (1 conv |w|)
elementwise and rms(err / S) <= 1e-4 on the F(4,3) layers (measured 1.3-2.8e-4 / 1.8-3.8e-5); CRAFT heat-maps within 5e-3 of the
oracle on maps of magnitude ~3 (measured 1e-3), i.e. 100x the fp32-class modes -- and therefore never a default and never `value` in bench.py.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

MODES = ["bf16x3", "f16x2"]


@pytest.fixture(params=MODES)
def mode_ctx(ctx, request):
    old = ctx.get_split_mode()
    ctx.set_split_mode(request.param)
    yield ctx, request.param
    ctx.set_split_mode(old)


def _ref64(x, w, dil):
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    wt = torch.from_numpy(w).double().permute(3, 2, 0, 1)
    pad = dil * (w.shape[0] // 2)
    want = F.conv2d(xt, wt, None, padding=pad, dilation=dil).permute(0, 2, 3, 1).numpy()
    s = F.conv2d(xt.abs(), wt.abs(), None, padding=pad, dilation=dil).permute(0, 2, 3, 1).numpy()
    ones = F.conv2d(torch.ones_like(xt), wt.abs(), None, padding=pad, dilation=dil).permute(0, 2, 3, 1).numpy()
    return want, s, ones


def _check(got, x, w, dil, mode):
    want, s, ones = _ref64(x, w, dil)
    bound = 1e-6 * s
    if mode == "f16x2":  # per-image max |x|
        amax = np.abs(x).reshape(x.shape[0], -1).max(axis=1).astype(np.float64).reshape(-1, 1, 1, 1)
        bound = bound + 2.0 ** -36 * amax * ones
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    assert np.isfinite(got).all()
    assert worst <= 1.0, f"{mode}: max err / bound = {worst:.3f}"


def _conv_rows(ctx, x, wt, **kw):
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.conv2d_nhwc(x, wt, **kw)
    rows = sorted(k for k in ctx.profile_report() if k.startswith("conv"))
    ctx.profile_enable(False)
    return got, rows


def _plain_env():
    return not any(k.startswith("KOCR_") and k != "KOCR_SPLIT" for k in os.environ)


CASES = [
    # N, H, W, Cin, Cout, k, dil, kernel family in f16x2 mode
    (1, 48, 192, 256, 256, 3, 1, "conv_w4hv_256x128"),   # fp16 F(4,3), 4 x 64 tiles
    (2, 16, 96, 128, 128, 3, 1, "conv_w4ht_256x128"),    # fp16 F(4,3), 8 x 32 tiles, two images
    (1, 32, 128, 64, 64, 3, 1, "conv_w4hr_256x64"),      # 64 couts: fp16 row-reuse kernel, 4 x 64 tiles
    (1, 6, 128, 32, 48, 3, 1, "conv_w4s_256x64"),        # 64 couts, 2 x 128 tiles: bf16x3 row-reuse kernel in both modes
    (1, 96, 96, 128, 192, 1, 1, "conv_ds_256x128"),      # direct split kernel, 1x1 (bf16x3 in both modes)
    (1, 80, 64, 64, 128, 3, 6, "conv_ds_256x128"),       # direct split kernel, dilated, W % 24 != 0
]


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
def test_fp32_class_on_ordinary_data(mode_ctx, case):
    ctx, mode = mode_ctx
    n, h, w, cin, cout, k, dil, family = case
    rng = np.random.default_rng(abs(hash(case[:7])) % 2 ** 32)
    x = np.maximum(rng.standard_normal((n, h, w, cin)), 0).astype(np.float32)
    wt = (rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
    got, rows = _conv_rows(ctx, x, wt, dilation=dil)
    if _plain_env():
        want_row = family if mode == "f16x2" else family.replace("conv_w4hr", "conv_w4s").replace("conv_w4h", "conv_w4")
        assert rows == [want_row], f"{mode}: expected {want_row}, profiler rows {rows}"
    _check(got, x, wt, dil, mode)


@pytest.mark.parametrize("scale_x,scale_w", [(1e-20, 1.0), (1e20, 1e-3), (3e-7, 5e4), (1.0, 1e-25)])
def test_extreme_magnitudes_are_rescaled_exactly(mode_ctx, scale_x, scale_w):
    """The power-of-two scaling must keep tiny / huge tensors inside the fp16 range without losing bits."""
    ctx, mode = mode_ctx
    rng = np.random.default_rng(11)
    x = (np.maximum(rng.standard_normal((1, 40, 64, 64)), 0) * scale_x).astype(np.float32)
    wt = (rng.standard_normal((3, 3, 64, 96)) * 0.05 * scale_w).astype(np.float32)
    got, rows = _conv_rows(ctx, x, wt)
    if _plain_env() and mode == "f16x2":
        assert rows == ["conv_w4hv_256x128"], rows
    _check(got, x, wt, 1, mode)


def test_weights_of_very_different_channels_are_scaled_per_cout(mode_ctx):
    """Output channels whose weights differ by 1e8 in magnitude: the per-cout weight exponent keeps each inside fp16."""
    ctx, mode = mode_ctx
    rng = np.random.default_rng(13)
    x = np.maximum(rng.standard_normal((1, 16, 64, 32)), 0).astype(np.float32)
    wt = (rng.standard_normal((3, 3, 32, 96)) * 0.05).astype(np.float32)
    wt[..., ::3] *= 1e-4
    wt[..., 1::3] *= 1e4
    _check(ctx.conv2d_nhwc(x, wt), x, wt, 1, mode)


def test_wide_dynamic_range_inside_one_tensor(mode_ctx):
    """Half of the image 1e7 times weaker than the other half: the stated f16x2 bound has the additive term."""
    ctx, mode = mode_ctx
    rng = np.random.default_rng(12)
    x = np.maximum(rng.standard_normal((1, 64, 128, 64)), 0).astype(np.float32)
    x[:, :, :64, :] *= 1e3
    x[:, :, 64:, :] *= 1e-4
    wt = (rng.standard_normal((3, 3, 64, 128)) * 0.05).astype(np.float32)
    got = ctx.conv2d_nhwc(x, wt)
    _check(got, x, wt, 1, mode)
    # and the weak half is still resolved to ~5 digits relative to ITSELF in f16x2 (7 in bf16x3)
    want, s, _ = _ref64(x, wt, 1)
    rel = np.abs(got[:, :, 70:, :] - want[:, :, 70:, :]) / s[:, :, 70:, :]
    assert float(rel.max()) <= (1e-6 if mode == "bf16x3" else 2e-4)


def test_every_image_has_its_own_scale(mode_ctx):
    """Images of very different magnitude in one batch: each result is BIT-IDENTICAL to the image convolved alone (the
    input scale is per image: nothing depends on what else is in the batch), and the weak image keeps fp32-class
    accuracy relative to itself."""
    ctx, mode = mode_ctx
    rng = np.random.default_rng(14)
    x = np.maximum(rng.standard_normal((3, 16, 128, 64)), 0).astype(np.float32)
    x[1] *= 1e-6
    x[2] *= 1e5
    wt = (rng.standard_normal((3, 3, 64, 128)) * 0.05).astype(np.float32)
    b = rng.uniform(-0.1, 0.1, 128).astype(np.float32)
    got = ctx.conv2d_nhwc(x, wt, pre_b=b, relu=True)
    for i in range(3):
        alone = ctx.conv2d_nhwc(x[i:i + 1], wt, pre_b=b, relu=True)
        assert np.array_equal(got[i:i + 1], alone), f"{mode}: image {i} depends on its batch"
    _check(ctx.conv2d_nhwc(x, wt), x, wt, 1, mode)


@pytest.mark.parametrize("cout", [64, 128])
def test_all_zero_input(mode_ctx, cout):
    ctx, mode = mode_ctx
    x = np.zeros((1, 32, 64, 64), np.float32)
    wt = np.ones((3, 3, 64, cout), np.float32)
    b = np.linspace(-1, 1, cout).astype(np.float32)
    got = ctx.conv2d_nhwc(x, wt, pre_b=b)
    assert np.array_equal(got, np.broadcast_to(b, got.shape))


def test_heatmaps_agree_between_modes(ctx, craft_weights):
    """Whole CRAFT forward (per-image max|x| slots through convs, pools, the folded decoder, concat buffers)."""
    from oracle import craft as ocraft

    ctx.load_craft(craft_weights)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (2, 128, 192, 3), dtype=np.uint8)
    img[1] //= 6  # a dark page next to a bright one: the two images get different input scales
    want = ocraft.detector_predict(craft_weights, img)
    old = ctx.get_split_mode()
    try:
        out = {}
        for mode in MODES:
            ctx.set_split_mode(mode)
            out[mode] = ctx.craft_forward(img)
            assert float(np.abs(out[mode] - want).max()) <= 5e-5, mode
        assert float(np.abs(out["bf16x3"] - out["f16x2"]).max()) <= 5e-5
        ctx.set_split_mode("f16x2")  # batch invariance of the whole detector in the default mode, bit for bit
        for i in range(2):
            assert np.array_equal(ctx.craft_forward(img[i:i + 1]), out["f16x2"][i:i + 1])
    finally:
        ctx.set_split_mode(old)


def test_crnn_labels_agree_between_modes(ctx, crnn_weights):
    ctx.load_crnn(crnn_weights)
    rng = np.random.default_rng(6)
    crops = rng.random((24, 31, 200), dtype=np.float32)
    old = ctx.get_split_mode()
    try:
        res = {}
        for mode in MODES:
            ctx.set_split_mode(mode)
            res[mode] = ctx.crnn_forward(crops, return_probs=True)
        la, pa = res["bf16x3"]
        lb, pb = res["f16x2"]
        # the CRNN parity bar against the oracle is 1e-4 on the softmax (tests/test_crnn_gpu.py); two
        # fp32-class evaluations of the same graph differ by round-off amplified through the two BiLSTMs
        assert float(np.abs(pa - pb).max()) <= 1e-4
        top2 = np.sort(pa, axis=-1)[..., -2:]
        safe = ((top2[..., 1] - top2[..., 0]) > 1e-3).all(axis=1)
        assert np.array_equal(la[safe], lb[safe])
    finally:
        ctx.set_split_mode(old)


# ---------------------------------------------------------------------------------------------------------------------
# KOCR_SPLIT_F16X1: the reduced-precision fast mode and its stated tolerance
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fast_ctx(ctx):
    old = ctx.get_split_mode()
    ctx.set_split_mode("f16x1")
    yield ctx
    ctx.set_split_mode(old)


FAST_CASES = [
    (1, 48, 192, 256, 256, "conv_w4qv_256x128"),
    (2, 16, 96, 128, 128, "conv_w4qt_256x128"),
    (1, 96, 192, 512, 130, "conv_w4qv_256x128"),
]


@pytest.mark.parametrize("case", FAST_CASES, ids=[str(c) for c in FAST_CASES])
def test_fast_mode_holds_its_stated_tolerance(fast_ctx, case):
    n, h, w, cin, cout, family = case
    rng = np.random.default_rng(abs(hash(case[:5])) % 2 ** 32)
    x = np.maximum(rng.standard_normal((n, h, w, cin)), 0).astype(np.float32)
    wt = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (cin * 9))).astype(np.float32)
    got, rows = _conv_rows(fast_ctx, x, wt)
    if _plain_env():
        assert rows == [family], rows
    want, s, ones = _ref64(x, wt, 1)
    amax = np.abs(x).reshape(n, -1).max(axis=1).astype(np.float64).reshape(-1, 1, 1, 1)
    err = np.abs(got.astype(np.float64) - want)
    ratio = err / np.maximum(s, 1e-300)
    rms = float(np.sqrt((ratio ** 2).mean()))
    print(f"fast conv {case[:5]}: max err / S = {ratio.max():.3e}, rms = {rms:.3e}")
    assert float((err / (1e-3 * s + 2.0 ** -24 * amax * ones)).max()) <= 1.0
    assert rms <= 1e-4
    # ... and it is NOT an fp32-class mode: the test would be vacuous if the full-precision kernel had run
    assert float(ratio.max()) > 5e-6


def test_fast_mode_heatmaps_and_boxes(fast_ctx, craft_weights):
    """CRAFT in the fast mode: heat-maps within the stated 5e-3 of the oracle (maps of magnitude ~3), and the per-image
    scale still makes every image independent of its batch, bit for bit."""
    from oracle import craft as ocraft

    fast_ctx.load_craft(craft_weights)
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (2, 128, 192, 3), dtype=np.uint8)
    want = ocraft.detector_predict(craft_weights, img)
    got = fast_ctx.craft_forward(img)
    err = float(np.abs(got - want).max())
    print(f"fast mode heat-map error {err:.3e} on maps of magnitude {np.abs(want).max():.2f}")
    assert err <= 5e-3
    for i in range(2):
        assert np.array_equal(fast_ctx.craft_forward(img[i:i + 1]), got[i:i + 1])


# ---------------------------------------------------------------------------------------------------------------------
# The epilogues of the exact bf16x3 F(4,3) kernels (csrc/conv_w43.hip) with the affines a network gives them: pre_a != 1,
# a bias, ReLU, the CRNN's post-ReLU BatchNorm.  One small shape per arrangement of that file.
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def bf16x3_ctx(ctx):
    old = ctx.get_split_mode()
    ctx.set_split_mode("bf16x3")
    yield ctx
    ctx.set_split_mode(old)


AFFINE_CASES = [
    # N, H, W, Cin, Cout, dil, profiler row family
    (3, 8, 4, 32, 96, 1, "conv_w4s_256x128"),     # flattened pixels
    (2, 17, 36, 64, 128, 1, "conv_w4s_256x128"),  # flattened pixels, the last tile partly outside
    (1, 12, 24, 32, 96, 2, "conv_w4s_256x128"),   # flattened pixels, dilated
    (1, 17, 36, 32, 48, 1, "conv_w4s_512x64"),    # 64 couts, flattened pixels
    (1, 6, 128, 32, 48, 1, "conv_w4s_256x64"),    # 64 couts, row reuse on 2 x 128 tiles
    (3, 12, 64, 32, 33, 1, "conv_w4s_256x64"),    # 64 couts, row reuse on 4 x 64 tiles
    (1, 4, 192, 32, 130, 1, "conv_w4v_256x128"),  # vertical reuse on 4 x 64 tiles
    (1, 8, 32, 32, 130, 1, "conv_w4t_256x128"),   # vertical reuse on 8 x 32 tiles
]


@pytest.mark.parametrize("case", AFFINE_CASES, ids=[str(c) for c in AFFINE_CASES])
@pytest.mark.parametrize("variant", ["bias_relu", "relu_then_bn", "linear"])
def test_bf16x3_w43_epilogue_affines(bf16x3_ctx, case, variant):
    """|err| <= 1.25e-6 * B elementwise against fp64, with S = |x| conv |w| and B = (S |pre_a| + |pre_b|) |post_a| + |post_b|
    (B = S |pre_a| + |pre_b| without a post affine): 1e-6 S is the kernels' stated bound, the two affines add at most four
    fp32 roundings of 2^-24 each on quantities no larger than B, and ReLU is 1-Lipschitz."""
    n, h, w, cin, cout, dil, family = case
    rng = np.random.default_rng([AFFINE_CASES.index(case), ["bias_relu", "relu_then_bn", "linear"].index(variant)])
    x = rng.standard_normal((n, h, w, cin), dtype=np.float32)
    wt = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (cin * 9))).astype(np.float32)
    pre_a = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    pre_b = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
    post_a = post_b = None
    relu = variant != "linear"
    if variant == "relu_then_bn":
        post_a = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        post_b = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
    got, rows = _conv_rows(bf16x3_ctx, x, wt, dilation=dil, pre_a=pre_a, pre_b=pre_b, relu=relu, post_a=post_a, post_b=post_b)
    if _plain_env():
        assert len(rows) == 1 and rows[0].startswith(family), f"expected {family}*, profiler rows {rows}"
        assert not rows[0].startswith(("conv_w4h", "conv_w4q")), rows
    conv, s, _ = _ref64(x, wt, dil)
    want = conv * pre_a.astype(np.float64) + pre_b.astype(np.float64)
    bound = s * np.abs(pre_a).astype(np.float64) + np.abs(pre_b).astype(np.float64)
    if relu:
        want = np.maximum(want, 0.0)
    if post_a is not None:
        want = want * post_a.astype(np.float64) + post_b.astype(np.float64)
        bound = bound * np.abs(post_a).astype(np.float64) + np.abs(post_b).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / (1.25e-6 * bound)).max())
    print(f"bf16x3 F(4,3) epilogue {case[:6]} {variant}: max err / (1.25e-6 B) = {worst:.3f}")
    assert np.isfinite(got).all()
    assert worst <= 1.0, f"max err / bound = {worst:.3f}"
