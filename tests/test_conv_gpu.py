"""Parity of the MFMA implicit-GEMM convolution (csrc/conv_mfma.hip) against a plain
PyTorch fp32 reference of the same op (floating-point kernel -> torch fp32 reference).

Tolerance: both sides accumulate in fp32 in different orders; |err| <= 2e-5 * sqrt(K) *
max|out| is far above fp32 round-off for these sizes and far below the heat-map tolerance.
"""
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _seed(*key):
    """per-case seed that does not depend on PYTHONHASHSEED (str hashes are salted per process)"""
    return zlib.crc32(repr(key).encode())


CASES = [
    # N, H, W, Cin, Cout, k, dil
    (1, 16, 16, 16, 32, 3, 1),
    (2, 17, 23, 64, 64, 3, 1),     # ragged pixel count, 256x64 tile
    (1, 24, 40, 128, 256, 3, 1),   # 128x128 tile, 2 n-tiles
    (2, 9, 11, 32, 16, 3, 1),      # Cout < 32
    (1, 20, 12, 16, 2, 1, 1),      # conv_cls.8 shape class
    (1, 14, 14, 512, 1024, 3, 6),  # dilated slice5.1 class (reduced spatial)
    (1, 12, 12, 1536, 512, 1, 1),  # upconv1.conv.0 class
    (3, 13, 10, 3, 64, 3, 1),      # Cin = 3 scalar gather
    (2, 31, 20, 1, 64, 3, 1),      # Cin = 1 (CRNN conv_1 class)
    (1, 50, 7, 512, 16, 5, 1),     # STN localisation conv (5x5)
    (4, 1, 1, 11200, 64, 1, 1),    # dense as 1x1 conv
    (1, 50, 1, 256, 37, 1, 1),     # fc_12 class (Cout = 37)
    # W % 128 == 0, 3x3, Cin % 16 == 0 (round 1's fp32 Winograd shape class; <= 32 couts now on conv_hs, the rest on F(4,3) / fp32 MFMA)
    (1, 8, 128, 16, 32, 3, 1),
    (2, 6, 256, 64, 64, 3, 1),
    (1, 5, 128, 128, 200, 3, 1),
    (1, 3, 384, 256, 64, 3, 1),
    # even W, tiles crossing rows and images, ragged last tile (per-pair row-edge masks)
    (2, 7, 10, 16, 32, 3, 1),
    (1, 9, 96, 32, 64, 3, 1),
    (3, 5, 6, 16, 16, 3, 1),
    (1, 2, 2, 48, 70, 3, 1),
]


def _ref(x, w, dil, pre_a, pre_b, relu, post_a, post_b):
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    wt = torch.from_numpy(w).permute(3, 2, 0, 1)  # HWIO -> OIHW
    kh, kw = w.shape[:2]
    y = F.conv2d(xt, wt, None, padding=(dil * (kh - 1) // 2, dil * (kw - 1) // 2), dilation=dil)
    y = y * torch.from_numpy(pre_a).view(1, -1, 1, 1) + torch.from_numpy(pre_b).view(1, -1, 1, 1)
    if relu:
        y = F.relu(y)
    if post_a is not None:
        y = y * torch.from_numpy(post_a).view(1, -1, 1, 1) + torch.from_numpy(post_b).view(1, -1, 1, 1)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


@pytest.mark.parametrize("case", CASES, ids=[str(c) for c in CASES])
@pytest.mark.parametrize("variant", ["bias_relu", "relu_then_bn", "linear"])
def test_conv_matches_torch(ctx, case, variant):
    n, h, w, cin, cout, k, dil = case
    rng = np.random.default_rng(_seed(case, variant))
    x = rng.standard_normal((n, h, w, cin), dtype=np.float32)
    wt = (rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
    pre_a = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    pre_b = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
    post_a = post_b = None
    relu = variant != "linear"
    if variant == "relu_then_bn":  # CRNN bn_3/5/7 placement (recognition.py:226-242)
        post_a = rng.uniform(0.5, 1.5, cout).astype(np.float32)
        post_b = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
    got = ctx.conv2d_nhwc(x, wt, dilation=dil, pre_a=pre_a, pre_b=pre_b, relu=relu, post_a=post_a, post_b=post_b)
    want = _ref(x, wt, dil, pre_a, pre_b, relu, post_a, post_b)
    tol = 2e-5 * np.sqrt(cin * k * k) * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    assert got.shape == want.shape
    assert err <= tol, f"max abs err {err} > {tol}"


def test_conv_transpose_detecting(ctx):
    """A = identity-like probe with an ASYMMETRIC weight matrix: catches a swapped C/D map."""
    cin, cout = 32, 64
    x = np.zeros((1, 8, 8, cin), np.float32)
    for c in range(cin):
        x[0, c // 8, c % 8, c] = 1.0
    w = (np.arange(cin * cout, dtype=np.float32).reshape(1, 1, cin, cout) + 1) / 100.0
    got = ctx.conv2d_nhwc(x, w)
    want = np.einsum("nhwc,co->nhwo", x, w[0, 0])
    assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------
# conv_wsplit.hip: 3x3 convolutions run on the bf16 matrix cores with every fp32 operand split exactly
# into three bf16 pieces and six of the nine piece products kept.  The claim to defend is "fp32-class":
# the error against an fp64 convolution of the same fp32 inputs must stay at fp32 round-off level,
#     |err| <= 1e-6 * (|x| conv |w|)     elementwise
# (a plain fp32 fma chain of K = 9*Cin terms has a worst case of K * 6e-8 and typically 2e-7 of that
# bound; a kernel that dropped the third piece would sit at 4e-6..4e-5).  Shapes are chosen so that the
# persistent blocks walk over several tiles each and both tile shapes (128 px x 128 couts, 256 px x 64
# couts) and odd/even K-step counts are hit.
# ---------------------------------------------------------------------------------------------------
# Every case names the kernel family it must run on in the DEFAULT arithmetic (fp16x2 F(4,3) where an fp16 arrangement
# exists, else the exact bf16x3 kernels); under KOCR_SPLIT=bf16 "conv_w4h" reads "conv_w4".  The profiler row of the
# launch is asserted (a dispatch regression must not pass silently), unless a KOCR_* developer switch
# reroutes the layer (tests/test_fallback_paths_gpu.py).
SPLIT_CASES = [
    # N, H, W, Cin, Cout, family
    (1, 96, 192, 256, 256, "conv_w4hv_256x128"),   # 288 tiles > 256 CUs: blocks take a second tile; vertical reuse, 4 x 64
    (2, 64, 128, 64, 64, "conv_w4hr_256x64"),       # 64 couts: row-reuse arrangement, 4 x 64
    (1, 40, 64, 48, 96, "conv_ws_128x128"),        # Cin % 32 != 0: F(2,3) kernel, 9 K-steps (odd)
    (1, 30, 50, 512, 130, "conv_w4hv_256x128_rag"),  # W % 4 != 0: the ragged 4 x 64 grid (one tile column, 14 columns of padding); F(2,3) in bf16x3 mode
    # conv_w43.hip (Winograd F(4,3): Cin % 32 == 0, Cout > 64, W % 4 == 0)
    (1, 30, 52, 512, 130, "conv_w4hf_256x128"),     # H % 4 != 0: flattened-pixel tiles, ragged couts, last tile partly outside
    (2, 17, 36, 64, 128, "conv_w4hf_256x128"),      # 12 K-steps, two images, odd height
    (1, 64, 128, 128, 256, "conv_w4hv_256x128"),   # two cout tiles per pixel tile
    (3, 8, 4, 32, 96, "conv_w4s_256x128"),         # a single quad per row: both column paddings in one quad
    # 32 < Cout <= 64: the 64-cout arrangement of conv_w43.hip (512-pixel tiles, two gather items per thread)
    (1, 17, 36, 32, 48, "conv_w4s_512x64"),        # ragged couts, odd height, last tile mostly outside
    (2, 40, 128, 128, 64, "conv_w4hr_256x64"),      # upconv3.conv.3 class (row reuse, 4 x 64)
    # 32 < Cout <= 64 on images that tile as 4 rows x 64 columns / 2 rows x 128 columns: the row-reuse arrangement
    (1, 6, 128, 32, 48, "conv_w4s_256x64"),        # 2 x 128 (H % 4 != 0): two channel groups, one tile per row pair, ragged couts
    (2, 8, 256, 64, 64, "conv_w4hr_256x64"),        # 4 x 64: slice1.3 class, four channel groups, four tiles per row quad, two images
    (1, 4, 384, 96, 40, "conv_w4hr_256x64"),        # 4 x 64: six channel groups, one row quad
    (2, 10, 256, 64, 64, "conv_w4s_256x64"),       # 2 x 128: two tiles per row pair, two images
    (3, 12, 64, 32, 33, "conv_w4hr_256x64"),        # 4 x 64: one tile per row quad, one live column in the second cout half
    # Cout > 64 on images that tile as 4 rows x 64 columns or 8 rows x 32 columns: the vertical-reuse arrangement
    (2, 8, 256, 64, 128, "conv_w4hv_256x128"),     # 4 x 64: slice1.7 class, four channel groups, four tiles per row quad, two images
    (1, 4, 192, 32, 130, "conv_w4hv_256x128"),     # 4 x 64: one row quad (both vertical paddings in every tile), ragged couts
    (3, 12, 64, 96, 96, "conv_w4hv_256x128"),      # 4 x 64: one tile per row quad (both column paddings in every tile)
    (2, 16, 96, 64, 128, "conv_w4ht_256x128"),     # 8 x 32: slice4.34 class geometry (96 wide), two images
    (1, 8, 32, 32, 130, "conv_w4ht_256x128"),      # 8 x 32: a single tile per image (all four paddings), ragged couts
    (3, 24, 160, 96, 96, "conv_w4ht_256x128"),     # 8 x 32: five column blocks, three row octets, three images
    (1, 6, 128, 32, 130, "conv_w4hf_256x128"),
    (5, 31, 200, 64, 128, "conv_w4ht_256x128_rag"),  # 31 x 200 images: the ragged 8 x 32 grid (32 x 224: 16 % padding)
    (7, 15, 100, 256, 130, "conv_w4hf_256x128"),   # conv_5 class: 1500-pixel crops, ragged couts, last tile partly outside      # H % 4 != 0: stays on conv_w43_kernel (flattened-pixel tiles)
    # round 5: ragged images (any H, W) on the vertical- / row-reuse kernels: masked gather, masked stores
    (1, 93, 125, 64, 128, "conv_w4hv_256x128_rag"),   # CRAFT 1/16 level of a 1500 x 2000 page: odd width and height
    (2, 46, 250, 128, 256, "conv_w4hv_256x128_rag"),  # W % 4 == 2: the last quad of a row has two live columns; two images, two cout blocks
    (1, 187, 250, 32, 130, "conv_w4hv_256x128_rag"),  # 1/8 level, ragged couts, H % 4 == 3
    (1, 50, 1000, 32, 128, "conv_w4hv_256x128_rag"),  # W % 4 == 0 but not a multiple of 64: 16 tile columns, the last one 40 wide
    (2, 30, 90, 96, 96, "conv_w4ht_256x128_rag"),     # 8 x 32 grid (96 wide covers 90 with less padding than 128), H % 8 == 6
    (1, 9, 33, 64, 96, "conv_w4hv_256x128_rag"),      # W % 4 == 1 on a tiny image: one tile column (31 columns of padding), three row quads, the last with one live row
    (1, 75, 125, 64, 64, "conv_w4hr_256x64_rag"),     # 64 couts (slice1.3 class) on a ragged image: row reuse, exchange epilogue
    (2, 94, 250, 128, 48, "conv_w4hr_256x64_rag"),    # ... ragged couts, two images
    (3, 5, 66, 32, 64, "conv_w4hr_256x64_rag"),       # two live columns in the second tile column, H % 4 == 1
    # Cout <= 32 (conv_hsplit.hip: haloed 8x32 tile split once into LDS; any size since round 6 -- the small ones are in tests/dispatch_cases.py)
    (1, 64, 64, 32, 32, "conv_hh_256x32"),         # conv_cls.0 / .2 class, tiles exact
    (2, 70, 45, 64, 32, "conv_hh_256x32"),         # upconv4.conv.3 class: 4 chunks, ragged tiles in both directions, two images
    (1, 67, 100, 32, 16, "conv_hs_256x16"),        # conv_cls.4 class: the 16-wide product tile
    (1, 130, 33, 16, 7, "conv_hs_256x16"),         # one chunk, a single used column in the second tile column
]


def _expect_family(ctx, rows, family):
    """The profiler must show the launch on `family` (name of the default arithmetic; KOCR_SPLIT=bf16 maps the fp16 rows
    back to their bf16x3 kernels).  Skipped when a KOCR_* developer switch other than KOCR_SPLIT is set."""
    if any(k.startswith("KOCR_") and k not in ("KOCR_SPLIT",) for k in os.environ):
        return
    if ctx.get_split_mode() == 0 and family.endswith("_rag"):
        return  # the ragged grids exist in the fp16 kernels only: in bf16x3 mode these shapes take whatever took them before
    if ctx.get_split_mode() == 0:
        family = family.replace("conv_w4hr", "conv_w4s").replace("conv_w4hf", "conv_w4s").replace("conv_w4h", "conv_w4").replace("conv_hh", "conv_hs")
    conv = sorted(k for k in rows if k.startswith("conv"))
    assert conv == [family], f"expected the launch on {family}, profiler rows: {sorted(rows)}"


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[str(c) for c in SPLIT_CASES])
def test_split_kernel_is_fp32_class_against_fp64(ctx, case):
    n, h, w, cin, cout, family = case
    rng = np.random.default_rng(_seed(case[:5]))
    x = np.maximum(rng.standard_normal((n, h, w, cin)), 0).astype(np.float32)  # post-ReLU-like, half zeros
    wt = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (cin * 9))).astype(np.float32)
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.conv2d_nhwc(x, wt).astype(np.float64)
    rows = ctx.profile_report()
    ctx.profile_enable(False)
    _expect_family(ctx, rows, family)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    wtt = torch.from_numpy(wt).double().permute(3, 2, 0, 1)
    want = F.conv2d(xt, wtt, None, padding=1).permute(0, 2, 3, 1).numpy()
    bound = F.conv2d(xt.abs(), wtt.abs(), None, padding=1).permute(0, 2, 3, 1).numpy()
    ratio = np.abs(got - want) / np.maximum(bound, 1e-30)
    rms = float(np.sqrt((ratio ** 2).mean()))
    print(f"split conv {case[:5]} on {family}: max err / (|x| conv |w|) = {ratio.max():.3e}, rms = {rms:.3e}")
    assert float(ratio.max()) <= 1e-6, f"max err / (|x| conv |w|) = {ratio.max():.3e}"
    assert rms <= 1.5e-7, f"rms = {rms:.3e}"


def test_switches_act_per_context(monkeypatch):
    """The kernel selection switches are read when a context is created (kocr_create), not once per process: KOCR_W43R=0
    moves a 64-cout layer that tiles 4 x 64 off the row-reuse arrangement (onto conv_w43n_kernel's 512 x 64 tiles), and a
    context created after the switch is unset in the same process is back on it."""
    import keras_ocr_amd

    if any(k.startswith("KOCR_") and k != "KOCR_DISPATCH_LOG" for k in os.environ):
        pytest.skip("a KOCR_* switch is set for the whole process")
    rng = np.random.default_rng(_seed("switches_per_context"))
    x = np.maximum(rng.standard_normal((2, 64, 128, 64)), 0).astype(np.float32)
    wt = (rng.standard_normal((3, 3, 64, 64)) * np.sqrt(2.0 / (64 * 9))).astype(np.float32)

    def conv_rows():
        c = keras_ocr_amd.Context(0)
        try:
            c.profile_enable(True)
            c.conv2d_nhwc(x, wt)
            return sorted(k for k in c.profile_report() if k.startswith("conv"))
        finally:
            c.close()

    monkeypatch.setenv("KOCR_W43R", "0")
    assert conv_rows() == ["conv_w4s_512x64"]
    monkeypatch.delenv("KOCR_W43R")
    assert conv_rows() == ["conv_w4hr_256x64"]

# conv_k5.hip: 5x5, 16 couts, images of <= 384 pixels (the recogniser's stn_conv_1, recognition.py:259-262): one image
# per block, two taps per MFMA K-step
K5_CASES = [
    # N, H, W, Cin
    (3, 7, 50, 512),    # stn_conv_1 itself: 22 tiles (6 / 6 / 5 / 5 per wave), the last one partly outside
    (2, 5, 33, 32),     # two chunks, 11 tiles (some waves own 2, some 3), ragged last tile
    (5, 1, 9, 16),      # a single row, a single chunk, a single partly-filled tile: every tap but the centre row is padding
    (1, 16, 24, 48),    # the largest pixel count the kernel takes (384 = 24 full tiles)
]


@pytest.mark.parametrize("case", K5_CASES, ids=[str(c) for c in K5_CASES])
def test_k5_kernel_is_fp32_class_against_fp64(ctx, case):
    n, h, w, cin = case
    cout = 16
    rng = np.random.default_rng(_seed(case))
    x = np.maximum(rng.standard_normal((n, h, w, cin)), 0).astype(np.float32)
    wt = (rng.standard_normal((5, 5, cin, cout)) * np.sqrt(2.0 / (cin * 25))).astype(np.float32)
    pre_b = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.conv2d_nhwc(x, wt, pre_b=pre_b, relu=True).astype(np.float64)
    rows = ctx.profile_report()
    ctx.profile_enable(False)
    if os.environ.get("KOCR_K5", "1") != "0":
        assert any(k.startswith("conv_k5") for k in rows), f"conv_k5 did not run: {sorted(rows)}"
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    wtt = torch.from_numpy(wt).double().permute(3, 2, 0, 1)
    b = torch.from_numpy(pre_b).double().view(1, -1, 1, 1)
    want = F.relu(F.conv2d(xt, wtt, None, padding=2) + b).permute(0, 2, 3, 1).numpy()
    bound = (F.conv2d(xt.abs(), wtt.abs(), None, padding=2) + b.abs()).permute(0, 2, 3, 1).numpy()
    ratio = np.abs(got - want) / np.maximum(bound, 1e-30)
    print(f"k5 conv {case}: max err / bound = {ratio.max():.3e}, rms = {np.sqrt((ratio ** 2).mean()):.3e}")
    assert got.shape == want.shape
    assert float(ratio.max()) <= 1e-6, f"max err / bound = {ratio.max():.3e}"


# conv_dsplit.hip: the same bf16x3 arithmetic for 1x1 / dilated / larger kernels (>= 4096 pixels)
DSPLIT_CASES = [
    # N, H, W, Cin, Cout, k, dil, family
    (1, 96, 96, 512, 256, 3, 6, "conv_w4hf_256x128_dil"),   # slice5.1 class: dilated, W % (4 dil) == 0 -> F(4,3) on the comb of pixels
    (2, 64, 72, 1024, 128, 1, 1, "conv_ds_256x128"),       # slice5.2 class
    (1, 192, 192, 192, 64, 1, 1, "conv_ds_512x64"),        # upconv4.conv.0 class: 512x64 tiles
    (1, 70, 61, 48, 100, 1, 1, "conv_ds_256x128"),         # ragged pixels / couts, 3 K-steps
    (1, 65, 67, 32, 40, 5, 1, "conv_ds_512x64"),           # 5x5, tiles crossing rows, odd sizes
    (2, 50, 90, 64, 70, 3, 2, "conv_ds_256x128"),          # dilation 2, W % 8 != 0: direct split kernel, two images
    (2, 48, 48, 64, 128, 3, 6, "conv_w4hf_256x128_dil"),    # slice5.1 geometry at 768x768 input
    (1, 33, 40, 32, 96, 3, 2, "conv_w4hf_256x128_dil"),     # dilation 2, odd height, ragged couts, tile ends inside a row
    (3, 24, 48, 64, 130, 3, 6, "conv_w4hf_256x128_dil"),    # three images of 288 quads: tiles crossing images (two scales per tile), ragged couts
]


@pytest.mark.parametrize("case", DSPLIT_CASES, ids=[str(c) for c in DSPLIT_CASES])
def test_direct_split_kernel_is_fp32_class_against_fp64(ctx, case):
    n, h, w, cin, cout, k, dil, family = case
    rng = np.random.default_rng(_seed(case[:7]))
    x = np.maximum(rng.standard_normal((n, h, w, cin)), 0).astype(np.float32)
    wt = (rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
    pre_a = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    pre_b = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
    ctx.profile_enable(True)
    ctx.profile_reset()
    got = ctx.conv2d_nhwc(x, wt, dilation=dil, pre_a=pre_a, pre_b=pre_b, relu=True).astype(np.float64)
    rows = ctx.profile_report()
    ctx.profile_enable(False)
    _expect_family(ctx, rows, family)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    wtt = torch.from_numpy(wt).double().permute(3, 2, 0, 1)
    pad = dil * (k // 2)
    a = torch.from_numpy(pre_a).double().view(1, -1, 1, 1)
    b = torch.from_numpy(pre_b).double().view(1, -1, 1, 1)
    want = F.relu(F.conv2d(xt, wtt, None, padding=pad, dilation=dil) * a + b).permute(0, 2, 3, 1).numpy()
    bound = (F.conv2d(xt.abs(), wtt.abs(), None, padding=pad, dilation=dil) * a + b.abs()).permute(0, 2, 3, 1).numpy()
    ratio = np.abs(got - want) / np.maximum(bound, 1e-30)
    assert got.shape == want.shape
    assert float(ratio.max()) <= 1e-6, f"max err / bound = {ratio.max():.3e}"
