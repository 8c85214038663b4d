"""Shapes on the two sides of every threshold of the convolution dispatcher (tests/dispatch_statement.py), and what
tests/test_dispatch_edges_gpu.py needs to judge a launch: the inputs, the float64 reference and the stated bound.

A case is (N, H, W, Cin, Cout, k, dil).  DEFAULT lists each case with the row the default arithmetic (fp16x2) is read to
reach; tests/test_dispatch_statement_cpu.py holds that column against the statement, the GPU test asserts the statement.
PAIRS names the two sides of one predicate: two different rows.

Out of reach of a test of this size, and not covered here: the 2^29-pixel limit of the F(4,3) family and the 2^31-byte
image limits of the reuse arrangements (w43_small) and of conv_hs* (hsplit_applicable).
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests.layer_bounds import family

# ---- wide F(4,3), Cout > 64 ----------------------------------------------------------------------------------------
TINY_RAGGED = [
    (1, 1, 1, 32, 96, 3, 1),     # one live pixel in a 256-pixel tile, all four paddings in one quad
    (3, 2, 2, 64, 128, 3, 1),    # three images of one half-filled quad row each
    (2, 3, 5, 32, 130, 3, 1),    # W % 4 == 1: a second quad with one live column; ragged couts
    (1, 1, 7, 64, 96, 3, 1),     # one row: both vertical taps are padding
]
PIXELS_240, PIXELS_256, PIXELS_272 = (3, 15, 16, 32, 96, 3, 1), (3, 16, 16, 32, 96, 3, 1), (4, 17, 16, 32, 96, 3, 1)
# the images of these three cases are scaled so that a wrong per-image scale cannot hide
IMAGE_SCALES = {PIXELS_240: (1.0, 2.0 ** -9, 2.0 ** 7), PIXELS_256: (1.0, 2.0 ** -9, 2.0 ** 7),
                PIXELS_272: (1.0, 2.0 ** -9, 2.0 ** 7, 1.0)}
SHARE_52, SHARE_48 = (1, 8, 52, 64, 128, 3, 1), (1, 8, 48, 64, 128, 3, 1)        # padding share 64/52 <= 1.25 < 64/48
SHARE_104, SHARE_100 = (1, 8, 104, 64, 128, 3, 1), (1, 8, 100, 64, 128, 3, 1)    # the same with two tile columns
GEO_4X64, GEO_8X32 = (1, 4, 90, 32, 96, 3, 1), (1, 8, 90, 32, 96, 3, 1)          # 4 x 128 against 8 x 96 covering pixels

DEFAULT = [
    (TINY_RAGGED[0], "conv_w4hv_256x128_rag"),
    (TINY_RAGGED[1], "conv_w4hv_256x128_rag"),
    (TINY_RAGGED[2], "conv_w4hv_256x128_rag"),
    (TINY_RAGGED[3], "conv_w4hv_256x128_rag"),
    (GEO_4X64, "conv_w4hv_256x128_rag"),
    (GEO_8X32, "conv_w4ht_256x128_rag"),
    (PIXELS_240, "conv_w4s_256x128"),     # under 256 pixels: bf16x3 flattened, tiles span images
    (PIXELS_256, "conv_w4hf_256x128"),    # fp16 flattened, one tile is one image
    (PIXELS_272, "conv_w4hf_256x128"),    # every tile holds parts of two images, two scales
    (SHARE_52, "conv_w4hv_256x128_rag"),
    (SHARE_48, "conv_w4hf_256x128"),
    (SHARE_104, "conv_w4hv_256x128_rag"),
    (SHARE_100, "conv_w4hf_256x128"),
    ((1, 4, 64, 32, 65, 3, 1), "conv_w4hv_256x128"),     # one exact 4 x 64 tile, one live column in the third 32-cout tile
    ((1, 4, 64, 32, 129, 3, 1), "conv_w4hv_256x128"),    # ... one live column in the second cout block
    ((1, 8, 32, 32, 129, 3, 1), "conv_w4ht_256x128"),    # one exact 8 x 32 tile
    # ---- narrow F(4,3), 32 < Cout <= 64 ----
    ((1, 1, 1, 32, 64, 3, 1), "conv_w4hr_256x64_rag"),
    ((2, 3, 6, 32, 33, 3, 1), "conv_w4hr_256x64_rag"),
    ((1, 4, 64, 32, 64, 3, 1), "conv_w4hr_256x64"),      # the smallest 4 x 64
    ((1, 2, 128, 32, 48, 3, 1), "conv_w4s_256x64"),      # the smallest 2 x 128
    ((1, 2, 64, 32, 64, 3, 1), "conv_w4s_512x64"),       # neither geometry, 128 pixels: the flattened 512 x 64 tiles
    ((1, 9, 33, 32, 33, 3, 1), "conv_w4hr_256x64_rag"),
    ((1, 9, 33, 32, 32, 3, 1), "conv_hh_256x32"),        # 33 -> 32 couts: conv_hs*
    # ---- conv_hs* at any size ----
    ((1, 1, 1, 16, 32, 3, 1), "conv_hh_256x32"),
    ((2, 3, 5, 16, 17, 3, 1), "conv_hh_256x32"),
    ((2, 3, 5, 16, 16, 3, 1), "conv_hs_256x16"),         # the 16-wide product tile
    ((1, 8, 32, 16, 7, 3, 1), "conv_hs_256x16"),         # one exact tile
    ((1, 9, 33, 48, 32, 3, 1), "conv_hh_256x32"),        # one live row and column in the second tiles
    # ---- dilated ----
    ((1, 8, 24, 32, 96, 3, 6), "conv_w4s_256x128_dil"),  # 192 pixels: the bf16x3 comb
    ((1, 12, 24, 32, 96, 3, 6), "conv_w4hf_256x128_dil"),  # 288 pixels: the fp16 comb
    ((1, 12, 20, 32, 96, 3, 6), "conv_mfma_128x128_m0"),  # W % 24 != 0 below 4096 pixels
    ((1, 1, 24, 32, 96, 3, 6), "conv_w4s_256x128_dil"),  # every tap but the centre is padding
    # ---- conv_ds at 4096 pixels ----
    ((1, 63, 65, 64, 100, 1, 1), "conv_mfma_128x128_m0"),
    ((1, 64, 64, 64, 100, 1, 1), "conv_ds_256x128"),
    ((2, 32, 64, 64, 100, 1, 1), "conv_ds_256x128"),     # 4096 pixels made of two images
    ((1, 63, 65, 32, 40, 5, 1), "conv_mfma_128x64_m0"),
    ((1, 64, 64, 32, 40, 5, 1), "conv_ds_512x64"),
    ((1, 63, 65, 64, 70, 3, 2), "conv_mfma_128x128_m0"),   # dilation 2, W % 8 != 0
    ((1, 64, 66, 64, 70, 3, 2), "conv_ds_256x128"),
    # ---- conv_k5 (5 x 5, 16 couts) ----
    ((2, 4, 81, 32, 16, 5, 1), "conv_k5_352x16"),        # halo plane exactly full: 8 x 85 = 680
    ((1, 1, 132, 16, 16, 5, 1), "conv_k5_352x16"),       # ... 5 x 136 = 680
    ((1, 4, 82, 32, 16, 5, 1), "conv_mfma_128x32_m0"),   # 8 x 86 = 688
    ((1, 1, 133, 16, 16, 5, 1), "conv_mfma_128x32_m0"),  # 5 x 137 = 685
    ((1, 12, 32, 16, 16, 5, 1), "conv_k5_352x16"),       # 384 pixels, halo 576
    ((1, 20, 20, 16, 16, 5, 1), "conv_mfma_128x32_m0"),  # 400 pixels, halo 576: the pixel limit alone
    # ---- F(2,3) conv_ws and the fp32 kernel ----
    ((1, 1, 2, 16, 48, 3, 1), "conv_ws_256x64"),
    ((1, 3, 4, 48, 96, 3, 1), "conv_ws_128x128"),
    ((1, 3, 5, 48, 96, 3, 1), "conv_mfma_128x128_m0"),   # odd W
    ((1, 1, 1, 20, 40, 3, 1), "conv_mfma_128x64_m1"),    # Cin % 16 != 0: the scalar gather on one pixel
]
DEFAULT_CASES = [c for c, _ in DEFAULT]

# ---- bf16x3 mode (set on the context): where the fp16-only arrangements send their shapes ----
BF16X3 = [
    (TINY_RAGGED[0], "conv_mfma_128x128_m0"),
    (TINY_RAGGED[1], "conv_ws_128x128"),
    (TINY_RAGGED[2], "conv_mfma_128x128_m0"),
    (TINY_RAGGED[3], "conv_mfma_128x128_m0"),
    (PIXELS_240, "conv_w4s_256x128"),
    (PIXELS_256, "conv_w4s_256x128"),
    (PIXELS_272, "conv_w4s_256x128"),
    (SHARE_52, "conv_w4s_256x128"),
]
BF16X3_CASES = [c for c, _ in BF16X3]

# ---- f16x1 control: one fp16 piece must miss the fp32-class bound wherever a conv_w4q* row runs ----
F16X1 = [
    (TINY_RAGGED[0], "conv_w4hv_256x128_rag"),   # the ragged grids exist with two pieces only: fp32-class even here
    (TINY_RAGGED[1], "conv_w4hv_256x128_rag"),
    (TINY_RAGGED[2], "conv_w4hv_256x128_rag"),
    (TINY_RAGGED[3], "conv_w4hv_256x128_rag"),
    (PIXELS_256, "conv_w4qf_256x128"),
    (PIXELS_272, "conv_w4qf_256x128"),
    (SHARE_48, "conv_w4qf_256x128"),
    ((1, 4, 64, 32, 129, 3, 1), "conv_w4qv_256x128"),
    ((1, 8, 32, 32, 129, 3, 1), "conv_w4qt_256x128"),
    ((1, 4, 64, 32, 64, 3, 1), "conv_w4qr_256x64"),
]
F16X1_CASES = [c for c, _ in F16X1]

# the two sides of one predicate, default mode: two different rows
PAIRS = [
    ("4 x 64 against 8 x 32 ragged geometry (c1 <= 1.02 c2)", GEO_4X64, GEO_8X32),
    ("256 pixels per image", PIXELS_240, PIXELS_256),
    ("padding share 1.25, one tile column", SHARE_52, SHARE_48),
    ("padding share 1.25, two tile columns", SHARE_104, SHARE_100),
    ("exact 4 x 64 against exact 8 x 32", (1, 4, 64, 32, 129, 3, 1), (1, 8, 32, 32, 129, 3, 1)),
    ("narrow 4 x 64 against 2 x 128", (1, 4, 64, 32, 64, 3, 1), (1, 2, 128, 32, 48, 3, 1)),
    ("narrow 4 x 64 against neither geometry", (1, 4, 64, 32, 64, 3, 1), (1, 2, 64, 32, 64, 3, 1)),
    ("33 against 32 couts", (1, 9, 33, 32, 33, 3, 1), (1, 9, 33, 32, 32, 3, 1)),
    ("17 against 16 couts", (2, 3, 5, 16, 17, 3, 1), (2, 3, 5, 16, 16, 3, 1)),
    ("64 against 65 couts", (1, 4, 64, 32, 64, 3, 1), (1, 4, 64, 32, 65, 3, 1)),
    ("dilated, 256 pixels", (1, 8, 24, 32, 96, 3, 6), (1, 12, 24, 32, 96, 3, 6)),
    ("dilated, W % (4 dil)", (1, 12, 24, 32, 96, 3, 6), (1, 12, 20, 32, 96, 3, 6)),
    ("4096 pixels, 1 x 1", (1, 63, 65, 64, 100, 1, 1), (1, 64, 64, 64, 100, 1, 1)),
    ("4096 pixels, 5 x 5", (1, 63, 65, 32, 40, 5, 1), (1, 64, 64, 32, 40, 5, 1)),
    ("4096 pixels, dilation 2", (1, 63, 65, 64, 70, 3, 2), (1, 64, 66, 64, 70, 3, 2)),
    ("conv_k5 halo plane, 4 rows", (2, 4, 81, 32, 16, 5, 1), (1, 4, 82, 32, 16, 5, 1)),
    ("conv_k5 halo plane, 1 row", (1, 1, 132, 16, 16, 5, 1), (1, 1, 133, 16, 16, 5, 1)),
    ("conv_k5 pixel limit", (1, 12, 32, 16, 16, 5, 1), (1, 20, 20, 16, 16, 5, 1)),
    ("conv_ws, W % 2", (1, 3, 4, 48, 96, 3, 1), (1, 3, 5, 48, 96, 3, 1)),
]


def case_id(case):
    return "x".join(str(v) for v in case)


def seed(*key):
    """per-case seed that does not depend on PYTHONHASHSEED"""
    return zlib.crc32(repr(key).encode())


_problems = {}


def problem(case):
    """The case's inputs and float64 judgement, made once: x (post-ReLU-like, the images scaled by IMAGE_SCALES), He-scaled
    weights, a per-cout pre_a in [0.5, 1.5] and pre_b in [-0.3, 0.3], and with ReLU on
        want      the float64 convolution of the same float32 inputs,
        first(T)  (T|x| conv |w|) |pre_a| + |pre_b|, T|x| the maximum of |x| over +-T columns at the layer's dilation,
        second    2^-36 max|x| (1 conv |w|) |pre_a| per image.
    Nothing here is to be written to."""
    if case in _problems:
        return _problems[case]
    n, h, w, cin, cout, k, dil = case
    rng = np.random.default_rng(seed(case))
    x = np.maximum(rng.standard_normal((n, h, w, cin)), 0).astype(np.float32)
    for i, s in enumerate(IMAGE_SCALES.get(case, ())):
        x[i] *= np.float32(s)
    wt = (rng.standard_normal((k, k, cin, cout)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32)
    pre_a = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    pre_b = rng.uniform(-0.3, 0.3, cout).astype(np.float32)
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
    wtt = torch.from_numpy(wt).double().permute(3, 2, 0, 1)
    a = torch.from_numpy(pre_a).double().view(1, -1, 1, 1)
    b = torch.from_numpy(pre_b).double().view(1, -1, 1, 1)
    pad = dil * (k // 2)

    def nhwc(t):
        return t.permute(0, 2, 3, 1).numpy()

    def first(window):
        xa = xt.abs()
        if window:
            xa = F.max_pool2d(F.pad(xa, (window * dil, window * dil)), kernel_size=(1, 2 * window + 1), stride=1, dilation=(1, dil))
        return nhwc(F.conv2d(xa, wtt.abs(), None, padding=pad, dilation=dil) * a.abs() + b.abs())

    want = nhwc(F.relu(F.conv2d(xt, wtt, None, padding=pad, dilation=dil) * a + b))
    ones = nhwc(F.conv2d(torch.ones_like(xt[:1]), wtt.abs(), None, padding=pad, dilation=dil) * a.abs())
    amax = np.abs(x).reshape(n, -1).max(axis=1).astype(np.float64).reshape(-1, 1, 1, 1)
    firsts = {}

    def first_cached(window):
        if window not in firsts:
            firsts[window] = first(window)
        return firsts[window]

    p = {"x": x, "w": wt, "pre_a": pre_a, "pre_b": pre_b, "want": want, "first": first_cached, "second": 2.0 ** -36 * amax * ones}
    for v in (x, wt, pre_a, pre_b, want, p["second"]):
        v.setflags(write=False)
    _problems[case] = p
    return p


def allowed(case, ran):
    """the stated bound, element by element, of the kernel row that ran (tests/layer_bounds.family)"""
    n, h, w, cin, cout, k, dil = case
    p = problem(case)
    const, window = family(ran, (cout, cin, k, k))
    return const * p["first"](window) + p["second"]
