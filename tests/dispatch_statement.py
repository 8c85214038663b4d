"""A plain statement of the convolution dispatcher: which kernel arrangement a layer reaches, as the profiler row that
kocr_conv2d_nhwc must show.  Written from DESIGN.md section 3 and the predicates of launch_conv_pool, plan_w43,
w43_ragged_geo and the *_applicable functions; it imports nothing from the library and every comparison is made in
integers (the padding shares cross-multiplied), so it cannot drift with float rounding.

The order of the questions is the dispatcher's: conv_k5, the F(4,3) family, F(2,3) conv_ws, conv_ds, conv_hs*, and
the fp32 MFMA kernel for what is left.  The input is a dense NHWC tensor as kocr_conv2d_nhwc stages it (channel stride
= Cin, 16-byte aligned), all developer switches (KOCR_*) at their defaults.

    mode   0 = KOCR_SPLIT_BF16X3, 1 = KOCR_SPLIT_F16X2 (the default), 2 = KOCR_SPLIT_F16X1   (ctx.get_split_mode())
    pool   the layer is launched with a fused-or-not 2 x 2 max-pool destination (the detector's slice1.3, 1.10, 3.20,
           4.30); kocr_conv2d_nhwc never pools.  The row returned is the convolution's; an unfused pooling adds its own.

Thresholds stated here (each has a pair of cases in tests/dispatch_cases.py):
    conv_k5        5 x 5, 16 couts, H W <= 384 and (H + 4)(W + 4) <= 680 (the LDS halo plane), no pooling
    F(4,3)         3 x 3, Cin % 32 == 0, Cout > 32 (dilated: Cout > 64), N H W < 2^29, and a width some arrangement takes:
                   W % (4 dil) == 0, or a ragged grid (fp16 modes, dilation 1)
    ragged grid    fp16 modes, dilation 1: 4 x 64 tiles, or 8 x 32 where they cover the image with more than 2 % less
                   area (wide layers without pooling only); always when W % 4 != 0, else only for images of >= 256 pixels
                   whose padded grid is at most 1.25 of the image
    fp16 flattened images of >= 256 pixels (a 256-pixel tile must not span three images), no fused pooling
    conv_ws        3 x 3, dilation 1, Cin % 16 == 0, Cout > 32, W % 2 == 0
    conv_ds        Cin % 16 == 0, Cout > 32, not a plain 3 x 3, N H W >= 4096
    conv_hs*       3 x 3, dilation 1, Cout <= 32 (16-wide product tile up to 16 couts), Cin % 16 == 0, any size
"""

BF16X3, F16X2, F16X1 = 0, 1, 2

K5_MAXM = 384    # pixels conv_k5 takes per image
K5_MAXHP = 680   # halo pixels its LDS planes hold


def _ceil_to(a, b):
    return (a + b - 1) // b * b


def _small(h, w, cin):
    """the reuse arrangements address one image with 32-bit byte offsets"""
    return h * w * cin * 4 < 2 ** 31


def ragged_geo(h, w, cin, cout, dil, mode, pool=False):
    """The ragged tile grid of an image: 1 = 4 x 64 tiles, 2 = 8 x 32, -1 = none."""
    if mode == BF16X3 or dil != 1 or not _small(h, w, cin):
        return -1
    narrow = cout <= 64
    a1 = _ceil_to(h, 4) * _ceil_to(w, 64)   # pixels the 4 x 64 grid covers
    a2 = _ceil_to(h, 8) * _ceil_to(w, 32)   # ... the 8 x 32 grid
    # c1 <= 1.02 c2, both shares over the same H W.  (Exact equality, 50 a1 == 51 a2, needs a factor 17 in the 4 x 64
    # grid's tile counts: no shape tested has it, and there the library's double arithmetic decides.)
    geo = 1 if (narrow or pool or 100 * a1 <= 102 * a2) else 2
    a = a1 if geo == 1 else a2
    if w % 4 != 0:
        return geo          # no flattened arrangement takes this width
    if h * w < 256:
        return -1           # tiny images stay on the flattened bf16x3 tiles
    return geo if 4 * a <= 5 * h * w else -1   # padding share a / (H W) <= 1.25


def w43_row(n, h, w, cin, cout, dil, mode, pool=False):
    """The F(4,3) family's row for a 3 x 3 layer, or None where no arrangement takes it."""
    if cin % 32 != 0 or cout <= 32 or (cout <= 64 and dil != 1) or n * h * w >= 2 ** 29:
        return None
    fp16 = mode != BF16X3
    if w % (4 * dil) != 0 and ragged_geo(h, w, cin, cout, dil, mode, False) <= 0:
        return None
    rag = ragged_geo(h, w, cin, cout, dil, mode, pool)
    exact_fuse = pool and dil == 1 and h % 2 == 0 and w % 64 == 0
    reuse_ok = dil == 1 and (not pool or exact_fuse) and _small(h, w, cin)
    narrow = cout <= 64
    geo, ragged = 0, False
    if narrow:
        arr = "r"
        if reuse_ok and h % 4 == 0 and w % 64 == 0:
            geo = 1
        elif reuse_ok and h % 2 == 0 and w % 128 == 0:
            geo = 0
        elif rag == 1:
            geo, ragged = 1, True
        else:
            arr = "n"
    else:
        arr = "v"
        if reuse_ok and h % 4 == 0 and w % 64 == 0:
            geo = 1
        elif reuse_ok and not pool and h % 8 == 0 and w % 32 == 0:
            geo = 2
        elif rag > 0:
            geo, ragged = rag, True
        else:
            arr = "s"
    fuse = exact_fuse or (pool and ragged and geo == 1)
    pieces = 0
    if fp16:
        if arr == "s" and not fuse and h * w >= 256:
            arr = "f"
        if arr in ("v", "f") or (arr == "r" and geo == 1):
            pieces = 2 if (mode == F16X2 or ragged) else 1   # the ragged grids exist with two pieces only
    if arr == "v":
        letter = "t" if geo == 2 else "v"
    elif arr == "f" or (arr == "r" and pieces):
        letter = arr
    else:
        letter = "s"
    tile = {"r": "_256x64", "n": "_512x64"}.get(arr, "_256x128")
    name = "conv_w4" + {2: "h", 1: "q", 0: ""}[pieces] + letter + tile
    name += "_pool" if fuse else "_dil" if dil != 1 else ""
    return name + ("_rag" if ragged else "")


def row(n, h, w, cin, cout, k, dil, mode, pool=False):
    """The profiler row of a k x k convolution (dilation dil, 'same' padding) of an n x h x w x cin tensor to cout."""
    if k == 5 and dil == 1 and cout == 16 and cin % 16 == 0 and not pool and h * w <= K5_MAXM and (h + 4) * (w + 4) <= K5_MAXHP:
        return "conv_k5_352x16"
    if k == 3:
        r = w43_row(n, h, w, cin, cout, dil, mode, pool)
        if r is not None:
            return r
    if k == 3 and dil == 1 and cin % 16 == 0 and cout > 32 and w % 2 == 0:
        wide = cout > 64
        fuse = pool and h % 2 == 0 and w % (64 if wide else 128) == 0
        return ("conv_ws_128x128" if wide else "conv_ws_256x64") + ("_pool" if fuse else "")
    if cin % 16 == 0 and cout > 32 and not (k == 3 and dil == 1) and 4096 <= n * h * w and n * h * w * cin < 2 ** 40:
        return "conv_ds_256x128" if cout > 64 else "conv_ds_512x64"
    if k == 3 and dil == 1 and cout <= 32 and cin % 16 == 0 and _small(h, w, cin) and _small(h, w, 32):
        if cout <= 16:
            return "conv_hs_256x16"
        return "conv_hh_256x32" if mode != BF16X3 else "conv_hs_256x32"
    gather = 0 if cin % 16 == 0 else 1   # 16-channel vector loads, or the scalar gather
    bn = 128 if cout > 64 else 64 if cout > 32 else 32
    fuse = pool and gather == 0 and bn >= 64 and h % 2 == 0 and w % 64 == 0
    return f"conv_mfma_128x{bn}_m{gather}" + ("_pool" if fuse else "")
