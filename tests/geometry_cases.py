"""Shapes, boxes and quads for the image-geometry edge tests (tests/test_geometry_edges_cpu.py, tests/test_geometry_edges_gpu.py)
and the per-box oracle every warp test shares.  Plain data and small builders; every seed is fixed.

A resize case is (name, src_h, src_w, dst_h, dst_w, Hmax, Wmax, n, cval): n images of src_h x src_w resized to dst_h x dst_w
and padded bottom / right to Hmax x Wmax with cval.  A box case is (name, box (4, 2) float32, expect, branch); a quad case is
(name, src (4, 2), dst (4, 2), (crop_w, crop_h), image index, expect, branch).  ``expect`` is "ok", "zero" (a box without width
or height: the reference's ZeroDivisionError, status 1) or "singular" (the 8 x 8 system has a zero pivot, status 2); ``branch``
says which line of the kernels or of the host set-up the case is there for."""
import numpy as np

F32 = np.float32

# ---------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------
_RESIZE_SHAPES = [
    # name, src_h, src_w, dst_h, dst_w, Hmax, Wmax, n: what it is there for
    ("down_53x37", 53, 37, 31, 22, 31, 22, 1),          # non-integer downscale: taps skip source pixels
    ("down_64x96", 64, 96, 25, 90, 25, 90, 1),          # non-integer downscale, very different factors per axis
    ("half", 64, 96, 32, 48, 32, 48, 1),                # exact 2:1: coefficients 1024 / 1024, OpenCV's area path
    ("third_x", 40, 96, 40, 32, 40, 32, 1),             # 3:1 in x (the fraction is 0: one tap), 1:1 in y
    ("down_x_up_y", 20, 90, 50, 33, 50, 33, 1),         # down in x, up in y
    ("identity", 30, 45, 30, 45, 30, 45, 1),            # dst == src: every fraction 0
    ("row_1x40", 1, 40, 3, 80, 3, 80, 1),               # 1-pixel source axis: both vertical taps are row 0
    ("col_40x1", 40, 1, 80, 3, 80, 3, 1),               # both horizontal taps are column 0
    ("to_1x1", 7, 9, 1, 1, 1, 1, 1),                    # 1-pixel destination: the centre of the source
    ("from_1x1", 1, 1, 5, 6, 5, 6, 1),                  # 1 x 1 source: every tap is the one pixel
    ("w255", 20, 300, 13, 255, 13, 255, 1),             # one thread short of the 256-thread block
    ("w256", 20, 300, 13, 256, 13, 256, 1),             # exactly one block
    ("w257", 20, 300, 13, 257, 13, 257, 1),             # one pixel into the second block
    ("w250_pad260", 20, 300, 13, 250, 15, 260, 1),      # padding starts inside the first block and runs into the second
]
# n = 3, Hmax > dst_h, Wmax > dst_w: the batch stride of source and destination, and a cval that is neither 255 nor 0
_BATCH = ("batch3", 37, 53, 55, 80, 60, 90, 3)
_CVALS_U8 = (0, 7, 255)
_CVALS_F32 = (0.0, -1.5, 255.0)


def resize_cases_u8():
    return [s + (255,) for s in _RESIZE_SHAPES] + [(_BATCH[0] + f"_cval{c}",) + _BATCH[1:] + (c,) for c in _CVALS_U8]


def resize_cases_f32():
    """the same shapes; the padding value is a float (one of them negative and not an integer)"""
    return [s + (255.0,) for s in _RESIZE_SHAPES] + [(_BATCH[0] + f"_cval{c}",) + _BATCH[1:] + (c,) for c in _CVALS_F32]


def case_id(case):
    return case[0]


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name))


def resize_source_u8(case):
    name, sh, sw, _, _, _, _, n, _ = case
    return np.random.default_rng(_seed(name)).integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)


def resize_source_f32(case, channels):
    """both signs, magnitudes from 1 to 1e4 and no value on a coarse grid, so that every product and sum of the two passes
    rounds"""
    name, sh, sw, _, _, _, _, n, _ = case
    rng = np.random.default_rng(_seed(name) + channels)
    return (rng.standard_normal((n, sh, sw, channels)) * 10.0 ** rng.uniform(0, 4, (n, sh, sw, channels))).clip(-1e4, 1e4).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# warp: images, boxes, groups
# ---------------------------------------------------------------------------------------------------------------------
IMG_H, IMG_W = 48, 64
TARGETS = ((31, 200), (4, 8), (64, 64))  # (target_height, target_width): the recogniser's, and two non-default ones


def warp_images_u8():
    return np.random.default_rng(4864).integers(0, 256, (2, IMG_H, IMG_W, 3), dtype=np.uint8)


def warp_images_f32(channels):
    """the float twins: the same pages plus a fraction, so that the gray conversion and the blend round in float32"""
    frac = np.random.default_rng(4865).random((2, IMG_H, IMG_W, 3)).astype(F32)
    return np.ascontiguousarray((warp_images_u8().astype(F32) + frac)[..., :channels])


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], dtype=F32)


def _rotated(box, radians, centre):
    q = np.asarray(box, dtype=np.float64) - centre
    c, s = np.cos(radians), np.sin(radians)
    return (np.stack([q[:, 0] * c - q[:, 1] * s, q[:, 0] * s + q[:, 1] * c], axis=-1) + centre).astype(F32)


def box_cases():
    w, h = IMG_W, IMG_H
    return [
        # every tap outside: the border value 0 on all four taps, an all-zero crop
        ("outside", rect(-40, -30, -10, -20), "ok", "tap(): all four taps outside, left of and above the image"),
        # corners on the corner pixels: the last column / row is sampled with its neighbour outside at weight 0
        ("whole_image", rect(0, 0, w - 1, h - 1), "ok", "tap(): sx + 1 == W and sy + 1 == H at the far edge"),
        # one pixel outside on every side: X in (-32, 0) gives sx = -1 with an arithmetic shift, 0 with a division
        ("one_px_larger", rect(-1, -1, w, h), "ok", "X >> 5 and X & 31 for X in (-32, 0); a tap at W and at H"),
        ("three_times", rect(-w, -h, 2 * w, 2 * h), "ok", "a box larger than the image: scale < 1, most taps outside"),
        ("negative_fraction", rect(-3.25, -2.5, 20.75, 9.5), "ok", "X >> 5, X & 31 on negative fractional coordinates"),
        ("negative_rotated", _rotated(rect(-6.5, -4.25, 30.5, 7.75), 0.3, (2.0, 3.0)), "ok",
         "negative X and Y with both fractions non-zero"),
        ("across_bottom_edge", rect(20, 40, 60, 52), "ok", "tap(): rows 47 <= y < 48 blend the last row with the border below it"),
        ("one_pixel", rect(10, 10, 11, 11), "ok", "w == h == 1: scale 31, a 31 x 31 crop of one pixel's neighbourhood"),
        ("sliver_2x40", rect(5, 20, 45, 22), "ok", "h = 2: scale by the width, a crop 10 rows high"),
        ("tall_40x3", rect(30, 4, 33, 44), "ok", "scale decided by the height (sh < sw)"),
        ("width_200", rect(5, 5, 55, 10), "ok", "scale * w == 200 exactly: cw == target_width, no column left empty"),
        ("width_199_rounding", rect(-20, 10, 77, 14), "ok", "(200 / 97) * 97 < 200 in float64: cw == 199 by truncation"),
        ("width_199_height", rect(2, 30, 60, 39), "ok", "31 / 9 * 58 = 199.8: cw == 199, scale by the height"),
        # min_rotated_rect returns false (fewer than 3 distinct points / a hull without area): the raw points are ordered
        ("two_points_twice", np.array([[5, 5], [5, 5], [20, 9], [20, 9]], F32), "zero",
         "rotated_box fallback, duplicate corners: w = 15, h = 0 -> status 1"),
        ("two_points_interleaved", np.array([[5, 5], [20, 9], [5, 5], [20, 9]], F32), "zero",
         "rotated_box fallback, stable sort of equal x: w = 15, h = 0 -> status 1"),
        ("collinear_close_pairs", np.array([[5, 5], [5.5, 5.25], [25, 15], [25.5, 15.25]], F32), "zero",
         "rotated_box fallback, collinear: w = 22, h = int(0.56) = 0 -> status 1"),
        ("collinear_diagonal", np.array([[3, 3], [10, 10], [20, 20], [40, 40]], F32), "singular",
         "rotated_box fallback, collinear and far apart: w, h > 0, zero pivot in solve8 -> status 2"),
        # collinear, but round-off keeps every pivot non-zero: the matrix has a zero row, invert3 returns zeros, W0 == 0 at every
        # pixel and the whole crop is source pixel (0, 0)
        ("collinear_zero_inverse", np.array([[4, 4], [8, 6], [20, 12], [30, 17]], F32), "ok",
         "rotated_box fallback; det == 0 in invert3 -> W0 == 0 everywhere -> tap (0, 0)"),
    ]


# the crop sizes the named cases are there for, (target_height, target_width) = (31, 200): a later edit of a box must keep them
EXPECTED_DSIZE = {"width_200": (200, 20), "width_199_rounding": (199, 8), "width_199_height": (199, 31), "one_pixel": (31, 31),
                  "sliver_2x40": (200, 10), "tall_40x3": (2, 31)}


def ok_boxes():
    return [(name, box) for name, box, expect, _ in box_cases() if expect == "ok"]


def box_named(name):
    return next(box for n, box, _, _ in box_cases() if n == name)


def group_layouts():
    """(name, [boxes of image 0, boxes of image 1], failing): the per-image counts and the image index of every crop"""
    b = dict(ok_boxes())
    zero = box_named("two_points_twice")
    empty = np.zeros((0, 4, 2), F32)
    return [
        ("3_0", [np.stack([b["whole_image"], b["negative_rotated"], b["one_pixel"]]), empty], False),
        ("0_2", [empty, np.stack([b["one_px_larger"], b["tall_40x3"]])], False),
        ("2+zero_2", [np.stack([b["whole_image"], zero, b["negative_fraction"]]), np.stack([b["sliver_2x40"], b["three_times"]])], True),
    ]


def split_boxes(count=65540, distinct=20):
    """``count`` boxes cycling through ``distinct`` non-degenerate ones inside and around the 48 x 64 image: more crops than
    one grid's y dimension (65 535) holds, so launch_warp / launch_warp_f32 take a second launch"""
    rng = np.random.default_rng(65535)
    base = []
    for k in range(distinct):
        cx, cy = rng.uniform(8, IMG_W - 8), rng.uniform(8, IMG_H - 8)
        bw, bh = rng.uniform(6, 30), rng.uniform(3, 12)
        base.append(_rotated(rect(cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2), rng.uniform(-0.5, 0.5), (cx, cy)))
    base = np.stack(base)
    return base, base[np.arange(count) % distinct]


# ---------------------------------------------------------------------------------------------------------------------
# warp_quads: perspective source quads (no parallelograms), all with target (16, 32)
# ---------------------------------------------------------------------------------------------------------------------
QUAD_TARGET = (16, 32)  # (target_height, target_width)
_QDST = rect(0, 0, 32, 16)


def quad_cases():
    return [
        ("trapezoid_4to1", np.array([[10, 10], [50, 10], [35, 40], [25, 40]], F32), _QDST, (32, 16), 0, "ok",
         "a top edge four times the bottom edge: W0 varies by a factor of four over the crop"),
        # the inverse map is exactly [[2, 0, -8], [0, 2, -16], [1, 0, -3]] (every step of the LU and of the adjugate is exact on
        # these integers): W0 = x - 3 is negative left of crop column 3, zero ON it and positive to its right
        ("denominator_changes_sign", np.array([[3, 8], [4, 16], [4, 8], [3, 4]], F32), np.array([[1, 0], [2, 0], [2, 4], [1, 4]], F32),
         (32, 16), 1, "ok", "W0 == 0.0 exactly at x == 3 (Wi = 0 -> source pixel (0, 0)); W0 < 0 left of it"),
        # crop pixel (0, 0) maps to image pixel (10, 10); every other one lands beyond +-2^31 / 32 pixels
        ("beyond_int32", np.array([[10, 10], [8e12, -7e12], [6e12, 6e12], [-9e12, 5e12]], F32), _QDST, (32, 16), 0, "ok",
         "fmax(-2^31, fmin(2^31 - 1, .)) before rint, on both sides"),
        ("collinear_source", np.array([[3, 3], [10, 10], [20, 20], [40, 40]], F32), _QDST, (32, 16), 1, "singular",
         "quad_homography returns false -> status 2, the slot's matrices are zeroed"),
    ]


# ---------------------------------------------------------------------------------------------------------------------
# the per-box oracle of the warp tests (tests/test_warp_gpu.py, tests/test_float_gpu.py and the edge tests)
# ---------------------------------------------------------------------------------------------------------------------
def oracle_crops(images, box_groups, target_height=31, target_width=200):
    """Recognizer.recognize_from_boxes' crop loop on uint8 pages: gray, warpBox per box, / 255 in float32"""
    from oracle import tools as otools

    crops = []
    for im, boxes in zip(images, box_groups):
        gray = otools.rgb2gray_u8(im)
        for box in boxes:
            crops.append(otools.warp_box(gray, box, target_height, target_width))
    return np.array(crops, dtype="float32") / 255 if crops else np.zeros((0, target_height, target_width), np.float32)


def oracle_crops_f32(images, box_groups, target_height=31, target_width=200):
    """the same loop on float pages (H, W, 3 or 1): float gray, float warp, no division"""
    from oracle import tools as otools

    crops = []
    for im, boxes in zip(images, box_groups):
        gray = otools.rgb2gray_float(im) if im.shape[-1] == 3 else np.asarray(im[..., 0], np.float32)
        for box in boxes:
            crops.append(otools.warp_box_float(gray, box, target_height, target_width))
    return np.stack(crops) if crops else np.zeros((0, target_height, target_width), np.float32)


def oracle_quad_crop(gray, src, dst, crop_wh, target_height, target_width):
    """one crop of kocr_warp_quads on a gray uint8 page -> (crop float32 / 255, forward matrix)"""
    from oracle import tools as otools

    M = otools.get_perspective_transform(src, dst)
    out = np.zeros((target_height, target_width), np.uint8)
    cw, ch = min(crop_wh[0], target_width), min(crop_wh[1], target_height)
    out[:ch, :cw] = otools.warp_perspective_u8(gray, M, (cw, ch))
    return out.astype(np.float32) / 255, M
