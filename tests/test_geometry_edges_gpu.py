"""The image-geometry kernels (csrc/imgproc.hip: resize_pad_kernel, resize_pad_f32_kernel and their host-built tap tables;
csrc/warp.hip: warp_kernel, warp_f32_kernel, warp_quads_kernel and the host set-up of kocr_warp_crops) at the edge shapes of
tests/geometry_cases.py, against the oracle (oracle/tools.py), which tests/test_geometry_edges_cpu.py anchors at these shapes.

Every comparison is bit for bit -- np.array_equal, on float results of their uint32 views: the kernels are integer work, or
float work in a fixed order built with -ffp-contract=off."""
import numpy as np
import pytest

from tests import geometry_cases as gc
from tests.test_device_pointers_gpu import _Abi

pytestmark = pytest.mark.gpu

KOCR_EINVAL, KOCR_EZERODIV = -1, -7


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32 and b.dtype == np.float32:
        return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return a.dtype == b.dtype and np.array_equal(a, b)


def _where(a, b):
    """the first differing index and the two values, for a failure message"""
    bad = np.argwhere(np.ascontiguousarray(a) != np.ascontiguousarray(b))
    return (len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]) if len(bad) else "bits only (signed zero / NaN)"


# ---------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------
def _check_resize(got, src, resize, case):
    from oracle import tools as ot

    name, _, _, dh, dw, hmax, wmax, n, cval = case
    assert got.shape == (n, hmax, wmax, src.shape[-1]) and got.dtype == src.dtype
    for k in range(n):
        want = resize(src[k], (dw, dh))
        assert _same(got[k, :dh, :dw], want), (name, "image", k, _where(got[k, :dh, :dw], want))
        below, right = got[k, dh:], got[k, :dh, dw:]
        assert (below == src.dtype.type(cval)).all(), (name, "padding below, image", k)
        assert (right == src.dtype.type(cval)).all(), (name, "padding to the right, image", k)
        assert _same(got[k], ot.pad(want, wmax, hmax, cval=cval).astype(src.dtype)), (name, "whole canvas, image", k)


@pytest.mark.parametrize("case", gc.resize_cases_u8(), ids=gc.case_id)
def test_resize_pad_equals_the_oracle(ctx, case):
    from oracle import tools as ot

    src = gc.resize_source_u8(case)
    got = ctx.resize_pad(src, (case[4], case[3]), out_hw=(case[5], case[6]), cval=case[8])
    _check_resize(got, src, ot.cv_resize_linear_u8, case)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("case", gc.resize_cases_f32(), ids=gc.case_id)
def test_resize_pad_f32_equals_the_oracle(ctx, case, channels):
    from oracle import tools as ot

    src = gc.resize_source_f32(case, channels)
    got = ctx.resize_pad_f32(src, (case[4], case[3]), out_hw=(case[5], case[6]), cval=case[8])
    _check_resize(got, src, ot.resize_linear_float, case)


@pytest.mark.parametrize("max_scale,max_size", [(2, 64), (0.7, 2048)], ids=["max_size_cap", "max_scale_below_1"])
def test_resize_image_downscales(ctx, max_scale, max_size):
    """tools.resize_image with a scale below 1: through the max_size cap (60 x 90 page, max_size 64) and through max_scale"""
    import keras_ocr_amd
    from oracle import tools as ot

    page = np.random.default_rng(6090).integers(0, 256, (60, 90, 3), dtype=np.uint8)
    got, scale = keras_ocr_amd.tools.resize_image(page, max_scale=max_scale, max_size=max_size, ctx=ctx)
    want, wscale = ot.resize_image(page, max_scale, max_size)
    assert scale == wscale < 1 and _same(got, want), (scale, wscale, got.shape, want.shape)
    fpage = gc.resize_source_f32(("page", 60, 90, 0, 0, 0, 0, 1, 0), 3)[0]
    got, scale = keras_ocr_amd.tools.resize_image(fpage, max_scale=max_scale, max_size=max_size, ctx=ctx)
    want = ot.resize_linear_float(fpage, (int(90 * wscale), int(60 * wscale)))
    assert scale == wscale and got.dtype == np.float32 and _same(got, want), (scale, got.shape, want.shape)


# ---------------------------------------------------------------------------------------------------------------------
# warp_crops / warp_crops_f32
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pages():
    return gc.warp_images_u8()


def _warp(ctx, kind, pages, groups, th, tw):
    """(got, want) of one call: kind "u8", "f32c3" or "f32c1" """
    if kind == "u8":
        return ctx.warp_crops(pages, groups, th, tw), gc.oracle_crops(pages, groups, th, tw)
    fp = gc.warp_images_f32(3 if kind == "f32c3" else 1)
    if len(pages) == 1:
        fp = fp[:1]
    return ctx.warp_crops_f32(fp, groups, th, tw), gc.oracle_crops_f32(fp, groups, th, tw)


KINDS = ["u8", "f32c3", "f32c1"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("target", gc.TARGETS, ids=lambda t: f"{t[0]}x{t[1]}")
def test_box_crops_equal_the_oracle(ctx, pages, target, kind):
    """every non-degenerate box case, on both pages in one call (image 0 takes the boxes in order, image 1 in reverse)"""
    names = [n for n, _ in gc.ok_boxes()]
    boxes = np.stack([b for _, b in gc.ok_boxes()])
    got, want = _warp(ctx, kind, pages, [boxes, boxes[::-1]], *target)
    assert got.shape == want.shape == (2 * len(boxes),) + target
    for i, name in enumerate(names + names[::-1]):
        assert _same(got[i], want[i]), (name, "image", i // len(names), _where(got[i], want[i]))
    k = names.index("outside")
    assert not got[k].any() and not got[2 * len(names) - 1 - k].any()


@pytest.mark.parametrize("kind", KINDS)
def test_degenerate_boxes_raise_what_the_reference_raises(ctx, pages, kind):
    import keras_ocr_amd

    for name, box, expect, _ in gc.box_cases():
        if expect == "zero":       # tools.py:95 divides by int(w) or int(h) == 0
            with pytest.raises(ZeroDivisionError):
                _warp(ctx, kind, pages[:1], [box[None]], 31, 200)
        elif expect == "singular":  # status 2: the library's own error (cv2.getPerspectiveTransform's behaviour is not pinned)
            with pytest.raises(keras_ocr_amd.KocrError, match="singular perspective transform"):
                _warp(ctx, kind, pages[:1], [box[None]], 31, 200)


@pytest.mark.parametrize("kind", KINDS)
def test_group_layouts(ctx, pages, kind):
    """the per-image counts and the image index of every crop: [3, 0], [0, 2], and a zero-size box among valid ones"""
    for name, groups, failing in gc.group_layouts():
        if not failing:
            got, want = _warp(ctx, kind, pages, groups, 31, 200)
            assert len(got) == sum(len(g) for g in groups) and _same(got, want), (name, _where(got, want))
            continue
        with pytest.raises(ZeroDivisionError):
            _warp(ctx, kind, pages, groups, 31, 200)
        # the same context, the valid boxes alone: the failed call left nothing behind
        valid = [np.stack([b for b in g if not np.array_equal(b, gc.box_named("two_points_twice"))]) for g in groups]
        assert [len(v) for v in valid] == [2, 2]
        got, want = _warp(ctx, kind, pages, valid, 31, 200)
        assert _same(got, want), (name, _where(got, want))


def test_zero_size_box_through_the_raw_entry_points(ctx, pages):
    """"any non-zero return | the contents of that call's output buffers are undefined (partial
    results may have been written)" -- so what the raw calls owe for a zero-size box among valid ones is the code,
    KOCR_EZERODIV ("ZeroDivisionError at tools.py:95"), for the uint8 and the float entry point, and a context that still
    works: the next call with the valid boxes is bit-exact."""
    abi = _Abi(ctx)
    _, groups, _ = next(g for g in gc.group_layouts() if g[2])
    counts = np.array([len(g) for g in groups], np.int32)
    flat = np.ascontiguousarray(np.concatenate(groups), dtype=np.float32)
    n, h, w, _ = pages.shape
    out = np.zeros((len(flat), 31, 200), np.float32)
    assert abi("kocr_warp_crops", pages, n, h, w, flat, counts, 31, 200, out, 0) == KOCR_EZERODIV
    fp = gc.warp_images_f32(3)
    assert abi("kocr_warp_crops_f32", fp, n, h, w, 3, flat, counts, 31, 200, out) == KOCR_EZERODIV
    keep = [i for i in range(len(flat)) if not np.array_equal(flat[i], gc.box_named("two_points_twice"))]
    counts2, flat2 = np.array([2, 2], np.int32), np.ascontiguousarray(flat[keep])
    out2 = np.zeros((4, 31, 200), np.float32)
    assert abi("kocr_warp_crops", pages, n, h, w, flat2, counts2, 31, 200, out2, 0) == 0
    assert _same(out2, gc.oracle_crops(pages, [flat2[:2], flat2[2:]]))


@pytest.mark.parametrize("kind", KINDS)
def test_swapping_the_images_swaps_the_crops(ctx, pages, kind):
    """no oracle: the same boxes on pages (A, B) and on (B, A), with unequal counts, must give the same crops in swapped order"""
    b = np.stack([box for name, box in gc.ok_boxes() if name in ("whole_image", "negative_rotated", "across_bottom_edge")])
    fp = gc.warp_images_f32(3 if kind == "f32c3" else 1)
    call = (lambda im, g: ctx.warp_crops(im, g, 31, 200)) if kind == "u8" else (lambda im, g: ctx.warp_crops_f32(im, g, 31, 200))
    im = pages if kind == "u8" else fp
    ab = call(im, [b, b[:2]])          # A: 3 crops, B: 2
    ba = call(im[::-1], [b[:2], b])    # B: 2 crops, A: 3
    assert _same(ba, np.concatenate([ab[3:], ab[:3]]))
    assert not _same(ab[:2], ab[3:])   # the two pages do differ


# ---------------------------------------------------------------------------------------------------------------------
# warp_quads
# ---------------------------------------------------------------------------------------------------------------------
def _quad_call(ctx, pages, cases):
    th, tw = gc.QUAD_TARGET
    return ctx.warp_quads(pages, [c[1] for c in cases], [c[2] for c in cases], [c[4] for c in cases], [c[3] for c in cases], th, tw,
                          return_transforms=True)


def test_perspective_quads_equal_the_oracle(ctx, pages):
    """kocr_warp_quads takes uint8 pages only (the float kernel is reached through kocr_warp_crops_f32 above)"""
    import keras_ocr_amd
    from oracle import tools as ot

    th, tw = gc.QUAD_TARGET
    good = [c for c in gc.quad_cases() if c[5] == "ok"]
    got, tf = _quad_call(ctx, pages, good)
    for i, (name, src, dst, wh, img, _, _) in enumerate(good):
        want, M = gc.oracle_quad_crop(ot.rgb2gray_u8(pages[img]), src, dst, wh, th, tw)
        assert _same(got[i], want), (name, _where(got[i], want))
        assert np.array_equal(tf[i].view(np.uint64), M.view(np.uint64)), (name, tf[i], M)   # the same float64 operation order
    # the singular quad: the documented error (status 2 -> KOCR_EINVAL "singular perspective transform") ...
    with pytest.raises(keras_ocr_amd.KocrError, match="singular perspective transform"):
        _quad_call(ctx, pages, gc.quad_cases())
    abi = _Abi(ctx)
    cases = gc.quad_cases()
    m, (n, h, w, _) = len(cases), pages.shape
    src, dst = (np.ascontiguousarray(np.stack([c[k] for c in cases]), dtype=np.float32) for k in (1, 2))
    idx = np.array([c[4] for c in cases], np.int32)
    cw, ch = (np.array([c[3][k] for c in cases], np.int32) for k in (0, 1))
    out, tfs = np.zeros((m, th, tw), np.float32), np.zeros((m, 3, 3), np.float64)
    assert abi("kocr_warp_quads", pages, n, h, w, m, src, dst, idx, cw, ch, th, tw, out, tfs) == KOCR_EINVAL
    # ... and, the output of a failed call being undefined, what "does not disturb the other quads"
    # can hold is the next call on the same context: the good quads again, bit-exact
    again, tf2 = _quad_call(ctx, pages, good)
    assert _same(again, got) and np.array_equal(tf2.view(np.uint64), tf.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------------
# more crops than one grid holds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["u8", "f32c3"])
def test_more_crops_than_one_launch_holds(ctx, pages, kind):
    """65 540 boxes on one page: launch_warp / launch_warp_f32 split the crops into launches of 65 535 (grid.y's limit); the
    second launch's parameter and output offsets are only reachable past that count"""
    th, tw = 4, 8
    base, boxes = gc.split_boxes()
    assert len(boxes) == 65540 > 65535 and len(base) == 20
    if kind == "u8":
        got, want20 = ctx.warp_crops(pages[:1], [boxes], th, tw), gc.oracle_crops(pages[:1], [base], th, tw)
    else:
        fp = gc.warp_images_f32(3)[:1]
        got, want20 = ctx.warp_crops_f32(fp, [boxes], th, tw), gc.oracle_crops_f32(fp, [base], th, tw)
    assert len({c.tobytes() for c in want20}) == 20     # the 20 oracle crops are distinct: a shifted crop cannot pass
    want = np.tile(want20, (len(boxes) // 20, 1, 1))
    assert got.shape == want.shape == (65540, th, tw)
    named = {i: _same(got[i], want[i]) for i in (65534, 65535, 65536, 65539)}
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=(1, 2)))[0]
    assert _same(got, want), (f"crops equal the oracle at {named}; {len(bad)} crops differ, first {bad[:5]}, last {bad[-5:]}")
