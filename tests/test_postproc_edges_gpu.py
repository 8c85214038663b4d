"""The heat-map -> boxes kernels (csrc/postproc.hip, K1 - K12 and the empty-contour error path) at their edges: every case of
tests/postproc_cases.py through kocr_get_boxes against the CPU oracle, which tests/test_postproc_edges_cpu.py anchors at the
same cases by hand.

Bar: identical counts and order and bit-identical float32 corners under both min-area-rectangle rules (integer and
fixed-order float work, -ffp-contract=off); detection scores bit for bit, a NaN as a NaN.  Each case's reference is computed
once (postproc_cases.oracle / .statements) and shared by the tests."""
import functools

import numpy as np
import pytest

from tests import postproc_cases as pc
from tests.test_postproc_gpu import _check

pytestmark = pytest.mark.gpu

BOXES = pc.names("boxes")
ERRORS = pc.names("index_error")
MULTI = pc.names("boxes", multi_image=True)


def _check_bits(got, want, what=""):
    """_check, then the corners on their uint32 views: -0.0 is not +0.0 and a NaN is equal to itself only here"""
    _check(got, want)
    for i, (g, w_) in enumerate(zip(got, want)):
        if len(w_):
            gb, wb = np.ascontiguousarray(g, np.float32).view(np.uint32), np.ascontiguousarray(w_, np.float32).view(np.uint32)
            assert np.array_equal(gb, wb), f"{what} image {i}: {int((gb != wb).any(axis=(1, 2)).sum())} of {len(w_)} boxes differ in bits"


def _same_scores(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g.dtype == np.float32 and g.shape == w_.shape, f"{what} image {i}: {g.shape} scores, the statement has {w_.shape}"
        nan = np.isnan(w_)
        assert np.array_equal(np.isnan(g), nan), f"{what} image {i}: NaN scores {np.isnan(g)}, the statement {nan}"
        assert np.array_equal(g[~nan].view(np.uint32), w_[~nan].view(np.uint32)), f"{what} image {i}: {g} != {w_}"


@functools.lru_cache(maxsize=None)
def _valid(name):
    """an index_error case with the link map under its threshold, and the oracle's boxes for it"""
    from oracle import postproc

    c = pc.case(name)
    y = pc.without_link(c["heat"])
    return y, postproc.get_boxes(y, **c["kwargs"])


@pytest.mark.parametrize("name", BOXES)
def test_boxes_default_rule(ctx, name):
    c = pc.case(name)
    want = pc.oracle(name)[0]
    got = ctx.get_boxes(c["heat"], **c["kwargs"])
    assert [len(b) for b in got] == c["counts"], (name, c["aims"])
    _check_bits(got, want, name)


@pytest.mark.parametrize("name", BOXES)
def test_boxes_opencv_rule(ctx, name):
    c = pc.case(name)
    _, want, _ = pc.statements(name)
    got = ctx.get_boxes(c["heat"], min_area_rect="opencv", **c["kwargs"])
    assert [len(b) for b in got] == c["counts"], (name, c["aims"])
    _check_bits(got, want, name)


@pytest.mark.parametrize("name", BOXES)
def test_scores(ctx, name):
    """the score is the tmax comp_kept compared: kept / dropped and the number reported must agree with np.max and <"""
    from tests import scores_statement as ss

    c = pc.case(name)
    kw = {k: v for k, v in c["kwargs"].items() if k in ("text_threshold", "link_threshold")}
    want = ss.detection_scores(c["heat"], pc.oracle(name)[1], **kw)
    boxes, scores = ctx.get_boxes(c["heat"], return_scores=True, **c["kwargs"])
    _check_bits(boxes, pc.oracle(name)[0], name)
    _same_scores(scores, want, name)


@pytest.mark.parametrize("name,true_max", [("pixel_grid", 9216), ("square_grid", 400)])
def test_capacity_retries(ctx, name, true_max):
    """the binding's default cap, a cap far too small (one retry with the true maximum) and an exactly full buffer"""
    c = pc.case(name)
    want = pc.oracle(name)[0]
    assert max(len(b) for b in want) == true_max
    for cap in (None, 7, true_max):
        _check_bits(ctx.get_boxes(c["heat"], cap=cap, **c["kwargs"]), want, f"{name} cap={cap}")


def test_dense_roots_keep_raster_order(ctx):
    """k_assign: 32 kept roots per ballot.  A rank that is wrong inside a ballot shows here as an order violation instead of
    9216 mismatching boxes"""
    c = pc.case("pixel_grid")
    got = ctx.get_boxes(c["heat"], **c["kwargs"])[0]
    assert got.shape == (9216, 4, 2)
    key = got[:, 0, 1].astype(np.int64) * 4096 + got[:, 0, 0].astype(np.int64)  # (y, x) of the first corner
    bad = np.flatnonzero(np.diff(key) <= 0)
    assert not len(bad), f"{len(bad)} boxes are not after their predecessor in (y, x) order, the first at slot {bad[0] + 1}"


@pytest.mark.parametrize("name", MULTI)
def test_image_by_image_equals_the_batch(ctx, name):
    c = pc.case(name)
    batch = ctx.get_boxes(c["heat"], **c["kwargs"])
    _check_bits(batch, pc.oracle(name)[0], name)
    for i in range(len(c["heat"])):
        alone = ctx.get_boxes(c["heat"][i:i + 1], **c["kwargs"])
        _check_bits(alone, batch[i:i + 1], f"{name} image {i} alone")


@pytest.mark.parametrize("name", ERRORS)
def test_index_error_from_the_context(ctx, name):
    """IndexError as the reference at detection.py:272; with cap=1 the capacity growth comes first, then the error.  The
    failed call's buffers are undefined: nothing is asserted about them"""
    c = pc.case(name)
    y, want = _valid(name)
    for cap in (None, 1):
        with pytest.raises(IndexError):
            ctx.get_boxes(c["heat"], cap=cap, **c["kwargs"])
        _check_bits(ctx.get_boxes(y, cap=cap, **c["kwargs"]), want, f"{name} after the failure, cap={cap}")
    with pytest.raises(IndexError):
        ctx.get_boxes(c["heat"], min_area_rect="opencv", **c["kwargs"])
    _check_bits(ctx.get_boxes(y, **c["kwargs"]), want, f"{name} after the failure under the OpenCV rule")


@pytest.mark.parametrize("on_device", [0, 1])
@pytest.mark.parametrize("name", ERRORS)
def test_index_error_from_the_entry_point(ctx, name, on_device):
    """kocr_get_boxes itself returns KOCR_EEMPTYCONTOUR (-6), for a host buffer and for device pointers"""
    from tests.test_device_pointers_gpu import _Abi, _dev, _host

    c = pc.case(name)
    kw = dict(detection_threshold=0.7, text_threshold=0.4, link_threshold=0.4, size_threshold=10)
    kw.update(c["kwargs"])
    thr = (kw["detection_threshold"], kw["text_threshold"], kw["link_threshold"], kw["size_threshold"])
    abi = _Abi(ctx)
    n, h, w, _ = c["heat"].shape
    cap = 16
    y, want = _valid(name)

    def call(heat):
        boxes, counts = np.zeros((n, cap, 4, 2), np.float32), np.zeros(n, np.int32)
        heat = np.array(heat)  # the cases are read-only
        d_heat, d_boxes = (_dev(heat), _dev(boxes)) if on_device else (heat, boxes)
        rc = abi("kocr_get_boxes", d_heat, n, h, w, *thr, d_boxes, counts, cap, on_device)
        return rc, (_host(d_boxes) if on_device else boxes), counts

    assert call(c["heat"])[0] == -6
    rc, boxes, counts = call(y)
    assert rc == 0 and counts.tolist() == [len(b) for b in want]
    _check_bits([boxes[i, :counts[i]] if counts[i] else np.array([]) for i in range(n)], want, f"{name} after the failure")


@pytest.mark.parametrize("name", ERRORS)
def test_index_error_from_getboxes(name):
    from keras_ocr_amd import detection

    c = pc.case(name)
    y, want = _valid(name)
    with pytest.raises(IndexError):
        detection.getBoxes(c["heat"], **c["kwargs"])
    _check_bits(detection.getBoxes(y, **c["kwargs"]), want, f"{name} after the failure")
