"""Anchors oracle/postproc.py at the edge cases of tests/postproc_cases.py by what can be derived by hand, independently of the
oracle's own code path: tests/test_postproc_edges_gpu.py then holds the kernels to the oracle at the same cases.  A GPU test
that compares two restatements sharing a misreading proves little; this file is where the misreading would show."""
import numpy as np
import pytest

from tests import postproc_cases as pc

BOXES = pc.names("boxes")
ERRORS = pc.names("index_error")


def _label_by_scan(fg):
    """4-connected components numbered by the raster position of their first pixel: a flood fill started from every still
    unlabelled pixel of np.argwhere's raster scan (no scipy)"""
    h, w = fg.shape
    lab = np.zeros((h, w), np.int64)
    n = 0
    for y, x in np.argwhere(fg):
        if lab[y, x]:
            continue
        n += 1
        lab[y, x] = n
        stack = [(int(y), int(x))]
        while stack:
            cy, cx = stack.pop()
            for ny, nx in ((cy - 1, cx), (cy + 1, cx), (cy, cx - 1), (cy, cx + 1)):
                if 0 <= ny < h and 0 <= nx < w and fg[ny, nx] and not lab[ny, nx]:
                    lab[ny, nx] = n
                    stack.append((ny, nx))
    return lab, n


def _kept_by_scan(y, detection_threshold=0.7, text_threshold=0.4, link_threshold=0.4, size_threshold=10):
    """[(label, area, x, y, w, h, max text)] of the components detection.py:233-241 keeps, in label order"""
    text, link = y[..., 0], y[..., 1]
    lab, n = _label_by_scan((text > np.float32(text_threshold)) | (link > np.float32(link_threshold)))
    order = np.argsort(lab, axis=None, kind="stable")
    order = order[lab.ravel()[order] > 0]
    groups = np.split(order, np.cumsum(np.bincount(lab.ravel()[order])[1:])[:-1]) if n else []
    kept = []
    for k, idx in enumerate(groups, 1):
        ys, xs = np.unravel_index(idx, lab.shape)
        tmax = text.ravel()[idx].max()
        if len(idx) < size_threshold or tmax < np.float32(detection_threshold):
            continue
        kept.append((k, len(idx), int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1), tmax))
    return kept


@pytest.mark.parametrize("name", BOXES)
def test_counts_labels_niter_and_roi(name):
    """the i-th box belongs to the kept component whose raster-first pixel is i-th; its size, niter and ROI are those of
    detection.py:258-260 on the hand-known area and bounding box"""
    c = pc.case(name)
    boxes, debug = pc.oracle(name)
    assert [len(b) for b in boxes] == c["counts"]
    h, w = c["heat"].shape[1:3]
    for y, dbg, comps in zip(c["heat"], debug, c["comps"]):
        kept = _kept_by_scan(y, **c["kwargs"])
        assert [d["component"] for d in dbg] == [k[0] for k in kept]
        assert [k[1:6] for k in kept] == [tuple(cm) for cm in comps]  # the hand-known values are the scan's
        for d, cm in zip(dbg, comps):
            assert d["size"] == cm[0]
            assert d["niter"] == pc.niter_of(cm[0], cm[3], cm[4])
            assert d["roi"] == pc.roi_of(cm, w, h)


@pytest.mark.parametrize("name", BOXES)
def test_closed_form_boxes(name):
    c = pc.case(name)
    want = pc.expected_boxes(c)
    assert want is not None
    got = pc.oracle(name)[0]
    for g, w_ in zip(got, want):
        assert g.shape == w_.shape
        assert g.dtype == np.float32 or not len(g)
        assert np.array_equal(g, w_), (g, w_)


def test_stated_extents():
    """the numbers the cases were designed around, written out"""
    box = lambda l, t, r, b: np.array([[l, t], [r, t], [r, b], [l, b]], np.float32)  # noqa: E731
    assert np.array_equal(pc.oracle("split_side_by_side")[0][0][0], box(126, 26, 162, 44))
    assert np.array_equal(pc.oracle("split_stacked")[0][0][0], box(26, 126, 44, 162))
    assert np.array_equal(pc.oracle("split_last_is_tiny")[0][0][0], box(154, 36, 162, 44))
    corners = pc.oracle("even_kernel_corners")[0][0]
    assert np.array_equal(corners[2], box(6, 6, 16, 16))    # centre: x, y in 3 .. 8, one pixel left and two right
    assert np.array_equal(corners[0], box(0, 0, 8, 8))      # clipped above and left
    assert np.array_equal(corners[4], box(16, 16, 22, 22))  # clipped below and right: 8 .. 11
    big = pc.oracle("big_kernel_corner")
    assert [d["niter"] for d in big[1][0]] == [12, 3]
    assert np.array_equal(big[0][0][0], box(0, 0, 90, 90)) and np.array_equal(big[0][0][1], box(2, 120, 126, 126))
    assert [d["roi"] for d in big[1][0]] == [(0, 0, 53, 53), (0, 58, 64, 64)]
    grid = pc.oracle("pixel_grid")[0][0]
    assert len(grid) == 96 * 96
    assert np.array_equal(grid[0], box(0, 0, 2, 2))                  # pixel (0, 0): clipped above and left
    assert np.array_equal(grid[1], box(2, 0, 6, 2))                  # pixel (0, 2): clipped above
    assert np.array_equal(grid[96 + 1], box(2, 2, 6, 6))             # pixel (2, 2): the 3 x 3 block around it
    assert np.array_equal(grid[-1], box(378, 378, 382, 382))         # pixel (190, 190)
    for h, w in ((33, 31), (2, 2), (41, 1), (1, 1)):
        got = pc.oracle(f"all_foreground_{h}x{w}")[0]
        assert all(np.array_equal(g[0], box(0, 0, 2 * (w - 1), 2 * (h - 1))) for g in got)
    assert [len(b) for b in pc.oracle("square_grid")[0]] == [400, 0, 100]
    assert len(pc.oracle("equalities")[0][0]) == 1
    for name in ("signed_zero_max", "nan_in_text_positive", "nan_in_text_negative"):
        assert len(pc.oracle(name)[0][0]) == 1


def test_nan_cases_carry_the_bit_patterns():
    for name, bits in (("nan_in_text_positive", pc.NAN_POSITIVE), ("nan_in_text_negative", pc.NAN_NEGATIVE)):
        assert pc.case(name)["heat"][0, 7, 9, :1].view(np.uint32)[0] == bits
    z = pc.case("signed_zero_max")["heat"][0, 5:10, 5:15, 0]
    assert (z.view(np.uint32) == 0x80000000).all()


def test_detection_scores_of_the_float_key_cases():
    """the statement's score: the component maximum as np.max gives it (a NaN stays a NaN), a zero of either sign as +0.0"""
    from tests import scores_statement as ss

    def score(name):
        c = pc.case(name)
        kw = {k: v for k, v in c["kwargs"].items() if k in ("text_threshold", "link_threshold")}
        return [s.view(np.uint32).tolist() for s in ss.detection_scores(c["heat"], pc.oracle(name)[1], **kw)]

    assert score("link_only") == [[np.float32(0.9).view(np.uint32)]]
    assert score("signed_zero_max") == [[0]]
    assert np.isnan(ss.detection_scores(pc.case("nan_in_text_negative")["heat"], pc.oracle("nan_in_text_negative")[1])[0]).all()
    assert np.isnan(ss.detection_scores(pc.case("nan_in_text_positive")["heat"], pc.oracle("nan_in_text_positive")[1])[0]).all()
    neg = pc.case("negative_thresholds")
    got = ss.detection_scores(neg["heat"], pc.oracle("negative_thresholds")[1], text_threshold=-1.0, link_threshold=-1.0)
    assert got[0][0] == neg["heat"][0, ..., 0].max() > 0 > got[1][0] == neg["heat"][1, ..., 0].max()


@pytest.mark.parametrize("name", ERRORS)
def test_index_error_and_its_cause(name):
    from oracle import postproc

    c = pc.case(name)
    with pytest.raises(IndexError):
        postproc.get_boxes(c["heat"], **c["kwargs"])
    valid = postproc.get_boxes(pc.without_link(c["heat"]), **c["kwargs"])  # the text AND link overlap was the cause
    assert sum(len(b) for b in valid) >= 1
    if name == "empty_contour_among_valid":
        assert [len(b) for b in valid] == [1, 3]
        # the block is the second of image 1's three components in raster order: both neighbours are ordinary words
        text = c["heat"][1, ..., 0]
        firsts = [tuple(np.argwhere(_label_by_scan(text > 0.4)[0] == k)[0]) for k in (1, 2, 3)]
        assert firsts == [(3, 4), (15, 20), (30, 30)]
        assert (c["heat"][1, 15:21, 20:40] == 1.0).all() and c["heat"][1, ..., 1].sum() == 6 * 20


@pytest.mark.parametrize("name", pc.names("boxes", multi_image=True))
def test_images_alone_give_the_batch(name):
    """no state crosses the image seam: every image passed alone gives the boxes it gives inside the batch"""
    from oracle import postproc

    c = pc.case(name)
    batch = pc.oracle(name)[0]
    for i, want in enumerate(batch):
        got = postproc.get_boxes(c["heat"][i:i + 1], **c["kwargs"])[0]
        assert got.shape == want.shape and np.array_equal(got, want)


def test_seams_do_not_merge():
    """by hand: a merge across the row seam would make one component per image, across the image seam one in all"""
    boxes = pc.oracle("seams")[0]
    want = np.array([pc.rect_box((0, 0, 1, 5)), pc.rect_box((6, 0, 7, 5))])
    assert all(np.array_equal(b, want) for b in boxes) and len(boxes) == 2
