"""getBoxes' min-area rectangle under the opt-in OpenCV rule (include/kocr.h: kocr_set_min_area_rect, KOCR_RECT_OPENCV).

The reference calls ``cv2.boxPoints(cv2.minAreaRect(contour))`` (detection.py:273): float32 rotating calipers.  The default
rule (KOCR_RECT_EXACT, oracle/postproc.py::min_area_box) picks the rectangle exactly; the OpenCV rule follows
oracle/postproc.py::min_area_box_cv32 operation by operation.  The statement each box is compared with is the oracle's
getBoxes with every component's box rebuilt by ``box_from_hull(hull, hx, hy, cv32=True)`` -- the hull's extremes are the
fragment's, which is all the diamond rule reads (as scripts/minarearect_deviation.py does).  Bar: bit-identical float32
corners.  The fixtures must also tell the rules apart: each random map asserts a minimum number of components whose exact
and cv32 boxes differ, at least one of them by another rectangle altogether."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _check(got, want):
    assert len(got) == len(want)
    for g, w_ in zip(got, want):
        assert g.shape == w_.shape, (g.shape, w_.shape)
        if len(w_):
            assert np.array_equal(g, w_.astype(np.float32)), np.abs(g - w_).max()


def _statements(y, **kw):
    """(exact boxes, cv32 boxes, per-component max corner deviation between the two) of the oracle's getBoxes on y."""
    from oracle import postproc
    from tests.postproc_cases import rule_statements

    return rule_statements(*postproc.get_boxes(y, return_debug=True, **kw))


def _hull_shapes():
    """One 700 x 1000 heat-map aimed at K13's branches: a digital diamond of 601 rows (more hull candidates than the LDS
    chains hold: the global-scratch hull), an ellipse (many hull vertices), a 1-pixel vertical line, a single pixel, a thin
    slanted bar and a small square.  The dilation (k >= 3, detection.py:258-264) gives every one of them a hull of at least
    three vertices; _degenerate_maps reaches the n == 2 and n == 1 branches."""
    h, w = 700, 1000
    yy, xx = np.mgrid[0:h, 0:w]
    text = np.zeros((h, w), np.float32)
    text[np.abs(xx - 310) + np.abs(yy - 320) <= 300] = 1.0                      # large diamond
    text[((xx - 780) / 120.0) ** 2 + ((yy - 250) / 200.0) ** 2 <= 1.0] = 1.0    # ellipse
    text[30:680, 950] = 1.0                                                    # vertical line
    text[640, 700] = 1.0                                                       # single pixel (size_threshold 1)
    text[(np.abs((yy - 560) - 0.37 * (xx - 880)) <= 2.0) & (np.abs(xx - 880) <= 45)] = 1.0  # slanted bar
    text[660:666, 640:646] = 1.0                                               # square
    return np.stack([text, np.zeros_like(text)], -1)[None]


def _degenerate_maps():
    """Hulls of two vertices and of one: on a heat-map one pixel wide (or high) the dilation ROI is clipped to that line,
    so a vertical (horizontal) segment stays a segment; on a 1 x 1 map one pixel stays one pixel."""
    col = np.zeros((1, 700, 1, 2), np.float32)
    col[0, 30:680, 0, 0] = 1.0
    row = np.zeros((1, 1, 500, 2), np.float32)
    row[0, 0, 17:401, 0] = 1.0
    return {"column": col, "row": row, "pixel": np.array([[[[1.0, 0.0]]]], np.float32)}


def _line(cell, rng):
    """A 1-pixel 4-connected line of random slope (4-connected so that it stays one component)."""
    m = np.zeros((cell, cell), bool)
    lo, hi = 3, cell - 4
    x0, y0, x1, y1 = (int(v) for v in rng.integers(lo, hi, 4))
    n = 4 * max(abs(x1 - x0), abs(y1 - y0)) + 1
    px = py = None
    for t in np.linspace(0.0, 1.0, n):
        x, y = int(round(x0 + t * (x1 - x0))), int(round(y0 + t * (y1 - y0)))
        if px is not None and x != px and y != py:
            m[py, x] = True
        m[y, x] = True
        px, py = x, y
    return m


def _shape(kind, cell, rng):
    """A boolean cell x cell mask holding one random shape, at least 2 pixels from the cell's border."""
    yy, xx = np.mgrid[0:cell, 0:cell].astype(np.float64)
    c = (cell - 1) / 2.0
    cx, cy = c + rng.uniform(-0.5, 0.5), c + rng.uniform(-0.5, 0.5)
    th = rng.uniform(0.0, np.pi)
    u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
    v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
    big = (cell - 6) / 2.0
    if kind == 0:    # rotated rectangle
        a = rng.uniform(1.5, big)
        b = rng.uniform(0.5, a)
        m = (np.abs(u) <= a) & (np.abs(v) <= b)
    elif kind == 1:  # rotated ellipse
        a = rng.uniform(1.5, big)
        b = rng.uniform(1.0, a)
        m = (u / a) ** 2 + (v / b) ** 2 <= 1.0
    elif kind == 2:  # 1-pixel line
        m = _line(cell, rng)
    elif kind == 3:  # near-square: the diamond rule of detection.py:276-281
        a = rng.uniform(2.0, min(big, 20.0) / 1.1)
        b = a * rng.uniform(0.93, 1.07)
        th = rng.choice([0.0, rng.uniform(0.0, np.pi)])
        u = (xx - cx) * np.cos(th) + (yy - cy) * np.sin(th)
        v = -(xx - cx) * np.sin(th) + (yy - cy) * np.cos(th)
        m = (np.abs(u) <= a) & (np.abs(v) <= b)
    else:            # integer octagon, unequal corner cuts: hull edges whose rectangles tie exactly in area are common
        W = int(rng.integers(8, min(cell - 6, 40)))
        H = int(rng.integers(6, min(cell - 6, 40)))
        c1 = int(rng.integers(1, min(W, H) - 1))
        c2 = int(rng.integers(1, min(W, H) - c1))
        x, y = xx - 3, yy - 3
        m = ((x >= 0) & (x <= W) & (y >= 0) & (y <= H) & (x + y >= c1) & (x + y <= W + H - c1) & (x - y <= W - c2)
             & (y - x <= H - c2))
    m = m.copy()
    m[:2] = m[-2:] = False
    m[:, :2] = m[:, -2:] = False
    return m


def _random_map(seed, cell, grid, kinds):
    """grid x grid cells of cell pixels, one random shape of the given kinds per cell (cells never touch)."""
    rng = np.random.default_rng(seed)
    text = np.zeros((cell * grid, cell * grid), np.float32)
    for gy in range(grid):
        for gx in range(grid):
            kind = kinds[int(rng.integers(len(kinds)))]
            text[gy * cell:(gy + 1) * cell, gx * cell:(gx + 1) * cell] = _shape(kind, cell, rng)
    return np.stack([text, np.zeros_like(text)], -1)[None]


@pytest.mark.parametrize("name,nverts", [("shapes", [8, 4, 112, 14, 4, 4]), ("column", [2]), ("row", [2]), ("pixel", [1])])
def test_hull_shapes_opencv_rule(ctx, name, nverts):
    from oracle import postproc

    y = _hull_shapes() if name == "shapes" else _degenerate_maps()[name]
    _, dbg = postproc.get_boxes(y, size_threshold=1, return_debug=True)
    assert [len(c["hull"]) for c in dbg[0]] == nverts  # the branches the map is meant to reach
    exact, want, _ = _statements(y, size_threshold=1)
    _check(ctx.get_boxes(y, size_threshold=1, min_area_rect="opencv"), want)
    _check(ctx.get_boxes(y, size_threshold=1), exact)


@pytest.mark.parametrize("seed,cell,grid,kinds,min_differ", [
    (1, 48, 16, (0, 1, 2, 3, 4), 40),   # 256 cells, shapes of 3 - 42 px (measured: 97 of 249 boxes differ, 15 > 0.5 px)
    (2, 48, 16, (0, 1, 2, 3, 4), 40),   # (94 of 250, 21)
    (3, 40, 16, (2, 4), 60),            # lines of many slopes and octagons only (134 of 241, 35)
    (4, 208, 5, (0, 1, 2), 3),          # 25 rectangles, ellipses and lines up to 200 px (8 of 25, 2)
])
def test_random_components_opencv_rule(ctx, seed, cell, grid, kinds, min_differ):
    y = _random_map(seed, cell, grid, kinds)
    exact, want, dev = _statements(y)
    assert len(want[0]) >= grid * grid * 0.7
    # the fixture tells the two rules apart: boxes that are not bit-identical, at least one of them another rectangle
    assert (dev > 0).sum() >= min_differ, (dev > 0).sum()
    assert (dev > 0.5).sum() >= 1
    got = ctx.get_boxes(y, min_area_rect="opencv")
    _check(got, want)
    _check(ctx.get_boxes(y), exact)


@pytest.fixture(scope="module")
def bench_setup():
    """A private context with the benchmark's head calibration (scripts/minarearect_deviation.py), three bench pages at
    768 x 768 resized x 2 on the device, and their heat-maps."""
    import bench
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    pages = bench.make_pages(3, bench.SIDE, seed=4)
    side = bench.SIDE * bench.SCALE
    big = c.resize_pad(pages, (side, side))
    cw = keras_ocr_amd.weights.synthetic_craft_weights(1234)
    c.load_craft(cw)
    frac = 0.0055
    cw = keras_ocr_amd.weights.calibrate_craft_head(cw, c.craft_forward(big), text_frac=frac, link_frac=frac / 3, top_q=0.9999)
    c.load_craft(cw)
    heat = c.craft_forward(big)
    yield c, pages, big, heat
    c.close()


def test_bench_pages_opencv_rule(bench_setup):
    c, _, _, heat = bench_setup
    exact, want, dev = _statements(heat)
    assert sum(len(b) for b in want) >= 30
    assert (dev > 0).sum() >= 1
    _check(c.get_boxes(heat, min_area_rect="opencv"), want)
    _check(c.get_boxes(heat), exact)


def test_per_call_rule_is_restored_and_contexts_are_independent(ctx):
    import keras_ocr_amd

    y = _random_map(1, 48, 16, (0, 1, 2, 3, 4))
    assert ctx.get_min_area_rect() == "exact"
    fresh = ctx.get_boxes(y)
    cv = ctx.get_boxes(y, min_area_rect="opencv")
    assert ctx.get_min_area_rect() == "exact"
    after = ctx.get_boxes(y)
    assert any(not np.array_equal(a, b) for a, b in zip(cv, fresh))
    _check(after, fresh)
    # the per-call value overrides the context's rule in both directions
    c2 = keras_ocr_amd.Context(0)
    try:
        c2.set_min_area_rect("opencv")
        assert c2.get_min_area_rect() == "opencv" and ctx.get_min_area_rect() == "exact"
        _check(c2.get_boxes(y), cv)
        _check(c2.get_boxes(y, min_area_rect="exact"), fresh)
        assert c2.get_min_area_rect() == "opencv"
        _check(ctx.get_boxes(y), fresh)
        c2.set_min_area_rect("exact")
        _check(c2.get_boxes(y), fresh)
    finally:
        c2.close()


def test_unknown_rule_is_rejected(ctx):
    import ctypes
    import keras_ocr_amd

    y = _hull_shapes()
    for bad in ("cv2", "OpenCV", 1, True):
        with pytest.raises(ValueError):
            ctx.get_boxes(y, min_area_rect=bad)
        with pytest.raises(ValueError):
            ctx.set_min_area_rect(bad)
    with pytest.raises(ValueError):
        ctx.detect(np.zeros((1, 64, 64, 3), np.uint8), min_area_rect="cv2")
    with pytest.raises(ValueError):
        keras_ocr_amd.detection.getBoxes(y, min_area_rect="cv2")
    assert ctx.get_min_area_rect() == "exact"
    lib = keras_ocr_amd.load_library()
    h = ctypes.c_void_p(ctx._h.value)  # pylint: disable=protected-access
    assert lib.kocr_set_min_area_rect(h, 2) == -1 and lib.kocr_set_min_area_rect(h, -1) == -1  # KOCR_EINVAL
    assert lib.kocr_get_min_area_rect(h) == 0
    assert lib.kocr_get_min_area_rect(None) == -1


def test_detect_carries_the_rule(bench_setup):
    import keras_ocr_amd

    c, _, big, heat = bench_setup
    want = c.get_boxes(heat, min_area_rect="opencv")
    _check(c.detect(big, min_area_rect="opencv"), want)
    _check(c.detect(big), c.get_boxes(heat))
    assert c.get_min_area_rect() == "exact"
    det = keras_ocr_amd.detection.Detector(weights=_calibrated(c, big), ctx=c)
    _check(det.detect(list(big), min_area_rect="opencv"), want)
    _check(det.detect(list(big)), c.get_boxes(heat))


def _calibrated(c, big):
    import keras_ocr_amd

    cw = keras_ocr_amd.weights.synthetic_craft_weights(1234)
    c.load_craft(cw)
    frac = 0.0055
    return keras_ocr_amd.weights.calibrate_craft_head(cw, c.craft_forward(big), text_frac=frac, link_frac=frac / 3,
                                                       top_q=0.9999)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_pipeline_carries_the_rule(bench_setup, crnn_weights, dtype):
    """Pipeline.recognize(detection_kwargs={"min_area_rect": "opencv"}): boxes = getBoxes under that rule on the detector's
    heat-maps, adjusted to input pixels, and texts = recognize_from_boxes on them -- on the fused uint8 path and on the float
    stage-wise path."""
    import keras_ocr_amd
    from keras_ocr_amd import tools

    c, pages, big, heat = bench_setup
    pages = pages[:2]
    det = keras_ocr_amd.detection.Detector(weights=_calibrated(c, big), ctx=c)
    rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=c)
    pipe = keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)
    images = [p.astype(dtype) for p in pages]
    got = pipe.recognize(images, detection_kwargs={"min_area_rect": "opencv"})
    assert c.get_min_area_rect() == "exact"
    if dtype == np.uint8:
        batch = big[:2]
        x = batch
    else:
        resized = [tools.resize_image(im, max_scale=2, max_size=2048, ctx=c)[0] for im in images]
        batch = np.array([tools.pad(r, width=r.shape[1], height=r.shape[0]) for r in resized])
        x = batch.astype("float32")  # Detector.detect's normalisation (detection.py:34-42)
        x -= np.array([0.485, 0.456, 0.406]) * 255
        x /= np.array([0.229, 0.224, 0.225]) * 255
    heat2 = c.craft_forward(x)
    boxes = c.get_boxes(heat2, min_area_rect="opencv")
    assert any(not np.array_equal(a, b) for a, b in zip(boxes, c.get_boxes(heat2)))
    texts = rec.recognize_from_boxes(batch, boxes)
    assert sum(len(b) for b in boxes) >= 20
    for g, b, t in zip(got, boxes, texts):
        assert [x_[0] for x_ in g] == t
        assert np.array_equal(np.stack([x_[1] for x_ in g]), tools.adjust_boxes(boxes=b, boxes_format="boxes", scale=0.5))


def test_getboxes_public_function():
    import keras_ocr_amd
    from keras_ocr_amd import detection

    y = _random_map(2, 48, 16, (0, 1, 2, 3, 4))
    exact, cv32, _ = _statements(y)
    _check(detection.getBoxes(y), exact)
    _check(detection.getBoxes(y, min_area_rect="opencv"), cv32)
    _check(detection.getBoxes(y, min_area_rect="exact"), exact)
    assert keras_ocr_amd.default_context().get_min_area_rect() == "exact"
    kw = dict(detection_threshold=0.9, text_threshold=0.5, link_threshold=0.6, size_threshold=30)
    _check(detection.getBoxes(y, min_area_rect="opencv", **kw), _statements(y, **kw)[1])
