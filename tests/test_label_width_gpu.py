"""The fused pipeline at other label widths: a recogniser built with rnn_steps_to_discard d has label rows of 50 - d columns
(kocr_crnn_label_width), and everything downstream of the recogniser's kernels CARRIES rows of that width -- the per-batch
row offsets of the fused tail, the capacity-overflow refetch, the resident getters, the tiled call's shared tail, the
device-resident entry.  The kernels themselves are held against the oracle at d = 0 and 5 elsewhere (tests/test_crnn_gpu.py);
here the carriers are, at d = 0, 5 and 49 (rows of 50, 45 and 1 columns: a 4-byte row pitch is the smallest at which a pitch or
alignment assumption can fail), with d = 2 as the control.

Every comparison is exact: strings equal, boxes and label rows bit for bit.  One fresh context per width (the session's context
keeps the discard other modules rely on); the staged composition of every width is computed once and shared.

The second part states the width contract of the resident results (include/kocr.h): rows keep the width they were PRODUCED
with, whatever kocr_crnn_set_rnn_steps_to_discard says between kocr_pipeline and the fetch."""
import types

import numpy as np
import pytest

from tests import synth, tiling_statement as ts

pytestmark = pytest.mark.gpu

DISCARDS = (2, 0, 5, 49)
PATTERN = {"letters+": r"[a-z]+"}


def _pages():
    return [synth.text_page(96, 128, 5, seed=21), synth.text_page(80, 100, 4, seed=22)]


@pytest.fixture(scope="module")
def calibrated(craft_weights):
    """The detector's head calibrated as in tests/test_pipeline_gpu.py, so that the random-init network emits word boxes"""
    import keras_ocr_amd
    from oracle import craft as ocraft, tools as otools

    page = synth.text_page(96, 128, 5, seed=21)[None]
    big = np.stack([otools.resize_image(p, 2, 2048)[0] for p in page])
    heat = ocraft.detector_predict(craft_weights, big)
    return keras_ocr_amd.weights.calibrate_craft_head(craft_weights, heat, text_frac=0.10, link_frac=0.04)


def _build(calibrated, crnn_weights, discard):
    import keras_ocr_amd
    from keras_ocr_amd.recognition import DEFAULT_BUILD_PARAMS

    c = keras_ocr_amd.Context(0)
    det = keras_ocr_amd.detection.Detector(weights=calibrated, ctx=c)
    rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=c,
                                               build_params=dict(DEFAULT_BUILD_PARAMS, rnn_steps_to_discard=discard))
    return c, keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)


@pytest.fixture(scope="module")
def at(calibrated, crnn_weights):
    """at(d): a pipeline at discard d on a context of its own, and the staged composition of its stages on the two pages:
    resize_pad -> detect -> recognize_from_boxes (test_fused_equals_stagewise's).  Built on first use, shared by the module's
    tests, closed at its end."""
    from oracle import tools as otools

    made = {}

    def build(d):
        if d in made:
            return made[d]
        c, pipe = _build(calibrated, crnn_weights, d)
        made[d] = types.SimpleNamespace(ctx=c)  # closed below whatever happens next
        assert c.crnn_label_width() == 50 - d
        pages = _pages()
        resized = [c.resize_pad(p[None], (p.shape[1] * 2, p.shape[0] * 2))[0] for p in pages]
        hmax, wmax = max(r.shape[0] for r in resized), max(r.shape[1] for r in resized)
        batch = np.stack([otools.pad(r, width=wmax, height=hmax) for r in resized])
        boxes = pipe.detector.detect(batch)
        assert sum(len(b) for b in boxes) >= 4, "calibration should produce word boxes"
        texts = pipe.recognizer.recognize_from_boxes(batch, boxes)
        made[d] = types.SimpleNamespace(d=d, lw=50 - d, ctx=c, pipe=pipe, pages=pages, batch=batch, boxes=boxes, texts=texts,
                                        m=sum(len(b) for b in boxes))
        return made[d]

    yield build
    for entry in made.values():
        entry.ctx.close()


def every_width(test):
    return pytest.mark.parametrize("d", DISCARDS, ids=[f"discard_{d}" for d in DISCARDS])(test)


def _same_boxes(fused, boxes):
    """The fused call's boxes (input-image pixels, scale 2) are the staged ones' bits"""
    assert [len(f) for f in fused] == [len(b) for b in boxes]
    for f, b in zip(fused, boxes):
        if len(b):
            assert np.array_equal(np.stack([x[1] for x in f]), b * np.float32(0.5))


def _same(a, b):
    assert len(a) == len(b)
    for pa, pb in zip(a, b):
        assert [x[0] for x in pa] == [x[0] for x in pb]
        assert len(pa) == len(pb) and all(np.array_equal(x[1], y[1]) for x, y in zip(pa, pb))


@every_width
def test_fused_equals_stagewise(at, d):
    built = at(d)
    fused = built.pipe.recognize(built.pages)
    assert [[x[0] for x in f] for f in fused] == built.texts
    _same_boxes(fused, built.boxes)
    assert all(len(t) <= built.lw for page in built.texts for t in page)


def test_control_is_the_default_build(at, crnn_weights):
    """d = 2 through build_params is the default recogniser: the same strings, boxes and label rows"""
    import keras_ocr_amd

    built = at(2)
    want = built.pipe.recognize_raw(built.pages)
    rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=built.ctx)
    default = keras_ocr_amd.pipeline.Pipeline(detector=built.pipe.detector, recognizer=rec)
    got = default.recognize_raw(built.pages)
    assert got[1].shape == (built.m, 48) and np.array_equal(got[1], want[1])
    assert all(np.array_equal(a, b) for a, b in zip(got[0], want[0]))
    _same(default.recognize(built.pages), built.pipe.recognize(built.pages))


@every_width
def test_raw_label_rows_have_the_width(at, d):
    built = at(d)
    boxes, labels = built.pipe.recognize_raw(built.pages)
    assert labels.shape == (built.m, built.lw) and built.m > 0 and labels.dtype == np.int32
    assert built.pipe.recognizer._decode(labels) == [t for page in built.texts for t in page]  # pylint: disable=protected-access
    # behind its text a row is -1 and nothing else
    assert all((row[len(t):] == -1).all() and (row[:len(t)] >= 0).all()
               for row, t in zip(labels, (t for page in built.texts for t in page)))
    assert built.pipe.recognize_raw([])[1].shape == (0, built.lw)


@every_width
def test_capacity_overflow_refetch(at, d):
    """More boxes than cap: the whole chain runs once and kocr_pipeline_results copies the resident rows -- the same boxes and
    the same label rows, bit for bit, as the call whose buffers were large enough"""
    built = at(d)
    pages = built.pages
    _, dhs, dws, hmax, wmax = built.pipe._plan([p.shape for p in pages])  # pylint: disable=protected-access
    args = (pages, [p.shape[0] for p in pages], [p.shape[1] for p in pages], dhs, dws, hmax, wmax)
    big_boxes, big_labels = built.ctx.pipeline(*args, cap=64)
    assert max(len(b) for b in big_boxes) > 2 and big_labels.shape == (built.m, built.lw)
    assert all(np.array_equal(a, b) for a, b in zip(big_boxes, built.boxes))
    small_boxes, small_labels = built.ctx.pipeline(*args, cap=2)
    assert [len(b) for b in small_boxes] == [len(b) for b in big_boxes]
    assert all(np.array_equal(a, b) for a, b in zip(small_boxes, big_boxes))
    assert small_labels.shape == big_labels.shape and np.array_equal(small_labels, big_labels)
    # ... and more crops than max_crops
    few_boxes, few_labels = built.ctx.pipeline(*args, cap=64, max_crops=2)
    assert all(np.array_equal(a, b) for a, b in zip(few_boxes, big_boxes)) and np.array_equal(few_labels, big_labels)
    assert built.ctx.pipeline_results_shape() == (built.m, built.lw)
    res = built.ctx.pipeline_device_results()
    assert res["n"] == 2 and res["m"] == built.m and res["lw"] == built.lw


@every_width
def test_device_resident_batch_equals_host_batch(at, d):
    built = at(d)
    import torch

    pages = np.stack([synth.text_page(96, 128, 5, seed=21), synth.text_page(96, 128, 4, seed=22)])
    host = built.pipe.recognize(pages)
    assert sum(len(p) for p in host) >= 4
    t = torch.from_numpy(pages).cuda()
    _same(built.pipe.recognize_device(t.data_ptr(), 2, 96, 128), host)
    res = {}
    raw = built.pipe.recognize_device_raw(t.data_ptr(), 2, 96, 128, device_results=res)
    assert raw[1].shape == (sum(len(p) for p in host), built.lw) and res["lw"] == built.lw and res["m"] == len(raw[1])
    # the rows as they lie in HBM, viewed at the reported width
    from keras_ocr_amd.dist import _DeviceArray
    lab = torch.as_tensor(_DeviceArray(res["labels"], (res["m"], res["lw"]), "<i4"), device="cuda").cpu().numpy()
    assert np.array_equal(lab, raw[1])


@every_width
def test_scores_have_the_width(at, d):
    built = at(d)
    scored = built.pipe.recognize_with_scores(built.pages)
    assert [[t for t, _, _ in page] for page in scored] == built.texts
    _same_boxes(scored, built.boxes)
    boxes, labels, (det, log_word, chars) = built.pipe.recognize_raw(built.pages, return_scores=True)
    assert chars.shape == (built.m, built.lw) and chars.dtype == np.float32 and log_word.shape == (built.m,)
    assert labels.shape == (built.m, built.lw)
    # one character score per decoded label, zero behind the decode
    flat = [t for page in built.texts for t in page]
    assert all((row[:len(t)] > 0).all() and (row[:len(t)] <= 1).all() and not row[len(t):].any() for row, t in zip(chars, flat))
    assert all(len(s.characters) == len(t) for page in scored for t, _, s in page)


@every_width
def test_beam_alternatives_decode(at, d):
    built = at(d)
    kw = {"beam_width": 4, "top_paths": 2}
    beams = built.pipe.recognize(built.pages, recognition_kwargs=kw)
    _same_boxes(beams, built.boxes)
    for page in beams:
        for alternatives, _ in page:
            assert isinstance(alternatives, list) and 1 <= len(alternatives) <= 2
            assert all(isinstance(t, str) and len(t) <= built.lw and np.isfinite(v) for t, v in alternatives)
            assert len(alternatives) == 1 or alternatives[0][1] >= alternatives[1][1]
    raw = built.pipe.recognize_raw(built.pages, recognition_kwargs=kw)
    assert raw[3][0].shape == (built.m, 2, built.lw) and raw[3][1].shape == (built.m, 2)
    # the same alternatives through recognize_from_boxes on the staged boxes
    staged = built.pipe.recognizer.recognize_from_boxes(built.batch, built.boxes, **kw)
    assert [[a for a, _ in page] for page in beams] == staged


@every_width
def test_pattern_and_flip_equal_the_staged_calls(at, d):
    built = at(d)
    rec = built.pipe.recognizer
    rec.set_patterns(PATTERN)
    try:
        on = built.pipe.recognize(built.pages, recognition_kwargs={"pattern": "letters+"})
        _same_boxes(on, built.boxes)
        assert [[w for w, _ in page] for page in on] == rec.recognize_from_boxes(built.batch, built.boxes, pattern="letters+")
        assert all(w == (None, -np.inf) or (isinstance(w[0], str) and 1 <= len(w[0]) <= built.lw) for page in on for w, _ in page)
        raw = built.pipe.recognize_raw(built.pages, recognition_kwargs={"pattern": "letters+"})
        assert raw[-1][0].shape == (built.m, built.lw)
    finally:
        rec.set_patterns(None)
    flipped = built.pipe.recognize(built.pages, recognition_kwargs={"orientation": "flip"})
    staged = rec.recognize_from_boxes(built.batch, built.boxes, orientation="flip", return_orientation=True)
    assert [[t for t, _ in page] for page in flipped] == [[t for t, _ in page] for page in staged]
    for page, group in zip(flipped, staged):
        assert all(np.array_equal(box, how.box * np.float32(0.5)) for (_, box), (_, how) in zip(page, group))


def test_tiled_call_shares_the_tail(at, calibrated):
    """recognize_tiled on fixture B (6 tiles) == its staged form (tests/test_tiling_gpu.py: test_fused_equals_staged), at
    rows of 45 columns"""
    import keras_ocr_amd

    built = at(5)
    f = ts.fixture("B")
    assert len(f.plan.origins) == 6
    c, rec = built.ctx, built.pipe.recognizer
    try:
        pipe = keras_ocr_amd.pipeline.Pipeline(detector=keras_ocr_amd.detection.Detector(weights=f.weights, ctx=c), recognizer=rec)
        fused = pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap)
        dh, dw = f.page.shape[0] * f.scale, f.page.shape[1] * f.scale
        canvas = c.resize_pad(f.page[None], (dw, dh), out_hw=f.plan.canvas)
        tiles = c.gather_tiles(canvas, f.tile, f.overlap)
        heat = c.stitch_heat(c.craft_forward(tiles), f.plan.canvas, f.tile, f.overlap)
        boxes = c.get_boxes(heat)
        texts = rec.recognize_from_boxes(canvas, boxes)
        assert len(boxes[0]) >= 4, "calibration should produce word boxes"
        assert len(fused) == 1 and [t for t, _ in fused[0]] == texts[0]
        assert np.array_equal(np.stack([b for _, b in fused[0]]), boxes[0] * np.float32(0.5))
        h, w = f.page.shape[:2]
        args = ([f.page], [h], [w], [dh], [dw], f.tile, f.overlap)
        big_boxes, big_labels = c.pipeline_tiled(*args, cap=64)
        small_boxes, small_labels = c.pipeline_tiled(*args, cap=2)
        assert len(big_boxes[0]) > 2 and big_labels.shape == (len(boxes[0]), 45)
        assert np.array_equal(small_boxes[0], big_boxes[0]) and np.array_equal(small_labels, big_labels)
        assert c.pipeline_results_shape() == (len(boxes[0]), 45)
    finally:
        keras_ocr_amd.detection.Detector(weights=calibrated, ctx=c)  # the module's detector back on the shared context


@pytest.mark.parametrize("d", [0, 5], ids=["discard_0", "discard_5"])
def test_end_to_end_vs_oracle(at, calibrated, crnn_weights, d):
    """test_end_to_end_vs_oracle of tests/test_pipeline_gpu.py at its bars, the oracle's recogniser run at the same discard"""
    from oracle import pipeline as opipe, tools as otools
    from tests.parity import compare_page, flips

    built = at(d)
    got = built.pipe.recognize(built.pages)
    heats = []
    want = opipe.recognize(calibrated, crnn_weights, built.pages, scale=2, max_size=2048, heat_out=heats, rnn_steps_to_discard=built.d)
    resized = [otools.resize_image(p, 2, 2048) for p in built.pages]
    h_gpu = built.ctx.craft_forward(built.batch)
    report = {"boxes_equal": 0, "boxes_moved_by_flips": 0, "flipped_pixels": 0, "pixels": 0}
    for g, w_, hg, hr, (_, sc) in zip(got, want, h_gpu, heats[0], resized):
        fl = flips(hg, hr)
        if len(fl) == 0:
            assert len(g) == len(w_)
        compare_page(g, w_, fl, sc, hr.shape[:2], report)
    print(f"e2e at discard {built.d}:", report)
    assert report["boxes_equal"] >= 4
    assert report["flipped_pixels"] <= 2


# ---- resident results keep their width ---------------------------------------------------------------------------------------
SENTINEL = -7777


@pytest.mark.parametrize("produced, changed_to", [(2, 0), (5, 2), (0, 5)], ids=["48_then_50", "45_then_48", "50_then_45"])
def test_resident_rows_keep_the_width_they_were_produced_with(calibrated, crnn_weights, produced, changed_to):
    """include/kocr.h, "The width contract": kocr_crnn_set_rnn_steps_to_discard between kocr_pipeline and the fetch changes
    kocr_crnn_label_width() but not the resident rows.  kocr_pipeline_results copies M rows of the PRODUCED width, densely --
    never re-pitched to the new width -- and writes nothing behind them (the buffer is sized for the wider of the two and
    filled with a sentinel); kocr_pipeline_results_shape and Context.pipeline_device_results()["lw"] report that width, and
    the device rows viewed at it are the rows."""
    import torch
    from keras_ocr_amd._lib import _ptr
    from keras_ocr_amd.dist import _DeviceArray

    c, pipe = _build(calibrated, crnn_weights, produced)
    try:
        pages = _pages()
        _, dhs, dws, hmax, wmax = pipe._plan([p.shape for p in pages])  # pylint: disable=protected-access
        boxes, labels = c.pipeline(pages, [p.shape[0] for p in pages], [p.shape[1] for p in pages], dhs, dws, hmax, wmax)
        lw, new = 50 - produced, 50 - changed_to
        m = len(labels)
        assert m >= 3 and labels.shape == (m, lw)
        c.crnn_set_rnn_steps_to_discard(changed_to)
        assert c.crnn_label_width() == new
        assert c.pipeline_results_shape() == (m, lw)
        res = c.pipeline_device_results()
        assert res["m"] == m and res["lw"] == lw and res["n"] == 2
        lib, h = c._lib, c._h  # pylint: disable=protected-access
        cap = res["cap"] + 3
        got_b = np.zeros((2, cap, 4, 2), np.float32)
        flat = np.full((m + 5) * max(lw, new), SENTINEL, np.int32)
        assert lib.kocr_pipeline_results(h, _ptr(got_b), cap, _ptr(flat), m + 5) == 0
        assert np.array_equal(flat[:m * lw].reshape(m, lw), labels), "the rows were re-pitched or cut short"
        assert (flat[m * lw:] == SENTINEL).all(), "written past the M rows of the produced width"
        assert all(np.array_equal(got_b[i, :len(b)], b) for i, b in enumerate(boxes))
        lab = torch.as_tensor(_DeviceArray(res["labels"], (m, res["lw"]), "<i4"), device="cuda").cpu().numpy()
        assert np.array_equal(lab, labels)
        # too few rows' worth of buffer is still refused before anything is written
        small = np.full(lw, SENTINEL, np.int32)
        assert lib.kocr_pipeline_results(h, _ptr(got_b), cap, _ptr(small), 1) == -4 and (small == SENTINEL).all()
        # the next call produces rows of the new width
        again = c.pipeline(pages, [p.shape[0] for p in pages], [p.shape[1] for p in pages], dhs, dws, hmax, wmax)
        assert again[1].shape == (m, new) and c.pipeline_results_shape() == (m, new)
        assert all(np.array_equal(a, b) for a, b in zip(again[0], boxes))
    finally:
        c.close()
