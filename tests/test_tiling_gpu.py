"""Tiled pages on the GPU ("Tiled pages"): the two copies bit for bit against their statement
(tests/tiling_statement.py), the tiled detector pass against the oracle's within the project's heat-map bound, the fused
call against its stages exactly and against the oracle end to end, and the tail it shares with kocr_pipeline.

The fixtures A and B (tests/tiling_statement.py; tests/test_tiling_statement_cpu.py asserts their box counts) are small pages
cut into 28 and 6 tiles, with most boxes lying across a core seam."""
import numpy as np
import pytest

from tests import synth, tiling_statement as ts

pytestmark = pytest.mark.gpu

# (T, O, dh, dw): several tiles with a ragged last one; no overlap and one pixel more than a tile; odd sizes; a canvas without
# pad; a page smaller than one tile; a non-power-of-two tile with one tile across; exactly one tile
COPY_CASES = [(64, 16, 120, 180), (64, 0, 64, 65), (64, 16, 91, 136), (128, 32, 192, 256), (64, 16, 30, 40), (96, 32, 97, 33),
              (64, 16, 64, 64)]

_loaded = {}


def pipe_for(ctx, crnn_weights, name, weights=None):
    """The pipeline of fixture ``name`` on the session's context; the detector's weights are loaded when another fixture's
    (or another module's) are there"""
    import keras_ocr_amd

    if _loaded.get("name") != name:
        det = keras_ocr_amd.detection.Detector(weights=ts.fixture(name).weights if weights is None else weights, ctx=ctx)
        rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=ctx)
        _loaded.update(name=name, pipe=keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec))
    return _loaded["pipe"]


@pytest.fixture(scope="module", autouse=True)
def _forget_loaded_weights():
    _loaded.clear()
    yield
    _loaded.clear()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("tile,overlap,dh,dw", COPY_CASES)
def test_library_plan_equals_the_statement(ctx, tile, overlap, dh, dw):
    p = ts.plan(dh, dw, tile, overlap)
    assert ctx.tile_plan(dh, dw, tile, overlap) == p.counts + p.canvas + (p.stride, len(p.origins))


@pytest.mark.parametrize("tile,overlap,dh,dw", COPY_CASES)
def test_gather_tiles_bit_exact(ctx, tile, overlap, dh, dw):
    p = ts.plan(dh, dw, tile, overlap)
    canvas = np.random.default_rng(dh * 1000 + dw).integers(0, 256, (2,) + p.canvas + (3,), dtype=np.uint8)
    got = ctx.gather_tiles(canvas, tile, overlap)
    want = np.concatenate([ts.gather(c, p) for c in canvas])
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want)


@pytest.mark.parametrize("tile,overlap,dh,dw", COPY_CASES)
def test_stitch_heat_bit_exact(ctx, tile, overlap, dh, dw):
    p = ts.plan(dh, dw, tile, overlap)
    n_tiles, t2 = len(p.origins), tile // 2
    # every value names its (canvas, tile, y, x, channel): a pixel taken from the wrong tile, or from the wrong place, shows
    heat = np.arange(2 * n_tiles * t2 * t2 * 2, dtype=np.float32).reshape(2 * n_tiles, t2, t2, 2)
    assert heat[-1, -1, -1, -1] < 2 ** 24
    # a NaN with a payload and a negative zero inside cores (they must arrive as they are), and another NaN in a halo (it
    # must not arrive at all) when there is one
    y0, _, x0, _ = (v // 2 for v in p.cores[-1])
    oy, ox = (v // 2 for v in p.origins[-1])
    _bits(heat)[n_tiles - 1, y0 - oy, x0 - ox, 0] = 0x7FC00123
    _bits(heat)[2 * n_tiles - 1, y0 - oy + 1, x0 - ox + 1, 1] = np.int32(-2 ** 31)
    if overlap and n_tiles > 1:
        _bits(heat)[0, t2 - 1, t2 - 1, 0] = 0x7FC00456  # the first tile's last pixel lies in its halo
    got = ctx.stitch_heat(heat, p.canvas, tile, overlap)
    assert (_bits(got) == 0x7FC00456).sum() == 0
    want = np.stack([ts.stitch(heat[i * n_tiles:(i + 1) * n_tiles], p, shrink=2) for i in range(2)])
    assert got.shape == want.shape == (2, p.canvas[0] // 2, p.canvas[1] // 2, 2)
    assert np.array_equal(_bits(got), _bits(want))
    assert (_bits(got) == 0x7FC00123).sum() == 1 and (_bits(got) == np.int32(-2 ** 31)).sum() == 1


def test_copies_refuse_what_is_not_a_canvas(ctx):
    import keras_ocr_amd

    with pytest.raises(ValueError, match="not a canvas"):
        ctx.gather_tiles(np.zeros((1, 100, 96, 3), np.uint8), 64, 16)
    with pytest.raises(ValueError):
        ctx.tile_plan(100, 100, 72, 16)
    # the library's own refusal, behind the Python check
    out = np.zeros((1, 64, 64, 3), np.uint8)
    rc = ctx._lib.kocr_gather_tiles(ctx._h, keras_ocr_amd._lib._ptr(np.zeros((1, 100, 96, 3), np.uint8)), 1, 100, 96, 64, 16,  # pylint: disable=protected-access
                                    keras_ocr_amd._lib._ptr(out), 0)  # pylint: disable=protected-access
    assert rc == -1 and b"not a canvas" in ctx._lib.kocr_last_error(ctx._h)  # pylint: disable=protected-access


def test_canvas_limit_is_refused_by_name(ctx, crnn_weights):
    """A canvas side beyond 8192 ends at the post-processing's heat-map side of 4096: KOCR_EINVAL naming it, before any work"""
    import keras_ocr_amd

    pipe_for(ctx, crnn_weights, "A")
    page = np.zeros((16, 16, 3), np.uint8)
    with pytest.raises(keras_ocr_amd.KocrError, match="8192 x 8192"):
        ctx.pipeline_tiled([page], [16], [16], [16], [8200], 1024, 128)


@pytest.mark.parametrize("name", ["A", "B"])
def test_craft_forward_tiled_vs_oracle(ctx, crnn_weights, name):
    from tests.parity import heat_tolerance, heat_within_tolerance

    f = ts.fixture(name)
    pipe_for(ctx, crnn_weights, name)
    got = ctx.craft_forward_tiled(f.canvas[None], f.tile, f.overlap)[0]
    d = np.abs(got.astype(np.float64) - f.heat)
    print(f"{name}: max |gpu - oracle| {d.max():.2e}, rms {np.sqrt((d ** 2).mean()):.2e}, bounds {heat_tolerance(f.heat)}")
    assert heat_within_tolerance(got, f.heat)
    # a smaller micro-batch of tiles gives the same bits
    assert np.array_equal(_bits(ctx.craft_forward_tiled(f.canvas[None], f.tile, f.overlap, micro_batch=4)[0]), _bits(got))


def test_fused_equals_staged(ctx, crnn_weights):
    """recognize_tiled == resize_pad to the canvas -> gather_tiles -> craft_forward on the tiles -> stitch_heat -> getBoxes
    -> recognize_from_boxes on the canvas, exactly (test_fused_equals_stagewise's shape)"""
    f = ts.fixture("A")
    pipe = pipe_for(ctx, crnn_weights, "A")
    fused = pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap)
    dh, dw = f.page.shape[0] * f.scale, f.page.shape[1] * f.scale
    canvas = ctx.resize_pad(f.page[None], (dw, dh), out_hw=f.plan.canvas)
    assert np.array_equal(canvas[0], f.canvas)
    tiles = ctx.gather_tiles(canvas, f.tile, f.overlap)
    heat = ctx.stitch_heat(ctx.craft_forward(tiles), f.plan.canvas, f.tile, f.overlap)
    boxes = ctx.get_boxes(heat)
    texts = pipe.recognizer.recognize_from_boxes(canvas, boxes)
    assert len(boxes[0]) >= 4, "calibration should produce word boxes"
    assert len(fused) == 1 and [t for t, _ in fused[0]] == texts[0]
    assert np.array_equal(np.stack([b for _, b in fused[0]]), boxes[0] * np.float32(0.5))
    # Detector.detect_tiled is the same detection
    staged = pipe.detector.detect_tiled([f.canvas[:dh, :dw]], tile=f.tile, overlap=f.overlap)
    assert len(staged) == 1 and np.array_equal(staged[0], boxes[0])


def test_end_to_end_vs_statement(ctx, crnn_weights):
    """Against the statement's recognize_tiled on A and B: every oracle box that no flipped threshold pixel touches is
    reproduced to 1e-3 px with the identical string (tests/parity.py), at test_end_to_end_vs_oracle's bars"""
    from tests.parity import compare_page, flips, page_report

    report = {"boxes_equal": 0, "boxes_moved_by_flips": 0, "flipped_pixels": 0, "pixels": 0}
    for name in ("A", "B"):
        f = ts.fixture(name)
        pipe = pipe_for(ctx, crnn_weights, name)
        got = pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap)[0]
        flipped = flips(ctx.craft_forward_tiled(f.canvas[None], f.tile, f.overlap)[0], f.heat)
        if len(flipped) == 0:
            assert len(got) == len(f.want)
        assert page_report(got, f.want, flipped, f.scale)["ok"]
        compare_page(got, f.want, flipped, f.scale, f.heat.shape[:2], report)
    print("tiled e2e:", report)
    assert report["boxes_equal"] >= 4
    assert report["flipped_pixels"] <= 2


def test_page_of_one_tile_is_recognize_padded(ctx, crnn_weights):
    """A page that fits one tile takes no halo and no seam: the bits of recognize_padded at the tile's size"""
    pipe = pipe_for(ctx, crnn_weights, "A")
    page = synth.text_page(30, 50, 3, seed=21)
    got = pipe.recognize_tiled([page], tile=128, overlap=32)
    want = pipe.recognize_padded([page], 128, 128)
    assert len(want[0]) > 0
    assert [[t for t, _ in g] for g in got] == [[t for t, _ in g] for g in want]
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(got[0], want[0]))


def test_the_tail_is_shared(ctx, crnn_weights):
    """Scores, beam and the capacity protocol act on the tiled call as on kocr_pipeline: it is the same code"""
    f = ts.fixture("A")
    pipe = pipe_for(ctx, crnn_weights, "A")
    plain = pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap)[0]
    scored = pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap, return_scores=True)[0]
    assert [t for t, _, _ in scored] == [t for t, _ in plain]
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(scored, plain))
    heat = ctx.craft_forward_tiled(f.canvas[None], f.tile, f.overlap)
    boxes, det_scores = ctx.get_boxes(heat, return_scores=True)
    assert np.array_equal(np.stack([b for _, b in plain]), boxes[0] * np.float32(0.5))
    assert np.array_equal(np.array([s.detection for _, _, s in scored], np.float32), det_scores[0])
    assert all(np.isfinite(s.log_word) and 0 < s.word <= 1 for _, _, s in scored)
    beams = pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap, recognition_kwargs={"beam_width": 8, "top_paths": 2})[0]
    assert len(beams) == len(plain) and all(np.array_equal(a[1], b[1]) for a, b in zip(beams, plain))
    assert all(isinstance(alts, list) and 1 <= len(alts) <= 2 for alts, _ in beams)
    # more boxes than cap: one pass, the results fetched from HBM
    h, w = f.page.shape[:2]
    args = ([f.page], [h], [w], [h * f.scale], [w * f.scale], f.tile, f.overlap)
    big_boxes, big_labels = ctx.pipeline_tiled(*args, cap=64)
    small_boxes, small_labels = ctx.pipeline_tiled(*args, cap=2)
    assert len(big_boxes[0]) > 2
    assert np.array_equal(small_boxes[0], big_boxes[0]) and np.array_equal(small_labels, big_labels)
    assert np.array_equal(big_boxes[0] * np.float32(0.5), np.stack([b for _, b in plain]))
    res = ctx.pipeline_device_results()
    assert res["n"] == 1 and res["m"] == len(big_labels)


def test_one_gather_one_forward_one_stitch(ctx, crnn_weights):
    """The profiler rows of a tiled call: each copy once under its own name, the detector once over all 28 tiles -- and in
    micro-batches of 8 tiles four times, with the same answer"""
    f = ts.fixture("A")
    pipe = pipe_for(ctx, crnn_weights, "A")
    answers = []
    for batch_size, forwards in ((None, 1), (8, 4)):
        ctx.profile_reset()
        ctx.profile_enable(True)
        try:
            answers.append(pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap,
                                                detection_kwargs={"batch_size": batch_size} if batch_size else None)[0])
            rep = ctx.profile_report()
        finally:
            ctx.profile_enable(False)
        assert rep["tile_gather"]["launches"] == 1 and rep["heat_stitch"]["launches"] == 1 and rep["resize_pad"]["launches"] == 1
        assert rep["tile_gather"]["bytes"] == 2 * 28 * 64 * 64 * 3 and rep["heat_stitch"]["bytes"] == 2 * 80 * 128 * 2 * 4
        first = [v for k, v in rep.items() if k.startswith("conv_hs_first") or k.startswith("conv_first")]
        assert first and sum(v["launches"] for v in first) == forwards, {k: v["launches"] for k, v in rep.items()}
    assert [t for t, _ in answers[0]] == [t for t, _ in answers[1]]
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(*answers))


def test_characters_and_orientation_reach_the_tiled_call(ctx, crnn_weights):
    f = ts.fixture("A")
    pipe = pipe_for(ctx, crnn_weights, "A")
    plain = pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap)[0]
    chars = pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap, char_boxes=True)[0]
    assert [(t, b.tobytes()) for t, b, _ in chars] == [(t, b.tobytes()) for t, b in plain]
    assert all(c.boxes.shape[1:] == (4, 2) and len(c.boxes) == len(c.scores) for _, _, c in chars)
    turned = pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap, recognition_kwargs={"orientation": "flip"})[0]
    assert len(turned) == len(plain)
    for (_, quad), (_, box) in zip(turned, plain):  # the same corners, renamed
        assert sorted(map(tuple, np.asarray(quad).tolist())) == sorted(map(tuple, np.asarray(box).tolist()))
    with pytest.raises(ValueError):
        pipe.recognize_tiled([f.page], tile=f.tile, overlap=f.overlap, recognition_kwargs={"orientation": "flip", "beam_width": 4})


def test_blank_page_and_refusals(ctx, crnn_weights):
    """An all-zero page gives [] -- with the head's biases shifted so that the blank canvas (black page, tools.pad's white
    around it) peaks at 0.2, as test_blank_image_has_no_predictions does for the whole-page path; what recognize_tiled refuses"""
    import keras_ocr_amd

    f = ts.fixture("A")
    black = np.zeros((100, 150, 3), np.uint8)
    heat, _ = ts.tiled_heat(f.weights, ts.resize(black, 2), 128, 32)
    assert heat.max() > 0.4  # without the shift the black-on-white edge would be text
    w = dict(f.weights)
    w["conv_cls.8.bias"] = (w["conv_cls.8.bias"] - np.maximum(heat.reshape(-1, 2).max(0) - 0.2, 0)).astype(np.float32)
    pipe = pipe_for(ctx, crnn_weights, "A-blank", weights=w)
    assert pipe.recognize_tiled([black], tile=128, overlap=32) == [[]]
    assert pipe.recognize_tiled([black], tile=128, overlap=32, return_scores=True) == [[]]
    assert pipe.recognize_tiled([]) == []
    with pytest.raises(NotImplementedError):
        pipe.recognize_tiled([black.astype(np.float32)], tile=128, overlap=32)
    with pytest.raises(NotImplementedError):
        pipe.detector.detect_tiled([black.astype(np.float32)], tile=128, overlap=32)
    with pytest.raises(ValueError):
        pipe.recognize_tiled([black], tile=72, overlap=16)
    with pytest.raises(ValueError):
        pipe.recognize_tiled([black], tile=128)  # the default overlap of 128 leaves no stride

    class Rec:  # not on the pipeline's context
        alphabet = pipe.recognizer.alphabet

        def recognize_from_boxes(self, images, box_groups, **kw):
            return pipe.recognizer.recognize_from_boxes(images, box_groups, **kw)

    foreign = keras_ocr_amd.pipeline.Pipeline(detector=pipe.detector, recognizer=Rec())
    with pytest.raises(TypeError, match="recognizer"):
        foreign.recognize_tiled([black], tile=128, overlap=32)
