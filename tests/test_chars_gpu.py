"""GPU suite: the character boxes of word boxes read off the region map on the device (kocr_char_boxes and the resident path of
kocr_set_char_boxes) against their float64 statement (tests/chars_statement.py): the counts equal, quads and scores bit for bit."""
import ctypes

import numpy as np
import pytest

from tests import chars_cases as cc
from tests import chars_statement as cs
from tests import stream_gate as sg
from tests import synth

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32


def _flat(groups):
    """Context.char_boxes' nested result -> (counts, quads, scores) in word order"""
    words = [word for page in groups for word in page]
    counts = np.array([len(q) for q, _ in words], I32)
    quads = np.concatenate([np.zeros((0, 4, 2), F32)] + [q for q, _ in words])
    scores = np.concatenate([np.zeros(0, F32)] + [s for _, s in words])
    return counts, quads, scores


def _assert_same(got, want, what):
    """(char_counts, char_quads, char_scores) of the device against the statement's"""
    assert got[0].dtype == np.int32 and got[0].shape == want[0].shape, (what, got[0].shape, want[0].shape)
    different = np.flatnonzero(got[0] != want[0])
    assert different.size == 0, (what, "char_counts", different[:5], got[0][different[:5]], want[0][different[:5]])
    for name, g, w, width in (("char_quads", got[1], want[1], 8), ("char_scores", got[2], want[2], 1)):
        assert g.dtype == np.float32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        different = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(-1, width).any(axis=1))
        assert different.size == 0, (what, name, different[:5], g[different[:5]], w[different[:5]])


def _same_groups(a, b):
    return [len(p) for p in a] == [len(p) for p in b] and sg.same_bits(list(_flat(a)), list(_flat(b)))


@pytest.fixture(scope="module")
def batch():
    """the ragged batch and the statement's answer, computed once"""
    heat, pages, inside = cc.batch()
    return heat, pages, inside, cs.char_batch(heat, pages)


def test_batch_equals_the_statement(ctx, batch):
    heat, pages, inside, want = batch
    assert [len(p) for p in pages] == list(cc.BATCH_WORDS) and 0 in cc.BATCH_WORDS
    got = ctx.char_boxes(heat, pages)
    assert [len(p) for p in got] == list(cc.BATCH_WORDS)
    _assert_same(_flat(got), want, "batch")
    assert want[0].sum() >= inside >= 15 and len(want[1]) == want[0].sum()
    # another rule, away from every default
    rule = {"peak_threshold": 0.6, "valley_ratio": 0.9, "extent_threshold": 0.05}
    _assert_same(_flat(ctx.char_boxes(heat, pages, **rule)), cs.char_batch(heat, pages, **rule), str(rule))


def test_wide_and_tall_words_equal_the_statement(ctx):
    for make in (cc.wide_word, cc.tall_word):
        text_map, quad, n = make()
        heat = np.zeros((1,) + text_map.shape + (2,), F32)
        heat[0, :, :, 0] = text_map
        want = cs.char_batch(heat, [quad[None]])
        assert want[0].tolist() == [n]
        _assert_same(_flat(ctx.char_boxes(heat, [quad[None]])), want, make.__name__)


def test_hand_made_cases(ctx):
    heat, pages = cc.exact_batch()
    cases = cc.hand_made()
    got = ctx.char_boxes(heat, pages, **cc.EXACT_RULE)
    _assert_same(_flat(got), cs.char_batch(heat, pages, **cc.EXACT_RULE), "hand-made cases")
    # and the answers known by hand
    for (name, _, quad, _, bounds, peaks), page in zip(cases, got):
        boxes, scores = page[0]
        assert len(boxes) == len(scores) == len(peaks), name
        for k in range(len(peaks)):
            left, right = quad[0, 0] + 2 * bounds[k], quad[0, 0] + 2 * bounds[k + 1]
            assert boxes[k].tolist() == [[left, quad[0, 1]], [right, quad[0, 1]], [right, quad[3, 1]], [left, quad[3, 1]]], name


def test_batch_independence(ctx, batch):
    """every page alone: the same counts and the same bits as inside the batch"""
    heat, pages, _, _ = batch
    together = ctx.char_boxes(heat, pages)
    for k, page in enumerate(pages):
        alone = ctx.char_boxes(heat[k:k + 1], [page])
        _assert_same(_flat(alone), _flat(together[k:k + 1]), f"page {k} of {len(page)} words alone")


@pytest.fixture(scope="module")
def many_words():
    """the batch of 1069 words and the statement's answer under EXACT_RULE, computed once"""
    heat, pages, fullest = cc.many_words_batch()
    return heat, pages, fullest, cs.char_batch(heat, pages, **cc.EXACT_RULE)


def test_many_words_equal_the_statement(ctx, many_words):
    """five blocks of chars_pack_kernel, one of them without characters, and a word of 256 characters behind it"""
    heat, pages, fullest, want = many_words
    got = ctx.char_boxes(heat, pages, **cc.EXACT_RULE)
    assert [len(p) for p in got] == list(cc.MANY_WORDS)
    _assert_same(_flat(got), want, "many words")
    assert want[0][fullest] == 256 and not want[0][cc.DEAD_WORDS[0]:cc.DEAD_WORDS[1]].any()


def test_many_words_batch_independence(ctx, many_words):
    """every page alone equals its slice of the batch, and so does the fullest word as a batch of one"""
    heat, pages, fullest, want = many_words
    together = ctx.char_boxes(heat, pages, **cc.EXACT_RULE)
    for k, page in enumerate(pages):
        alone = ctx.char_boxes(heat[k:k + 1], [page], **cc.EXACT_RULE)
        _assert_same(_flat(alone), _flat(together[k:k + 1]), f"page {k} of {len(page)} words alone")
    last = len(pages) - 1
    assert fullest == sum(len(p) for p in pages[:last])
    one = ctx.char_boxes(heat[last:], [pages[last][:1]], **cc.EXACT_RULE)
    _assert_same(_flat(one), _flat([together[last][:1]]), "the fullest word alone")
    before = int(want[0][:fullest].sum())
    _assert_same(_flat(one), (want[0][fullest:fullest + 1], want[1][before:before + 256], want[2][before:before + 256]), "the fullest word against the statement")
    assert len(one[0][0][0]) == 256


def _raw(lib, ctx, heat, n, quads, offsets, cap, boxes=True, rule=(0.4, 0.7, 0.2), on_device=0, flags=0, d_heat=None):
    from keras_ocr_amd import _lib

    total = len(quads)
    out = (np.full(max(total, 1), -7, I32), np.full((max(cap, 1), 4, 2), -7, F32), np.full(max(cap, 1), -7, F32))
    chars = ctypes.c_int64(-1)
    h, w = heat.shape[1:3]
    rc = lib.kocr_char_boxes(ctx._h, _lib._ptr(heat if d_heat is None else d_heat), n, h, w, _lib._ptr(quads), _lib._ptr(offsets), *rule,  # pylint: disable=protected-access
                             _lib._ptr(out[0]), _lib._ptr(out[1]) if boxes else None, _lib._ptr(out[2]) if boxes else None,  # pylint: disable=protected-access
                             cap if boxes else 0, ctypes.byref(chars), on_device, flags)
    return rc, chars.value, out, lib.kocr_last_error(ctx._h)  # pylint: disable=protected-access


def test_raw_abi(ctx, batch):
    import keras_ocr_amd
    from keras_ocr_amd import _lib

    lib = keras_ocr_amd.load_library()
    heat, pages, _, want = batch
    quads = np.ascontiguousarray(np.concatenate(pages))
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pages])]).astype(I32)
    n, total, chars = len(pages), len(quads), int(want[0].sum())
    rc, true_chars, out, message = _raw(lib, ctx, heat, n, quads, offsets, chars - 1)
    assert rc == _lib.KOCR_ECAPACITY and true_chars == chars and f"{chars} characters".encode() in message
    assert np.array_equal(out[0], want[0])  # the counts are complete
    rc, true_chars, out, _ = _raw(lib, ctx, heat, n, quads, offsets, chars)
    assert rc == 0 and true_chars == chars
    _assert_same((out[0], out[1][:chars], out[2][:chars]), want, "raw call")
    rc, true_chars, out, _ = _raw(lib, ctx, heat, n, quads, offsets, 0, boxes=False)  # char_quads == NULL
    assert rc == 0 and true_chars == chars and np.array_equal(out[0], want[0]) and (out[1] == -7).all() and (out[2] == -7).all()
    # the heat-maps behind a device pointer
    d_heat = ctypes.c_void_p()
    assert lib.kocr_device_alloc(ctx._h, ctypes.byref(d_heat), heat.nbytes) == 0  # pylint: disable=protected-access
    try:
        assert lib.kocr_memcpy_h2d(ctx._h, d_heat, _lib._ptr(heat), heat.nbytes) == 0  # pylint: disable=protected-access
        rc, true_chars, out, _ = _raw(lib, ctx, heat, n, quads, offsets, chars, on_device=1, d_heat=d_heat.value)
        assert rc == 0 and true_chars == chars
        _assert_same((out[0], out[1][:chars], out[2][:chars]), want, "device heat-maps")
    finally:
        assert lib.kocr_device_free(ctx._h, d_heat) == 0  # pylint: disable=protected-access
    # refusals, each with its message
    bad_offsets = offsets.copy()
    bad_offsets[0] = 1
    rc, _, _, message = _raw(lib, ctx, heat, n, quads, bad_offsets, 8)
    assert rc == _lib.KOCR_EINVAL and b"offsets must start at 0" in message
    bad_offsets = offsets.copy()
    bad_offsets[2] = 3
    rc, _, _, message = _raw(lib, ctx, heat, n, quads, bad_offsets, 8)
    assert rc == _lib.KOCR_EINVAL and b"offsets decreases at entry 2" in message
    for value in (np.nan, np.inf):
        bad = quads.copy()
        bad[offsets[2] + 3, 2, 1] = value
        rc, _, _, message = _raw(lib, ctx, heat, n, bad, offsets, 8)
        assert rc == _lib.KOCR_EINVAL and b"page 2, word 3: non-finite coordinate" in message
    with pytest.raises(ValueError, match="page 2, word 3"):
        groups = [p.copy() for p in pages]
        groups[2][3, 2, 1] = np.nan
        ctx.char_boxes(heat, groups)
    for rule, name in (((0.0, 0.7, 0.0), b"peak_threshold"), ((np.inf, 0.7, 0.2), b"peak_threshold"), ((np.nan, 0.7, 0.2), b"peak_threshold"),
                       ((0.4, -0.1, 0.2), b"valley_ratio"), ((0.4, 1.1, 0.2), b"valley_ratio"), ((0.4, np.nan, 0.2), b"valley_ratio"),
                       ((0.4, 0.7, -0.1), b"extent_threshold"), ((0.4, 0.7, 0.5), b"extent_threshold"), ((0.4, 0.7, np.nan), b"extent_threshold")):
        rc, _, _, message = _raw(lib, ctx, heat, n, quads, offsets, 8, rule=rule)
        assert rc == _lib.KOCR_EINVAL and name in message, (rule, message)
    for rule in ({"peak_threshold": -1.0}, {"valley_ratio": 2.0}, {"extent_threshold": 0.9}):
        with pytest.raises(ValueError, match=next(iter(rule))):
            ctx.char_boxes(heat, pages, **rule)
    rc, _, _, message = _raw(lib, ctx, heat, n, quads, offsets, 8, flags=1)
    assert rc == _lib.KOCR_EINVAL and b"flags must be 0" in message
    # N = 0 and a batch of pages without words
    none = np.zeros((0, 4, 2), F32)
    rc, true_chars, _, _ = _raw(lib, ctx, heat[:0], 0, none, np.array([0], I32), 0)
    assert rc == 0 and true_chars == 0
    rc, true_chars, _, _ = _raw(lib, ctx, heat[:3], 3, none, np.array([0, 0, 0, 0], I32), 4)
    assert rc == 0 and true_chars == 0
    assert ctx.char_boxes(heat[:2], [none, np.array([])]) == [[], []] and ctx.char_boxes(heat[:0], []) == []
    # the call after all of that is unharmed
    _assert_same(_flat(ctx.char_boxes(heat, pages)), want, "after the refusals")


def test_on_a_caller_stream(ctx, batch):
    """on a stream handed over with kocr_set_stream, behind long-running work queued there, the call gives the arrays it
    gives on the context's own stream, complete on return"""
    import torch
    import keras_ocr_amd

    lib = keras_ocr_amd.load_library()
    heat, pages, _, want = batch
    quads = np.ascontiguousarray(np.concatenate(pages))
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pages])]).astype(I32)
    total, chars = len(quads), int(want[0].sum())
    poison = heat[::-1].copy()
    case = sg.Case("kocr_char_boxes", [sg.In(heat, poison), len(pages), heat.shape[1], heat.shape[2], quads, offsets, 0.4, 0.7, 0.2,
                                       sg.Out(total, I32), sg.Out((chars + 64, 4, 2), F32), sg.Out(chars + 64, F32), chars + 64,
                                       np.zeros(1, np.int64), 0, 0], False, view=lambda outs: [outs[0], outs[1][:chars], outs[2][:chars]],
                   flag=False)
    stream = torch.cuda.Stream()
    try:
        ctx.set_stream(None)
        rc, outs, _ = sg.host_call(lib, ctx, case)
        assert rc == 0
        expected = case.view(outs)
        _assert_same(expected, want, "own stream")
        rc, outs, _ = sg.host_call(lib, ctx, case, "poison")
        assert rc in (0, keras_ocr_amd._lib.KOCR_ECAPACITY) and not np.array_equal(outs[0], expected[0])  # pylint: disable=protected-access
        ctx.set_stream(stream.cuda_stream)
        rc, outs, _ = sg.host_call(lib, ctx, case)
        assert rc == 0 and sg.same_bits(case.view(outs), expected)
        sg.host_call(lib, ctx, case, "poison")  # what the arenas hold before the gated call is not its answer
        g = sg.gated_call(lib, ctx, case, stream, sg.Gate(), on_device=0)
        assert g.rc == 0 and sg.same_bits(case.view(g.outs), expected), "the host outputs were not complete and correct on return"
        assert g.gate_ms > 10 * g.call_ms or g.gate_ms > 50, (g.gate_ms, g.call_ms)
    finally:
        ctx.set_stream(None)


# ---- the resident path ------------------------------------------------------------------------------------------------------

def test_get_boxes_leaves_the_characters_resident(ctx):
    heat = synth.heatmap_batch()
    plain = ctx.get_boxes(heat)
    boxes, chars = ctx.get_boxes(heat, char_boxes=True)
    assert ctx.get_char_boxes() == (False, cs.DEFAULTS)
    assert len(boxes) == len(plain) and all(a.tobytes() == b.tobytes() and a.shape == b.shape for a, b in zip(boxes, plain))
    want = ctx.char_boxes(heat, boxes)
    assert _same_groups(chars, want)
    assert [len(p) for p in chars] == [len(b) for b in boxes] and max(len(q) for p in chars for q, _ in p) >= 2
    _assert_same(_flat(chars), cs.char_batch(heat, boxes), "get_boxes")
    # with the scores, with rule parameters, and with a cap that has to grow
    rule = {"valley_ratio": 0.95, "peak_threshold": 0.3}
    b2, scores, c2 = ctx.get_boxes(heat, return_scores=True, char_boxes=rule, cap=1)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(b2, plain)) and len(scores) == len(plain)
    assert _same_groups(c2, ctx.char_boxes(heat, boxes, **rule)) and not _same_groups(c2, chars)
    assert ctx.get_char_boxes() == (False, cs.DEFAULTS)
    with pytest.raises(ValueError, match="valley_ratio"):
        ctx.get_boxes(heat, char_boxes={"valley_ratio": 3})
    with pytest.raises(TypeError, match="max_gap"):
        ctx.get_boxes(heat, char_boxes={"max_gap": 3})


def test_fetching_what_is_not_there():
    import keras_ocr_amd

    heat = synth.heatmap_batch()
    context = keras_ocr_amd.Context(0)
    try:
        with pytest.raises(ValueError, match="no character boxes are resident"):
            context.detection_char_boxes([0], 4)
        boxes, _ = context.get_boxes(heat, char_boxes=True)
        counts = [len(b) for b in boxes]
        assert len(context.detection_char_boxes(counts, 1024)) == len(boxes)  # a second fetch is allowed
        context.get_boxes(heat)
        with pytest.raises(ValueError, match="produced with character boxes off"):
            context.detection_char_boxes(counts, 1024)
        context.get_boxes(heat, char_boxes=True)
        context.char_boxes(heat, boxes)  # a call that processes images ends the validity
        with pytest.raises(ValueError, match="no character boxes are resident"):
            context.detection_char_boxes(counts, 1024)
    finally:
        context.close()


@pytest.fixture(scope="module")
def pipe(craft_weights, crnn_weights):
    """the pipeline of tests/test_scores_gpu.py: the detector's head calibrated on the first of its two small pages"""
    import keras_ocr_amd
    from oracle import craft as ocraft, tools as otools

    page = synth.text_page(96, 128, 5, seed=21)[None]
    big = np.stack([otools.resize_image(p, 2, 2048)[0] for p in page])
    calibrated = keras_ocr_amd.weights.calibrate_craft_head(craft_weights, ocraft.detector_predict(craft_weights, big), text_frac=0.10,
                                                            link_frac=0.04)
    c = keras_ocr_amd.Context(0)
    det = keras_ocr_amd.detection.Detector(weights=calibrated, ctx=c)
    rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=c)
    yield keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)
    c.close()


def _pages():
    return [synth.text_page(h, w, n, seed=s) for h, w, n, s in [(96, 128, 5, 21), (80, 100, 4, 22)]]


def _padded(pages):
    from oracle import tools as otools

    resized = [otools.resize_image(p, 2, 2048)[0] for p in pages]
    hmax, wmax = max(r.shape[0] for r in resized), max(r.shape[1] for r in resized)
    return np.stack([otools.pad(r, width=wmax, height=hmax) for r in resized])


def _pipeline_args(pipe, pages):
    _, dhs, dws, hmax, wmax = pipe._plan([p.shape for p in pages])  # pylint: disable=protected-access
    return ([np.ascontiguousarray(p) for p in pages], [p.shape[0] for p in pages], [p.shape[1] for p in pages], dhs, dws, hmax, wmax)


def test_detect_and_pipeline_leave_the_characters_resident(pipe):
    ctx = pipe.detector._ctx  # pylint: disable=protected-access
    pages = _pages()
    batch = _padded(pages)
    heat = ctx.craft_forward(batch)
    plain = ctx.detect(batch)
    boxes, chars = ctx.detect(batch, char_boxes=True)
    assert sum(len(b) for b in boxes) >= 4 and all(a.tobytes() == b.tobytes() for a, b in zip(boxes, plain))
    want = ctx.char_boxes(heat, boxes)
    assert _same_groups(chars, want) and [len(p) for p in chars] == [len(b) for b in boxes]
    _assert_same(_flat(chars), cs.char_batch(heat, boxes), "detect")
    # the fused pipeline: the same heat-maps, the same boxes, the same characters
    args = _pipeline_args(pipe, pages)
    p_boxes, p_labels = ctx.pipeline(*args)
    c_boxes, c_labels, c_chars = ctx.pipeline(*args, char_boxes=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(c_boxes, p_boxes)) and np.array_equal(c_labels, p_labels)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(c_boxes, boxes))
    assert _same_groups(c_chars, want)
    # cap = 1, max_crops = 1: the post-processing runs again on the resident heat-maps, KOCR_ECAPACITY, everything is fetched
    assert max(len(b) for b in boxes) > 1
    o_boxes, o_labels, o_scores, o_chars = ctx.pipeline(*args, cap=1, max_crops=1, return_scores=True, char_boxes=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(o_boxes, p_boxes)) and np.array_equal(o_labels, p_labels)
    assert len(o_scores) == 3 and _same_groups(o_chars, want)
    # with the switch off again nothing is resident
    ctx.pipeline(*args)
    with pytest.raises(ValueError, match="produced with character boxes off"):
        ctx.detection_char_boxes([len(b) for b in boxes], 256)


def test_switch_off_launches_nothing_new(pipe):
    ctx = pipe.detector._ctx  # pylint: disable=protected-access
    pages = _pages()
    batch, args, heat = _padded(pages), _pipeline_args(pipe, pages), synth.heatmap_batch()
    ctx.profile_enable(True)
    try:
        ctx.profile_reset()
        off = (ctx.get_boxes(heat), ctx.detect(batch), ctx.pipeline(*args))
        rows = ctx.profile_report()
        assert rows and not [name for name in rows if name.startswith("chars_")], sorted(rows)
        ctx.profile_reset()
        on = (ctx.get_boxes(heat, char_boxes=True), ctx.detect(batch, char_boxes=True), ctx.pipeline(*args, char_boxes=True))
        rows = ctx.profile_report()
        assert rows["chars_split"]["launches"] == 3 and rows["chars_pack"]["launches"] == 3
    finally:
        ctx.profile_enable(False)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off[0], on[0][0]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off[1], on[1][0]))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(off[2][0], on[2][0])) and off[2][1].tobytes() == on[2][1].tobytes()
    assert [len(b) for b in off[2][0]] == [len(b) for b in on[2][0]]


# ---- the Python surface -----------------------------------------------------------------------------------------------------

def _inside(word, boxes):
    """every corner of every character lies on the word's top edge (tl, tr) or bottom edge (bl, br), between its ends, within
    a few float32 ulps of the coordinates' size: the corners are interpolated in float64 and rounded once, then scaled"""
    word, boxes = np.asarray(word, np.float64), np.asarray(boxes, np.float64)
    slack = 8 * np.finfo(np.float32).eps * max(1.0, np.abs(word).max())
    for box in boxes:
        for corner, (a, b) in zip(box, ((word[0], word[1]), (word[0], word[1]), (word[3], word[2]), (word[3], word[2]))):
            edge = b - a
            length = np.sqrt((edge * edge).sum())
            t = ((corner - a) * edge).sum() / length
            d = abs((corner[0] - a[0]) * edge[1] - (corner[1] - a[1]) * edge[0]) / length
            if not (-slack <= t <= length + slack and d <= slack):
                return False
    return True


def test_recognize_characters(pipe):
    import keras_ocr_amd
    from keras_ocr_amd import detection, layout, tools

    ctx = pipe.detector._ctx  # pylint: disable=protected-access
    pages = _pages()
    plain = pipe.recognize(pages)
    got = pipe.recognize_characters(pages)
    assert ctx.get_char_boxes()[0] is False and sum(len(g) for g in plain) >= 4
    assert [[(t, b.tobytes()) for t, b in g] for g in plain] == [[(t, b.tobytes()) for t, b, _ in g] for g in got]
    # the resident characters of the same pipeline call, through adjust_boxes
    args = _pipeline_args(pipe, pages)
    scales = pipe._plan([p.shape for p in pages])[0]  # pylint: disable=protected-access
    _, _, resident = ctx.pipeline(*args, char_boxes=True)
    assert sum(len(c.boxes) for g in got for _, _, c in g) > 0
    for group, chars, scale in zip(got, resident, scales):
        assert len(group) == len(chars)
        for (_, box, characters), (quads, scores) in zip(group, chars):
            assert isinstance(characters, layout.Characters) and characters.boxes.dtype == characters.scores.dtype == np.float32
            assert characters.boxes.shape == (len(scores), 4, 2)
            assert characters.boxes.tobytes() == np.asarray(tools.adjust_boxes(boxes=quads, boxes_format="boxes", scale=1 / scale), F32).tobytes()
            assert characters.scores.tobytes() == scores.tobytes()
            assert _inside(box, characters.boxes)
    # rule parameters reach the kernel
    loose = pipe.recognize_characters(pages, valley_ratio=1.0, peak_threshold=0.05, extent_threshold=0.0)
    assert [[(t, b.tobytes()) for t, b, _ in g] for g in loose] == [[(t, b.tobytes()) for t, b, _ in g] for g in got]
    assert [len(c.boxes) for g in loose for _, _, c in g] != [len(c.boxes) for g in got for _, _, c in g]
    assert pipe.recognize_characters([]) == []
    with pytest.raises(ValueError, match="beam_width"):
        pipe.recognize_characters(pages[:1], recognition_kwargs={"beam_width": 4})
    with pytest.raises(ValueError, match="lexicon_top"):
        pipe.recognize_characters(pages[:1], recognition_kwargs={"lexicon_top": 2})
    with pytest.raises(TypeError, match="max_gap"):
        pipe.recognize_characters(pages[:1], max_gap=1.0)
    with pytest.raises(ValueError, match="valley_ratio"):
        pipe.recognize_characters(pages[:1], valley_ratio=-1.0)

    class Duck:
        def detect(self, images, **kwargs):
            return pipe.detector.detect(images, **kwargs)

    with pytest.raises(TypeError, match="Duck.detect.*cannot give character boxes"):
        keras_ocr_amd.pipeline.Pipeline(detector=Duck(), recognizer=pipe.recognizer).recognize_characters(pages[:1])
    # the stage-wise path (float images): detector.detect(char_boxes=...), texts and boxes those of recognize() on that path
    floats = [p.astype(np.float32) for p in pages[:1]]
    staged, staged_plain = pipe.recognize_characters(floats), pipe.recognize(floats)
    assert [[(t, b.tobytes()) for t, b in g] for g in staged_plain] == [[(t, b.tobytes()) for t, b, _ in g] for g in staged]
    assert all(isinstance(c, layout.Characters) and _inside(b, c.boxes) for g in staged for _, b, c in g)
    # Detector.detect and detection.get_char_boxes agree
    batch = _padded(pages)
    boxes, groups = pipe.detector.detect(batch, char_boxes=True)
    again = detection.get_char_boxes(ctx.craft_forward(batch), boxes, ctx=ctx)
    assert [[(c.boxes.tobytes(), c.scores.tobytes()) for c in g] for g in groups] == [[(c.boxes.tobytes(), c.scores.tobytes()) for c in g] for g in again]
    assert all(isinstance(c, layout.Characters) for g in groups for c in g) and [len(g) for g in groups] == [len(b) for b in boxes]
    b3, s3, g3 = pipe.detector.detect(batch, return_scores=True, char_boxes={"valley_ratio": 0.7})
    assert len(s3) == len(b3) == len(g3) and [[c.boxes.tobytes() for c in g] for g in g3] == [[c.boxes.tobytes() for c in g] for g in groups]
    assert pipe.detector.detect([], char_boxes=True) == ([], [])
