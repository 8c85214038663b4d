"""Long words on the GPU ("Long words"; include/kocr_windows.h) against tests/windows_statement.py.

  1. plan          Context.window_plan == the statement's K, quads and frame ranges, bit for bit;
  2. crops         every window crop == the oracle's warp of its ordered sub-quad (as tests/orientation_statement.py checks
                   turned quads); a box that is not long == Context.warp_crops' crop, bit for bit;
  3. stitch-decode Context.ctc_stitch_decode on chosen and on random logits == the statement: labels and frame counts exact,
                   character scores within the float32 softmax's own rounding, log_word within the project's CTC gate
                   GATE * T' * max(1, -statement), GATE = 1e-6 (tests/test_scores_gpu.py);
  4. whole route   K = 1 words == recognize_boxes(return_scores=True), K > 1 words == ctc_stitch_decode on the recogniser's own
                   logits for the windowed crops, both bit for bit; permutations; other boxes' pixels;
  5. batch edge    1040 windows in one call == the same boxes in two calls;
  6. refusals, the Python surface, resident results.
Character scores: the GPU's value is 1 / s with s the float32 sum of C terms e^(x - max), each within 2 ulp; the statement's is
the float64 softmax.  |difference| <= (C + 8) * 2^-24, the bound tests/crnn_layer_check.py states for a C-class softmax."""
import numpy as np
import pytest

from tests import windows_cases as wc
from tests import windows_statement as ws

pytestmark = pytest.mark.gpu

GATE = 1e-6
U = 2.0 ** -24
T = 50


def _sharpened(weights):
    w = dict(weights)
    w["fc_12/kernel"] = w["fc_12/kernel"] * np.float32(2)
    w["fc_12/bias"] = w["fc_12/bias"] * np.float32(2)
    return w


def _switches_off(c):
    c.set_scores(False)
    c.set_beam(0)
    c.set_lexicon_match(0)
    c.set_orientation(0)
    c.set_char_boxes(False)
    if c.charset_count():
        c.set_charset(-1)
    if c.pattern_count():
        c.set_pattern(-1)


@pytest.fixture(scope="module")
def wctx(crnn_weights):
    """a context of its own with the default build, fc_12 doubled as tests/test_orientation_gpu.py sharpens it"""
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    c.load_crnn(_sharpened(crnn_weights))
    assert c.crnn_classes() == 37 and c.crnn_label_width() == 48
    yield c
    c.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _same_rows(got, want, what=""):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, what
        assert np.array_equal(_bits(g), _bits(w)), what


# ---- 1. the plan -----------------------------------------------------------------------------------------------------
PLAN_SET = np.concatenate([wc.PLAN_BOXES, wc.long_box(20)[None], wc.rotated(900, 700, 1661, 8, 30)[None]])


@pytest.mark.parametrize("aspect, overlap", [(10.0, 40), (200 / 31, 16), (12.5, 96), (10.0, 96)])
def test_plan_equals_the_statement(wctx, aspect, overlap):
    for discard in wc.DISCARDS:
        wctx.crnn_set_rnn_steps_to_discard(discard)
        try:
            want_k, want_q, want_r, _ = ws.plan_boxes(PLAN_SET, aspect, overlap, discard)
            k, quads, ranges = wctx.window_plan(PLAN_SET, aspect, overlap)
        finally:
            wctx.crnn_set_rnn_steps_to_discard(2)
        assert k.tolist() == want_k.tolist()
        assert ranges.tolist() == want_r.tolist()
        assert np.array_equal(_bits(quads), _bits(want_q))
    if (aspect, overlap) == (10.0, 40):
        assert {1, 2, 3, 4, 40} <= set(want_k.tolist())
    assert (want_k == 1).sum() >= (2 if aspect >= 10 else 1) and (want_k > 1).sum() >= 5


def test_plan_edges(wctx):
    with pytest.raises(ZeroDivisionError):
        wctx.window_plan(np.stack([wc.PLAN_BOXES[3], wc.rect(5, 5, 300, 0.4)]))
    k, quads, ranges = wctx.window_plan(np.zeros((0, 4, 2), np.float32))
    assert k.shape == (0,) and quads.shape == (0, 4, 2) and ranges.shape == (0, 2)
    # one box alone and many: the scan over more boxes than one workgroup's lanes
    many = np.concatenate([wc.PLAN_BOXES] * 30)
    want = ws.plan_boxes(many)
    got = wctx.window_plan(many)
    assert got[0].tolist() == want[0].tolist() and np.array_equal(_bits(got[1]), _bits(want[1])) and got[2].tolist() == want[2].tolist()


# ---- 2. the crops ----------------------------------------------------------------------------------------------------
def test_crops_equal_the_oracle_warp_of_their_quads(wctx):
    page, other = wc.page(), np.ascontiguousarray(wc.page()[::-1])
    groups = [wc.PLAN_BOXES[:6], wc.PLAN_BOXES[6:]]
    crops, k, quads, ranges = wctx.warp_crops_windowed(np.stack([page, other]), groups, 10.0, 40)
    want_k, want_q, want_r, _ = ws.plan_boxes(wc.PLAN_BOXES)
    assert k.tolist() == want_k.tolist() and np.array_equal(_bits(quads), _bits(want_q)) and ranges.tolist() == want_r.tolist()
    n0 = int(want_k[:6].sum())
    want = np.concatenate([ws.crops(page, want_q[:n0]), ws.crops(other, want_q[n0:])])
    assert np.array_equal(crops, want)
    assert crops.reshape(len(crops), -1).max(1).min() > 0  # no empty crop
    # a box that is not long: warp_crops' crop
    plain = wctx.warp_crops(np.stack([page, other]), groups)
    off = np.concatenate([[0], np.cumsum(want_k)])
    short = [m for m in range(len(want_k)) if want_k[m] == 1]
    assert len(short) >= 2
    for m in short:
        assert np.array_equal(crops[off[m]], plain[m])
    # the last window of a long box is narrower: zero columns on the right
    m = int(np.argmax(want_k > 1))
    assert (crops[off[m + 1] - 1][:, -8:] == 0).all()
    empty = wctx.warp_crops_windowed(page[None], [np.zeros((0, 4, 2), np.float32)])
    assert [a.shape for a in empty] == [(0, 31, 200), (0,), (0, 4, 2), (0, 2)]


# ---- 3. stitch and decode on chosen logits ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[(37, 0), (37, 2), (37, 5), (96, 2)], ids=lambda p: f"C{p[0]}-d{p[1]}")
def built(request, crnn_weights):
    """(context, classes, discard) with the recogniser built through Recognizer(build_params=...)"""
    import keras_ocr_amd
    from keras_ocr_amd.recognition import DEFAULT_ALPHABET, DEFAULT_BUILD_PARAMS

    classes, discard = request.param
    c = keras_ocr_amd.Context(0)
    w = crnn_weights if classes == 37 else keras_ocr_amd.weights.synthetic_crnn_weights(4321, n_classes=classes)
    alphabet = DEFAULT_ALPHABET if classes == 37 else "".join(chr(200 + i) for i in range(classes - 1))
    rec = keras_ocr_amd.recognition.Recognizer(alphabet=alphabet, weights=dict(w), ctx=c,
                                               build_params=dict(DEFAULT_BUILD_PARAMS, rnn_steps_to_discard=discard))
    assert c.crnn_label_width() == 50 - discard
    yield c, classes, discard, rec
    c.close()


def _check_stitch_decode(c, logits, counts, overlap, discard, what, expect=None):
    labels, log_word, chars, frames = c.ctc_stitch_decode(logits, counts, overlap)
    stmt = ws.stitch_decode(logits, counts, overlap, discard)
    classes = logits.shape[2]
    width = max(s[3] for s in stmt)
    assert labels.shape == chars.shape == (len(counts), width) and labels.dtype == np.int32 and chars.dtype == np.float32
    assert frames.tolist() == [s[3] for s in stmt]
    worst = 0.0
    for m, (want_l, want_c, want_w, n, _) in enumerate(stmt):
        got_l = labels[m][labels[m] >= 0].tolist()
        assert got_l == want_l and (labels[m, len(want_l):] == -1).all(), (what, m)
        if expect is not None:
            assert got_l == expect[m], (what, m)
        assert (chars[m, len(want_l):] == 0).all(), (what, m)
        assert np.abs(chars[m, :len(want_l)].astype(np.float64) - want_c).max(initial=0.0) <= (classes + 8) * U, (what, m)
        gate = GATE * n * max(1.0, -want_w)
        err = abs(float(log_word[m]) - want_w)
        worst = max(worst, err / gate)
        assert err <= gate, (what, m, err, gate)
    print(f"\n{what}: max |log_word - statement| / gate = {worst:.3g}")
    return labels, log_word, chars, frames


@pytest.mark.parametrize("overlap", [16, 96])
def test_stitch_decode_on_chosen_logits(built, overlap):
    c, classes, discard, _ = built
    logits, counts, expect = wc.chosen_logits(classes, overlap, discard)
    assert sorted(set(counts.tolist())) == [1, 2, 3]
    _check_stitch_decode(c, logits, counts, overlap, discard, f"chosen C={classes} d={discard} O={overlap}", expect)


def test_stitch_decode_on_random_logits(built):
    """ragged words of 1 to 41 windows (41 windows at overlap 40: 1648 frames), more words than one wave's lanes of work"""
    c, classes, discard, _ = built
    rng = np.random.default_rng(classes + discard)
    counts = np.array([1, 41, 2, 1, 3, 7, 1, 2], np.int32)
    logits = wc.random_logits(rng, int(counts.sum()), classes)
    labels, log_word, chars, frames = _check_stitch_decode(c, logits, counts, 40, discard, f"random C={classes} d={discard}")
    assert frames.max() == 40 * 40 + 50 - discard
    # a word's bits do not depend on the other words of the call: each word alone, and the words in another order
    off = np.concatenate([[0], np.cumsum(counts)])
    for m in (1, 4):
        alone = c.ctc_stitch_decode(logits[off[m]:off[m + 1]], counts[m:m + 1], 40)
        n = alone[0].shape[1]
        assert np.array_equal(alone[0][0], labels[m, :n]) and alone[1][0] == log_word[m] and np.array_equal(alone[2][0], chars[m, :n])
    if discard == 2 and classes == 37:
        # K = 1 is the ordinary decode, bit for bit
        ones = np.ones(5, np.int32)
        got = c.ctc_stitch_decode(logits[:5], ones, 40)
        want = c.crnn_decode_logits(logits[:5], scores=True)
        _same_rows(got[:3], (want["labels"], want["log_word"], want["chars"]), "K = 1")


# ---- 4. the whole route ----------------------------------------------------------------------------------------------
ROUTE_BOXES = np.stack([wc.rect(10, 10, 60, 20), wc.rect(5, 70, 180, 16), wc.rect(90, 8, 70, 22), wc.rect(5, 90, 300, 16),
                        wc.rotated(200, 60, 180, 16, 30), wc.rect(200, 10, 90, 25), wc.rect(5, 40, 390, 14), wc.rect(300, 8, 80, 24),
                        wc.trapezoid(20, 30, 320, 20, 2), wc.rect(150, 95, 64, 20), wc.rect(230, 90, 100, 28), wc.rect(330, 60, 60, 30)])


def _logits_of(c, crops):
    c.crnn_set_taps(["ctc"])
    try:
        c.crnn_forward(crops)
        taps = c.crnn_taps()
    finally:
        c.crnn_set_taps([])
    return taps["ctc"]["in"][0].reshape(len(crops), T, -1)


def _pad(rows, width, fill):
    out = np.full((len(rows), width), fill, rows.dtype)
    out[:, :rows.shape[1]] = rows
    return out


def test_whole_route_equals_its_parts(wctx):
    c = wctx
    pages = np.stack([wc.page(), np.ascontiguousarray(wc.page()[:, ::-1])])
    groups = [ROUTE_BOXES[:7], ROUTE_BOXES[7:]]
    labels, log_word, chars, frames, windows = c.recognize_boxes_windowed(pages, groups, 10.0, 40)
    want_k, _, _, want_t = ws.plan_boxes(ROUTE_BOXES)
    assert windows.tolist() == want_k.tolist() and frames.tolist() == want_t.tolist()
    assert labels.shape == chars.shape == (12, want_t.max()) and (want_k == 1).sum() >= 5 and (want_k > 1).sum() >= 4
    # K = 1: recognize_boxes with scores, bit for bit
    plain = c.recognize_boxes(pages, groups, return_scores=True)
    one = want_k == 1
    _same_rows((labels[one][:, :48], log_word[one], chars[one][:, :48]), (plain[0][one], plain[1][one], plain[2][one]), "K = 1")
    assert (labels[one][:, 48:] == -1).all() and (chars[one][:, 48:] == 0).all()
    assert (labels[one] >= 0).any(1).sum() >= 3, "the short words must decode to something"
    # K > 1: the stitch-decode seam on the recogniser's own logits for the windowed crops
    crops = c.warp_crops_windowed(pages, groups, 10.0, 40)[0]
    logits = _logits_of(c, crops)
    seam = c.ctc_stitch_decode(logits, want_k, 40)
    _same_rows((labels, log_word, chars, frames), seam, "stitch-decode on the route's logits")
    stmt = ws.stitch_decode(logits, want_k, 40, 2)
    assert sum(s[4] for s, k in zip(stmt, want_k) if k > 1) * 2 >= (want_k > 1).sum()
    # permuting the boxes permutes the results
    perm = np.array([3, 0, 6, 1, 5, 2, 4])
    shuffled = c.recognize_boxes_windowed(pages, [groups[0][perm], groups[1]], 10.0, 40)
    order = np.concatenate([perm, np.arange(7, 12)])
    _same_rows(shuffled, (labels[order], log_word[order], chars[order], frames[order], windows[order]), "permuted")
    # other boxes' pixels: word 3 of image 0 keeps its bits when image 1 changes and the other boxes move
    loud = pages.copy()
    loud[1] = 255 - loud[1]
    moved = [np.stack([b + np.float32(1.0) if i != 3 else b for i, b in enumerate(groups[0])]), groups[1]]
    again = c.recognize_boxes_windowed(loud, moved, 10.0, 40)
    assert want_k[3] > 1
    _same_rows([a[3:4] for a in again], [a[3:4] for a in (labels, log_word, chars, frames, windows)], "other boxes")


# ---- 5. the batch edge -----------------------------------------------------------------------------------------------
def test_windows_straddle_the_recogniser_batch(wctx):
    """26 boxes of 1661 x 8 on a 270 x 1700 page: K = 40 each, 1040 windows, more than one recogniser batch of 1024, so the
    windows of one word lie on both sides of a batch edge.  The same boxes in two calls of 13 must give the same rows.
    (Measured with plain batches of 1024 + 16: words 0 .. 24 the same bits, word 25 -- its last 16 windows alone in the tail
    batch -- 4 ulp off in log_word and in its character scores, labels equal: below 82 crops the recogniser's per-frame 1x1
    layers run on another GEMM kernel.  The route therefore never leaves a tail of fewer than 82 crops behind a full batch:
    958 + 82 here, the edge inside word 23.)"""
    c = wctx
    page = wc.page(270, 1700, seed=11)
    boxes = np.stack([wc.long_box(4 + 10 * i) for i in range(26)])
    assert ws.plan_boxes(boxes)[0].tolist() == [40] * 26
    whole = c.recognize_boxes_windowed(page[None], [boxes], 10.0, 40)
    assert whole[4].tolist() == [40] * 26 and whole[0].shape == (26, 39 * 40 + 48)
    halves = [c.recognize_boxes_windowed(page[None], [boxes[s:s + 13]], 10.0, 40) for s in (0, 13)]
    want = [np.concatenate([a, b]) for a, b in zip(*halves)]
    differ = [int((_bits(g) != _bits(w)).reshape(26, -1).any(1).sum()) for g, w in zip(whole, want)]
    print(f"\nbatch edge: words that differ between one call and two, per output (labels, log_word, chars, frames, windows): {differ}")
    _same_rows(whole, want, "one call of 26 == two calls of 13")
    assert len({r.tobytes() for r in whole[2]}) == 26, "the reference rows must differ pairwise"


# ---- 6. refusals, surface, residency ---------------------------------------------------------------------------------
def test_refusals(wctx, crnn_weights):
    c = wctx
    page = wc.page()[None]
    long_ = [wc.PLAN_BOXES[3:4]]
    with pytest.raises(ValueError, match=r"box 1 of image 0.*KOCR_WINDOW_FRAMES_MAX"):
        c.recognize_boxes_windowed(np.zeros((1, 32, 3000, 3), np.uint8), [np.stack([wc.rect(0, 0, 100, 20), wc.rect(0, 0, 2900, 8)])])
    with pytest.raises(ValueError, match="KOCR_WINDOW_FRAMES_MAX"):
        c.window_plan(wc.rect(0, 0, 2900, 8)[None])
    for bad in (dict(overlap=12), dict(overlap=104), dict(aspect=6.4), dict(aspect=float("nan"))):
        for call in (lambda **kw: c.recognize_boxes_windowed(page, long_, **kw), lambda **kw: c.window_plan(long_[0], **kw),
                     lambda **kw: c.warp_crops_windowed(page, long_, **kw)):
            with pytest.raises(ValueError, match="aspect must be finite"):
                call(**bad)
    with pytest.raises(ValueError):
        c.ctc_stitch_decode(np.zeros((2, 50, 37), np.float32), [2], overlap=12)
    # d >= 50 - f
    c.crnn_set_rnn_steps_to_discard(38)
    try:
        with pytest.raises(ValueError, match="rnn_steps_to_discard 38"):
            c.recognize_boxes_windowed(page, long_, overlap=96)
        c.crnn_set_rnn_steps_to_discard(37)
        assert c.recognize_boxes_windowed(page, long_, overlap=96)[3].tolist() == [ws.plan_boxes(long_[0], 10.0, 96, 37)[3][0]]
    finally:
        c.crnn_set_rnn_steps_to_discard(2)
    # every conflicting switch, on the route and on the seams
    c.set_charsets(np.ones((1, 36), np.uint8))
    from tests import workspace_cases as wsc
    c.set_patterns(*wsc.patterns(37).tables())
    c.set_lexicon(np.array([[1, 2, -1]], np.int32), np.array([2], np.int32))
    switches = [("beam", lambda: c.set_beam(4, 2)), ("lexicon match", lambda: c.set_lexicon_match(1)), ("character set", lambda: c.set_charset(0)),
                ("pattern", lambda: c.set_pattern(0)), ("orientation", lambda: c.set_orientation("flip")),
                ("character boxes", lambda: c.set_char_boxes(True))]
    try:
        for name, on in switches:
            _switches_off(c)
            on()
            for call in (lambda: c.recognize_boxes_windowed(page, long_), lambda: c.window_plan(long_[0]), lambda: c.warp_crops_windowed(page, long_),
                         lambda: c.ctc_stitch_decode(np.zeros((1, 50, 37), np.float32), [1])):
                with pytest.raises(ValueError, match=f"long words.*cannot be combined with.*{name}"):
                    call()
    finally:
        _switches_off(c)
        c.set_lexicon(None)
    # float images (the Recognizer's refusal), zero boxes, zero images
    import keras_ocr_amd
    rec = keras_ocr_amd.recognition.Recognizer(weights=_sharpened(crnn_weights), ctx=c)
    with pytest.raises(NotImplementedError, match="uint8"):
        rec.recognize_from_boxes_windowed([wc.page().astype(np.float32)], [wc.PLAN_BOXES[:2]])
    for images, groups in ((page, [np.zeros((0, 4, 2), np.float32)]), (np.zeros((0, 120, 400, 3), np.uint8), [])):
        out = c.recognize_boxes_windowed(images, groups)
        assert [a.shape for a in out] == [(0, 48), (0,), (0, 48), (0,), (0,)]
    assert rec.recognize_from_boxes_windowed([wc.page()], [[]]) == [[]]
    with pytest.raises(ZeroDivisionError):
        c.recognize_boxes_windowed(page, [np.stack([wc.PLAN_BOXES[0], wc.rect(5, 5, 300, 0.4)])])


def test_recognizer_surface(wctx, crnn_weights):
    import keras_ocr_amd

    rec = keras_ocr_amd.recognition.Recognizer(weights=_sharpened(crnn_weights), ctx=wctx)
    pages = [wc.page(), np.ascontiguousarray(wc.page()[:, ::-1])]
    groups = [ROUTE_BOXES[:7], ROUTE_BOXES[7:]]
    texts = rec.recognize_from_boxes_windowed(pages, groups)
    labels, log_word, chars, frames, windows = wctx.recognize_boxes_windowed(np.stack(pages), groups)
    from keras_ocr_amd.pipeline import decode_labels
    assert [t for g in texts for t in g] == decode_labels(rec.alphabet, labels) and [len(g) for g in texts] == [7, 5]
    scored = rec.recognize_from_boxes_windowed(pages, groups, return_scores=True, return_windows=True)
    flat = [w for g in scored for w in g]
    assert [t for t, _, _ in flat] == [t for g in texts for t in g] and [k for _, _, k in flat] == windows.tolist()
    for m, (text, score, _) in enumerate(flat):
        assert score.detection is None and score.log_word == float(log_word[m]) and score.word == np.exp(score.log_word)
        assert np.array_equal(score.characters, chars[m, :len(text)]) and score.characters.dtype == np.float32
    counted = rec.recognize_from_boxes_windowed(pages, groups, return_windows=True)
    assert [w for g in counted for w in g] == [(t, k) for t, _, k in flat]
    plain = rec.recognize_from_boxes(pages, groups)
    for m, (a, b) in enumerate(zip([t for g in plain for t in g], [t for g in texts for t in g])):
        if windows[m] == 1:
            assert a == b
    # pages of two sizes: one call per image
    mixed = rec.recognize_from_boxes_windowed([pages[0], pages[1][:100]], [groups[0], groups[1][:2]])
    assert mixed[0] == texts[0] and len(mixed[1]) == 2


@pytest.fixture(scope="module")
def pipe(craft_weights, crnn_weights):
    import keras_ocr_amd
    from oracle import craft as ocraft, tools as otools
    from tests import synth

    page = synth.text_page(96, 128, 5, seed=21)[None]
    big = np.stack([otools.resize_image(p, 2, 2048)[0] for p in page])
    calibrated = keras_ocr_amd.weights.calibrate_craft_head(craft_weights, ocraft.detector_predict(craft_weights, big), text_frac=0.10,
                                                            link_frac=0.04)
    c = keras_ocr_amd.Context(0)
    det = keras_ocr_amd.detection.Detector(weights=calibrated, ctx=c)
    rec = keras_ocr_amd.recognition.Recognizer(weights=_sharpened(crnn_weights), ctx=c)
    yield keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)
    c.close()


def test_pipeline_surface(pipe):
    from oracle import tools as otools
    from tests import synth

    pages = [synth.text_page(96, 128, 5, seed=21), synth.text_page(80, 100, 4, seed=22)]
    plain = pipe.recognize(pages)
    assert sum(len(g) for g in plain) >= 4
    # an aspect that makes some of the detector's boxes long, if any is wider than 200 : 31 at all
    for aspect in (10.0, 200 / 31):
        got = pipe.recognize_windowed(pages, aspect=aspect, overlap=40)
        assert [len(g) for g in got] == [len(g) for g in plain]
        n_short = 0
        for g, p, page in zip(got, plain, pages):
            scale = otools.resize_scale(page.shape, 2, 2048)
            for (text, box), (ptext, pbox) in zip(g, p):
                assert np.array_equal(_bits(np.asarray(box, np.float32)), _bits(np.asarray(pbox, np.float32)))
                w, h = otools.get_rotated_width_height(otools.get_rotated_box(np.asarray(box, np.float32) * np.float32(scale))[0])
                if not float(w) > aspect * float(h) * 1.01 and not float(w) > aspect * float(h) * 0.99:
                    assert text == ptext
                    n_short += 1
        assert n_short >= 2
    scored = pipe.recognize_windowed(pages, return_scores=True)
    want = pipe.recognize_with_scores(pages)
    for g, w in zip(scored, want):
        assert len(g) == len(w)
        for (text, box, score), (wtext, wbox, wscore) in zip(g, w):
            assert np.array_equal(box, wbox) and score.detection == wscore.detection and isinstance(score.log_word, float)
            assert len(score.characters) == len(text)
    assert pipe.recognize_windowed([]) == []
    with pytest.raises(NotImplementedError, match="uint8"):
        pipe.recognize_windowed([pages[0].astype(np.float32)])


def test_resident_results(crnn_weights):
    """a cold context with guards; a second call with more windows and longer rows; release forgets the rows"""
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    try:
        c.load_crnn(_sharpened(crnn_weights))
        c.set_arena_guards(True)
        with pytest.raises(ValueError, match="no windowed result is resident"):
            c.windowed_results()
        page = wc.page()[None]
        small = c.recognize_boxes_windowed(page, [ROUTE_BOXES[:2]])
        assert c.check_arena_guards()[0] == 0
        assert small[0].shape == (2, ws.plan_boxes(ROUTE_BOXES[:2])[3].max())
        again = c.windowed_results()
        _same_rows(again, small, "fetched twice")
        large = c.recognize_boxes_windowed(page, [ROUTE_BOXES[:7]])
        assert c.check_arena_guards()[0] == 0
        assert large[0].shape[1] > small[0].shape[1] and large[4].sum() > small[4].sum()
        _same_rows([a[:2] for a in large[1:2]], [a for a in small[1:2]], "the first words again")
        for name, stats in c.arena_stats().items():
            assert stats["excess"] == 0, name
        # wider caller buffers are padded, smaller ones refused
        import ctypes
        lab = np.zeros((8, 400), np.int32)
        ch = np.ones((8, 400), np.float32)
        lib, h = c._lib, c._h  # pylint: disable=protected-access
        assert lib.kocr_windowed_results(h, lab.ctypes.data, None, ch.ctypes.data, None, None, 8, 400) == 0
        width = large[0].shape[1]
        assert np.array_equal(lab[:7, :width], large[0]) and (lab[:7, width:] == -1).all() and (ch[:7, width:] == 0).all()
        assert lib.kocr_windowed_results(h, lab.ctypes.data, None, None, None, None, 6, 400) == keras_ocr_amd._lib.KOCR_ECAPACITY  # pylint: disable=protected-access
        assert lib.kocr_windowed_results(h, lab.ctypes.data, None, None, None, None, 8, width - 1) == keras_ocr_amd._lib.KOCR_ECAPACITY  # pylint: disable=protected-access
        del ctypes
        # another call that sizes an arena forgets them; so does the release
        c.warp_crops(page, [ROUTE_BOXES[:1]])
        with pytest.raises(ValueError, match="no windowed result is resident"):
            c.windowed_results()
        c.recognize_boxes_windowed(page, [ROUTE_BOXES[:2]])
        c.release_arenas()
        with pytest.raises(ValueError, match="no windowed result is resident"):
            c.windowed_results()
        _same_rows(c.recognize_boxes_windowed(page, [ROUTE_BOXES[:2]]), small, "cold again")
    finally:
        c.close()


@pytest.fixture(scope="module")
def guarded(crnn_weights):
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    c.load_crnn(_sharpened(crnn_weights))
    c.set_arena_guards(True)
    yield c
    c.close()


@pytest.mark.parametrize("row", wc.workspace_rows(), ids=lambda r: r["name"])
def test_workspace_plans_hold_from_cold(guarded, row):
    """the rows of tests/windows_cases.py as tests/test_workspace_gpu.py runs those of tests/workspace_cases.py: from a cold
    context with guards behind every allocation, no guard damaged, no arena asked for more than its plan, the arenas the row
    names reserved; and the warm call gives the cold call's bits"""
    c = guarded
    c.release_arenas()
    args = row["args"]()
    cold = getattr(c, row["method"])(*args)
    assert c.check_arena_guards()[0] == 0, row["name"]
    stats = c.arena_stats()
    assert all(s["excess"] == 0 for s in stats.values()), (row["name"], stats)
    assert all(stats[a]["requested"] > 0 and stats[a]["peak"] > 0 for a in row["touches"]), (row["name"], stats)
    warm = getattr(c, row["method"])(*args)
    assert c.check_arena_guards()[0] == 0, row["name"]
    assert all(s["excess"] == 0 for s in c.arena_stats().values()), row["name"]
    _same_rows(warm, cold, row["name"])


def test_a_call_just_past_one_batch(wctx):
    """1030 short boxes, every K = 1: 1030 crops.  kocr_recognize_boxes reads them as 1024 + 6, this route as 948 + 82 (no tail
    under crnn_small_batch = 82 crops behind a full batch).  Which guarantee holds there: the route's own -- a word's bits do not
    depend on how the call is cut, so the same boxes in two calls of 515 give the same rows, bit for bit -- and, against
    kocr_recognize_boxes with scores, bit for bit for the words both read in a batch of at least 82 crops (the first 1024: in
    its full batch there, in the 948 or the 82 here).  The 6 words that kocr_recognize_boxes reads in a batch of their own
    take other GEMM kernels for the 1x1 layers and stn_conv_2, so their logits agree only as two runs of the recogniser
    agree, and log_word is held to the CTC gate 1e-6 * 48 * max(1, -log_word) around it where the labels agree."""
    c = wctx
    rng = np.random.default_rng(17)
    boxes = np.stack([wc.rect(int(rng.integers(0, 330)), int(rng.integers(0, 95)), int(rng.integers(40, 70)), int(rng.integers(12, 24)))
                      for _ in range(1030)])
    page = wc.page()[None]
    whole = c.recognize_boxes_windowed(page, [boxes])
    assert whole[4].tolist() == [1] * 1030 and whole[0].shape == (1030, 48)
    halves = [c.recognize_boxes_windowed(page, [boxes[s:s + 515]]) for s in (0, 515)]
    _same_rows(whole, [np.concatenate([a, b]) for a, b in zip(*halves)], "one call of 1030 == two calls of 515")
    plain = c.recognize_boxes(page, [boxes], return_scores=True)
    _same_rows([a[:1024] for a in whole[:3]], [a[:1024] for a in plain], "the words kocr_recognize_boxes reads in its full batch")
    tail = slice(1024, 1030)
    same = (whole[0][tail] == plain[0][tail]).all(1)
    err = np.abs(whole[1][tail].astype(np.float64) - plain[1][tail])
    print(f"\njust past one batch: tail words with equal labels {int(same.sum())} of 6, bit-equal log_word "
          f"{int((_bits(whole[1][tail]) == _bits(plain[1][tail])).sum())} of 6, max |difference| {err.max():.3g}")
    assert np.all(err[same] <= GATE * 48 * np.maximum(1.0, -plain[1][tail][same].astype(np.float64)))


def test_profiler_rows(wctx):
    wctx.profile_enable(True)
    try:
        wctx.profile_reset()
        wctx.recognize_boxes_windowed(wc.page()[None], [ROUTE_BOXES[:4]])
        rows = set(wctx.profile_report())
    finally:
        wctx.profile_enable(False)
    assert {"window_plan", "window_stitch", "ctc_scores_ragged", "warp_crops"} <= rows and "ctc_scores" not in rows and "ctc_greedy" not in rows

