"""Scores on the GPU (kocr_set_scores, kocr_crnn_forward_scores, kocr_detection_scores, kocr_recognition_scores and the
return_scores arguments) against the float64 statement tests/scores_statement.py ("Scores").

Bars: label rows, character scores, detection scores and log_word against -kocr_crnn_ctc_loss are bit for bit; log_word
against the statement on the returned probabilities is held to the CTC gate 1e-6 * T * max(1, loss); against the oracle's
probabilities to the Lipschitz bound sum_t max_c |d log q_t(c)| plus that gate, on the crops whose ORACLE top-two margin
exceeds tests/test_crnn_gpu.py's MARGIN on every frame, where the decodes must be equal."""
import numpy as np
import pytest

from tests import ctc_statement as cs
from tests import scores_statement as ss
from tests import synth

pytestmark = pytest.mark.gpu

GATE = 1e-6    # DESIGN.md section 4, the CTC gate
MARGIN = 1e-3  # tests/test_crnn_gpu.py


def _crops(n, seed):
    x = np.zeros((n, 31, 200), np.float32)
    for i in range(n):
        x[i] = synth.text_page(31, 200, 3, seed=seed + i)[..., 0] / np.float32(255)
    return x


def _recognizer(ctx, weights, **build):
    import keras_ocr_amd
    from keras_ocr_amd.recognition import DEFAULT_BUILD_PARAMS

    n = weights["fc_12/bias"].shape[0]
    alphabet = keras_ocr_amd.recognition.DEFAULT_ALPHABET if n == 37 else "".join(chr(200 + i) for i in range(n - 1))
    return keras_ocr_amd.recognition.Recognizer(alphabet=alphabet, weights=dict(weights), ctx=ctx,
                                                build_params=dict(DEFAULT_BUILD_PARAMS, **build))


@pytest.fixture(scope="module")
def cctx(crnn_weights):
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    c.load_crnn(crnn_weights)
    yield c
    c.close()


def _check_against_own_probs(c, x, what):
    """everything that is stated on the probabilities the same call returns"""
    labels, log_word, chars, probs = c.crnn_forward_scores(x, return_probs=True)
    m, lw = len(x), c.crnn_label_width()
    assert labels.shape == chars.shape == (m, lw) and log_word.shape == (m,) and probs.shape == (m, lw, c.crnn_classes())
    assert log_word.dtype == chars.dtype == np.float32
    want_l, want_p = c.crnn_forward(x, return_probs=True)
    assert np.array_equal(labels, want_l) and np.array_equal(probs, want_p), what
    L = (labels >= 0).sum(1)
    loss = c.crnn_ctc_loss(x, labels, L, np.full(m, lw))
    assert np.array_equal(log_word, -loss), what
    assert np.all(np.isfinite(log_word)) and np.all(log_word <= 1e-5)
    assert ss.no_ties(probs), "a frame of the test's inputs has two equal top probabilities"
    rows, Ls = ss.greedy_decode(probs)
    assert np.array_equal(rows, labels) and np.array_equal(Ls, L)
    stmt = ss.log_word(probs)
    err = np.abs(log_word.astype(np.float64) - stmt)
    gate = GATE * lw * np.maximum(1.0, -stmt)
    print(f"\n{what}: max |log_word - statement| / gate = {(err / gate).max():.3g}; decode lengths {L.min()}..{L.max()}")
    assert np.all(err <= gate), what
    assert np.array_equal(chars, ss.char_scores(probs)), what
    assert np.all(chars[labels < 0] == 0) and np.all(chars[labels >= 0] > 0)
    return labels, log_word, chars


@pytest.mark.parametrize("m", [1, 7, 512])
def test_recogniser_scores_default_build(cctx, m):
    _check_against_own_probs(cctx, _crops(m, seed=300), f"default build M={m}")


@pytest.mark.parametrize("build, classes, m", [({"rnn_steps_to_discard": 0}, 37, 33), ({"stn": False}, 37, 9),
                                                ({}, 1000, 64), ({"rnn_steps_to_discard": 0, "stn": False}, 1000, 5)],
                         ids=["discard_0", "no_stn", "classes_1000", "classes_1000_discard_0_no_stn"])
def test_recogniser_scores_other_builds(crnn_weights, build, classes, m):
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    try:
        w = crnn_weights if classes == 37 else keras_ocr_amd.weights.synthetic_crnn_weights(4321, n_classes=classes)
        rec = _recognizer(c, w, **build)
        x = _crops(m, seed=400)
        labels, log_word, chars = _check_against_own_probs(c, x, f"{build} C={classes} M={m}")
        pairs = rec.recognize_from_boxes([np.zeros((4, 4, 3), np.uint8)], [[]], return_scores=True)
        assert pairs == [[]]
        assert labels.shape[1] == 50 - build.get("rnn_steps_to_discard", 2)
    finally:
        c.close()


def test_scores_do_not_depend_on_the_batch(cctx):
    """A crop's scores do not depend on its position in the batch or on its neighbours, bit for bit, as long as the forward
    takes the same GEMM dispatch (tests/test_ctc_loss_gpu.py::test_loss_and_features_do_not_depend_on_the_batch: a crop
    alone may take another kernel for the 1x1 layers, so that comparison is not made here)."""
    x = _crops(512, seed=900)
    labels, log_word, chars = cctx.crnn_forward_scores(x)
    perm = np.roll(np.arange(512), 100)
    perm[[0, 7]] = perm[[7, 0]]
    l2, w2, c2 = cctx.crnn_forward_scores(x[perm])
    assert np.array_equal(l2, labels[perm]) and np.array_equal(w2, log_word[perm]) and np.array_equal(c2, chars[perm])
    loud = x[perm].copy()
    loud[1:] = 1.0 - loud[1:]
    l3, w3, c3 = cctx.crnn_forward_scores(loud)
    assert np.array_equal(l3[0], labels[perm][0]) and w3[0] == log_word[perm][0] and np.array_equal(c3[0], chars[perm][0])


@pytest.mark.parametrize("m", [1, 5, 40])
def test_scores_against_the_oracle(cctx, crnn_weights, m):
    from oracle import crnn as ocrnn

    x = _crops(m, seed=100)
    labels, log_word, chars, probs = cctx.crnn_forward_scores(x, return_probs=True)
    want_p = ocrnn.crnn_forward(crnn_weights, x[..., None])
    srt = np.sort(want_p, -1)
    safe = ((srt[..., -1] - srt[..., -2]) > MARGIN).all(1)
    assert safe.sum() >= max(1, m // 2)
    rows, _ = ss.greedy_decode(want_p)
    assert np.array_equal(labels[safe], rows[safe])
    stmt = ss.log_word(want_p)
    lip = np.abs(cs.log_q(probs) - cs.log_q(want_p)).max(-1).sum(-1)
    gate = GATE * labels.shape[1] * np.maximum(1.0, -stmt)
    err = np.abs(log_word - stmt)
    print(f"\nM={m}: {int(safe.sum())} safe; |log_word - oracle statement| max {err[safe].max():.3g}, bound min {(lip + gate)[safe].min():.3g}")
    assert np.all(err[safe] <= (lip + gate)[safe]), (err, lip)
    # character scores: each is an entry of the probabilities, so within the probabilities' own tolerance of the oracle's
    want_c = ss.char_scores(want_p)
    assert np.abs(chars[safe] - want_c[safe]).max() <= np.abs(probs - want_p).max() + 1e-7


def test_empty_decode_and_empty_batch(crnn_weights):
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    try:
        w = dict(crnn_weights)
        bias = w["fc_12/bias"].copy()
        bias[-1] += 1e3  # the blank wins every frame of every crop
        w["fc_12/bias"] = bias
        rec = _recognizer(c, w)
        x = _crops(3, seed=10)
        labels, log_word, chars, probs = c.crnn_forward_scores(x, return_probs=True)
        assert np.all(labels == -1) and np.all(chars == 0) and np.all(np.isfinite(log_word))
        stmt = cs.log_q(probs)[..., -1].sum(-1)  # the all-blank path
        assert np.all(np.abs(log_word - stmt) <= GATE * labels.shape[1] * np.maximum(1.0, -stmt))
        assert np.array_equal(log_word, -c.crnn_ctc_loss(x, labels, np.zeros(3, int), np.full(3, labels.shape[1])))
        text, score = rec.recognize((x[0] * 255).astype(np.uint8)[..., None].repeat(3, -1), return_scores=True)
        assert text == "" and score.detection is None and len(score.characters) == 0 and score.word == np.exp(score.log_word)
        # a crop batch of 0
        l0, w0, c0 = c.crnn_forward_scores(np.zeros((0, 31, 200), np.float32))
        assert l0.shape == (0, 48) and w0.shape == (0,) and c0.shape == (0, 48)
    finally:
        c.close()


def test_fetch_errors(crnn_weights):
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    try:
        c.load_crnn(crnn_weights)
        assert c.get_scores() is False
        with pytest.raises(ValueError, match="no detection scores are resident"):
            c.detection_scores([1], 4)
        with pytest.raises(ValueError, match="no recognition scores are resident"):
            c.recognition_scores()
        y = synth.heatmap_batch()
        c.get_boxes(y)  # switch off
        with pytest.raises(ValueError, match="produced with scores off"):
            c.detection_scores([1] * len(y), 1024)
        page = synth.text_page(64, 96, 3, seed=3)
        box = np.array([[[2, 2], [60, 2], [60, 20], [2, 20]]], np.float32)
        c.recognize_boxes(page[None], [box])  # switch off
        with pytest.raises(ValueError, match="produced with scores off"):
            c.recognition_scores()
        c.set_scores(True)
        assert c.get_scores() is True
        labels = c.recognize_boxes(page[None], [box])
        log_word, chars = c.recognition_scores()
        l2, w2, c2 = c.recognize_boxes(page[None], [box], return_scores=True)
        assert np.array_equal(labels, l2) and np.array_equal(log_word, w2) and np.array_equal(chars, c2)
        # the rows keep the width they were produced with
        c.crnn_set_rnn_steps_to_discard(0)
        w3, c3 = c.recognition_scores()
        assert c3.shape == (1, 48) and np.array_equal(c3, chars) and np.array_equal(w3, log_word)
        c.crnn_set_rnn_steps_to_discard(2)
        c.crnn_forward(_crops(1, seed=1))  # another call that processes images: nothing is resident any more
        with pytest.raises(ValueError, match="no recognition scores are resident"):
            c.recognition_scores()
        with pytest.raises(keras_ocr_amd.KocrError):
            c._check(c._lib.kocr_set_scores(c._h, 2))  # pylint: disable=protected-access
    finally:
        c.close()


# ---- detector -------------------------------------------------------------------------------------------------------------

def _smooth_fields():
    from scipy import ndimage

    rng = np.random.default_rng(42)
    ys = []
    for i in range(3):
        f = ndimage.gaussian_filter(rng.standard_normal((2, 150, 130)), (0, 3.0 + i, 3.0 + i))
        f = f / np.abs(f).max() * 1.6
        ys.append(np.moveaxis(f, 0, -1))
    return np.stack(ys).astype(np.float32)


def _check_detection(ctx, y, rule, cap=None, **kw):
    from oracle import postproc

    want_b, debug = postproc.get_boxes(y, return_debug=True, **kw)
    want = ss.detection_scores(y, debug, **{k: v for k, v in kw.items() if k in ("text_threshold", "link_threshold")})
    boxes, scores = ctx.get_boxes(y, min_area_rect=rule, cap=cap, return_scores=True, **kw)
    plain = ctx.get_boxes(y, min_area_rect=rule, cap=cap, **kw)
    assert len(scores) == len(boxes) == len(y)
    for b, p, s, w in zip(boxes, plain, scores, want):
        assert np.array_equal(b, p) and s.dtype == np.float32 and s.shape == (len(b),)
        assert np.array_equal(s, w), (s, w)
        assert np.all(s >= np.float32(kw.get("detection_threshold", 0.7)))
    return boxes, scores


@pytest.mark.parametrize("rule", ["exact", "opencv"])
def test_detection_scores_match_the_statement(ctx, rule):
    y = synth.heatmap_batch()
    boxes, scores = _check_detection(ctx, y, rule)
    assert sum(len(s) for s in scores) >= 6 and len(scores[1]) == 0  # an image without boxes
    _check_detection(ctx, y, rule, detection_threshold=0.5, text_threshold=0.3, link_threshold=0.5, size_threshold=4)
    f = _smooth_fields()
    boxes, scores = _check_detection(ctx, f, rule, cap=8)  # more boxes than cap: the retry of Context.get_boxes
    assert max(len(s) for s in scores) > 8
    assert ctx.get_scores() is False  # return_scores is per call


def test_get_boxes_module_function(ctx):
    import keras_ocr_amd

    y = synth.heatmap_batch()
    d = keras_ocr_amd._lib.default_context()  # pylint: disable=protected-access
    boxes, scores = keras_ocr_amd.detection.getBoxes(y, return_scores=True)
    want_b, want_s = d.get_boxes(y, return_scores=True)
    assert all(np.array_equal(a, b) for a, b in zip(scores, want_s)) and all(np.array_equal(a, b) for a, b in zip(boxes, want_b))


# ---- end to end -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def calibrated(craft_weights):
    import keras_ocr_amd
    from oracle import craft as ocraft, tools as otools

    page = synth.text_page(96, 128, 5, seed=21)[None]
    big = np.stack([otools.resize_image(p, 2, 2048)[0] for p in page])
    heat = ocraft.detector_predict(craft_weights, big)
    return keras_ocr_amd.weights.calibrate_craft_head(craft_weights, heat, text_frac=0.10, link_frac=0.04)


@pytest.fixture(scope="module")
def pipe(calibrated, crnn_weights):
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    det = keras_ocr_amd.detection.Detector(weights=calibrated, ctx=c)
    rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=c)
    yield keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)
    c.close()


PAGES = [(96, 128, 5, 21), (80, 100, 4, 22)]


def _pages():
    return [synth.text_page(h, w, n, seed=s) for h, w, n, s in PAGES]


def _padded(pages):
    from oracle import tools as otools

    resized = [otools.resize_image(p, 2, 2048)[0] for p in pages]
    hmax, wmax = max(r.shape[0] for r in resized), max(r.shape[1] for r in resized)
    return np.stack([otools.pad(r, width=wmax, height=hmax) for r in resized])


def _same_score(a, b):
    return a.detection == b.detection and a.log_word == b.log_word and a.word == b.word and np.array_equal(a.characters, b.characters)


def test_pipeline_scores_equal_the_stages(pipe):
    ctx = pipe.detector._ctx  # pylint: disable=protected-access
    pages = _pages()
    plain = pipe.recognize(pages)
    scored = pipe.recognize_with_scores(pages)
    assert ctx.get_scores() is False
    assert sum(len(g) for g in plain) >= 4
    for g, s in zip(plain, scored):
        assert [t for t, _ in g] == [t for t, _, _ in s]
        assert all(np.array_equal(a[1], b[1]) for a, b in zip(g, s))
    batch = _padded(pages)
    boxes, det = pipe.detector.detect(batch, return_scores=True)
    assert all(np.array_equal(a, b) for a, b in zip(boxes, pipe.detector.detect(batch)))
    pairs = pipe.recognizer.recognize_from_boxes(batch, boxes, return_scores=True)
    assert [[t for t, _ in g] for g in pairs] == pipe.recognizer.recognize_from_boxes(batch, boxes)
    # detection scores against the statement on the heat-map the GPU computed
    heat = ctx.craft_forward(batch)
    from oracle import postproc
    stmt = ss.detection_scores(heat, postproc.get_boxes(heat, return_debug=True)[1])
    for s, d, p, w in zip(scored, det, pairs, stmt):
        assert np.array_equal(d, w)
        assert len(s) == len(d) == len(p)
        for (text, _, score), dv, (ptext, pscore) in zip(s, d, p):
            assert isinstance(score.detection, float) and isinstance(score.word, float) and isinstance(score.log_word, float)
            assert score.detection == float(dv) and score.detection >= 0.7
            assert text == ptext and pscore.detection is None
            assert score.log_word == pscore.log_word and np.array_equal(score.characters, pscore.characters)
            assert score.word == np.exp(score.log_word) and 0.0 < score.word <= 1.0 + 1e-6
            assert score.characters.dtype == np.float32 and len(score.characters) == len(text)
    # recognize_padded with the flag; the device-pointer call agrees with the host-pointer call
    again = pipe.recognize_padded(pages, None, None, return_scores=True)
    assert all(_same_score(a[2], b[2]) for g, h in zip(scored, again) for a, b in zip(g, h))


def test_capacity_overflow_keeps_the_scores(pipe):
    """cap = 1: kocr_pipeline repeats the post-processing on the resident heat-maps, returns KOCR_ECAPACITY, and the boxes,
    labels and scores come through the fetches"""
    ctx = pipe.detector._ctx  # pylint: disable=protected-access
    pages = _pages()
    imgs = [np.ascontiguousarray(p) for p in pages]
    scales, dhs, dws, hmax, wmax = pipe._plan([p.shape for p in pages])  # pylint: disable=protected-access
    args = (imgs, [p.shape[0] for p in pages], [p.shape[1] for p in pages], dhs, dws, hmax, wmax)
    boxes, labels, (det, log_word, chars) = ctx.pipeline(*args, return_scores=True)
    assert max(len(b) for b in boxes) > 1
    b1, l1, (d1, w1, c1) = ctx.pipeline(*args, cap=1, max_crops=1, return_scores=True)
    assert all(np.array_equal(a, b) for a, b in zip(boxes, b1)) and np.array_equal(labels, l1)
    assert all(np.array_equal(a, b) for a, b in zip(det, d1)) and np.array_equal(log_word, w1) and np.array_equal(chars, c1)
    with pytest.raises(ValueError, match="produced with scores off"):
        ctx.pipeline(*args)
        ctx.detection_scores([len(b) for b in boxes], 256)


def test_pipeline_scores_against_the_oracle(pipe, calibrated, crnn_weights):
    from oracle import pipeline as opipe
    from oracle import parity, postproc

    pages = _pages()
    scored = pipe.recognize_with_scores(pages)
    heat_out = []
    want = opipe.recognize(calibrated, crnn_weights, pages, heat_out=heat_out)
    heat = heat_out[0]
    stmt = ss.detection_scores(heat, postproc.get_boxes(heat, return_debug=True)[1])
    matched = 0
    for i, (got, ref, st) in enumerate(zip(scored, want, stmt)):
        tol = parity.heat_tolerance(heat[i])[0]
        assert len(ref) == len(st)
        for (_, rbox), sv in zip(ref, st):
            for _, gbox, score in got:
                if np.abs(np.asarray(gbox) - np.asarray(rbox)).max() <= 1e-3:  # a box both sides report
                    assert abs(score.detection - float(sv)) <= tol, (score.detection, sv, tol)
                    matched += 1
                    break
    assert matched >= 4


def test_float_pages_and_device_batch(pipe):
    import torch

    pages = _pages()
    floats = pipe.recognize_padded([p.astype(np.float32) for p in pages], None, None, return_scores=True)
    plain = pipe.recognize([p.astype(np.float32) for p in pages])
    assert sum(len(g) for g in floats) >= 1
    for g, h in zip(floats, plain):
        assert [t for t, _, _ in g] == [t for t, _ in h]
        for text, box, score in g:
            assert score._fields == ("detection", "word", "log_word", "characters")
            assert isinstance(score.detection, float) and score.detection >= 0.7 and isinstance(score.log_word, float)
            assert score.characters.dtype == np.float32 and len(score.characters) == len(text) and np.shape(box) == (4, 2)
    batch = np.stack([synth.text_page(96, 128, 5, seed=21), synth.text_page(96, 128, 4, seed=23)])
    host = pipe.recognize_padded(batch, None, None, return_scores=True)
    t = torch.from_numpy(batch).cuda()
    torch.cuda.synchronize()
    dev = pipe.recognize_device(t.data_ptr(), 2, 96, 128, return_scores=True)
    assert sum(len(g) for g in host) >= 2
    for g, h in zip(host, dev):
        assert len(g) == len(h)
        for a, b in zip(g, h):
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and _same_score(a[2], b[2])
    assert [[(t_, b) for t_, b, _ in g] for g in dev] is not None
    plain_dev = pipe.recognize_device(t.data_ptr(), 2, 96, 128)
    assert all(len(x) == 2 for g in plain_dev for x in g)


def test_duck_typed_stage_without_scores_is_refused(pipe):
    import keras_ocr_amd

    class PlainDetector:
        def __init__(self, inner):
            self.inner = inner

        def detect(self, images, **kwargs):
            return self.inner.detect(images, **kwargs)

    class PlainRecognizer:
        def __init__(self, inner):
            self.inner, self.alphabet = inner, inner.alphabet

        def recognize_from_boxes(self, images, box_groups, **kwargs):
            return self.inner.recognize_from_boxes(images, box_groups)

    pages = _pages()
    p = keras_ocr_amd.pipeline.Pipeline(detector=PlainDetector(pipe.detector), recognizer=pipe.recognizer)
    assert [[t for t, _ in g] for g in p.recognize(pages)] == [[t for t, _ in g] for g in pipe.recognize(pages)]
    with pytest.raises(TypeError, match="detector"):
        p.recognize_with_scores(pages)
    p = keras_ocr_amd.pipeline.Pipeline(detector=pipe.detector, recognizer=PlainRecognizer(pipe.recognizer))
    with pytest.raises(TypeError, match="recognizer"):
        p.recognize_with_scores(pages)


# ---- launches -------------------------------------------------------------------------------------------------------------

def test_scores_off_launches_what_it_always_did(pipe):
    """Off: no profiler row that the switch adds.  On: the recogniser's decode is ONE launch, ctc_scores in the place of
    ctc_greedy, and the detector launches nothing more; every other row keeps its launch count."""
    ctx = pipe.detector._ctx  # pylint: disable=protected-access
    pages = _pages()

    def rows(on):
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            pipe.recognize_padded(pages, None, None, return_scores=on)
            return {name: row["launches"] for name, row in ctx.profile_report().items()}
        finally:
            ctx.profile_enable(False)

    off, on = rows(False), rows(True)
    assert "ctc_scores" not in off and off["ctc_greedy"] >= 1
    assert set(on) - set(off) == {"ctc_scores"} and set(off) - set(on) == {"ctc_greedy"}
    assert on["ctc_scores"] == off["ctc_greedy"]
    assert {k: v for k, v in on.items() if k != "ctc_scores"} == {k: v for k, v in off.items() if k != "ctc_greedy"}
