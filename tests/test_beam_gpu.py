"""CTC prefix beam search on the GPU (kocr_crnn_beam, ctc_beam_kernel; DESIGN.md section 4, "Beam search") against the float64
statement tests/beam_statement.py, run on the GPU's own fc_12 logits (the "ctc" tap's input, as tests/crnn_layer_check.py
takes them): only the search is under test here, the network is covered elsewhere.

Label rows must equal the statement's EXACTLY on every crop whose decision margin (beam_statement: the smallest relative gap
at any decision) exceeds margin_bound().  The float32-vs-float64 error of one CTC total is what tests/test_ctc_loss_gpu.py gates:
GATE = 1e-6, |err| <= 1e-6 * T_m * max(1, |total|) (its lines 4 and 14).  A decision compares two totals, hence twice that.
At least max(1, m // 2) crops must be compared (the rule of tests/test_crnn_gpu.py:45); the share is printed (pytest -s).
TensorFlow's own decoder cannot be executed here; the statement is pinned by exhaustive enumeration instead
(tests/test_beam_statement_cpu.py).

Inputs.  A wide beam decides between close candidates: per frame the B-th and the (B + 1)-th of up to B * (C - 1) + B totals,
48 times per crop.  On the plain synthetic weights (frame maxima around 0.35) the statement, run on the CPU oracle's logits,
leaves 27 of 40 consecutive crops above the margin at B = 4, 8 of 40 at B = 16 and none of 40 at B = 64.  So (a) fc_12 of the
synthetic weights is doubled (SHARPEN), which spreads the candidates (B = 4 / 16 / 64: 87 % / 55 % / 14 % of 256 crops above the
margin), and (b) per beam width the crop seeds are chosen BY THE STATEMENT ALONE, on the oracle's logits, among 856 scanned:
the leading entries of SEEDS[B] had margin / bound above 1.8 (B = 64) resp. 3.5 (B = 16) there for K = 1 and K = 3, the rest
are unselected consecutive seeds, most of which are not compared.  The GPU's own logits decide in the test what is compared."""
import numpy as np
import pytest

from tests import beam_statement as bs
from tests import ctc_statement as cs
from tests import synth

pytestmark = pytest.mark.gpu

GATE = 1e-6  # tests/test_ctc_loss_gpu.py
T = 50
SHARPEN = 2.0
SEEDS = {
    4: list(range(1000, 1040)),
    16: [1047, 1228, 1004, 1221, 1001, 1186, 1137, 1207, 1245, 1000, 1241, 1139, 1210, 1055, 1090, 1041, 1169, 1017, 1104, 1194,
         1195, 1111, 1048, 1065, 1122, 1168, 1205, 1172, 1002, 1112] + list(range(100, 110)),
    64: [2299, 1204, 1174, 2105, 1172, 2373, 1122, 2248, 1238, 2161, 1091, 2253, 2023, 2364, 2409, 2485, 2592, 1165, 2180, 2340,
         2392, 2262, 2376, 2256, 2471, 2009, 2085, 1192, 2196, 1017, 2362, 2468] + list(range(100, 108)),
}
WIDE_SEEDS = {0: [302, 307, 406, 415, 427, 432, 448, 465, 470], 5: [300, 302, 306, 307, 406, 416, 428, 444, 451]}


def margin_bound(frames):
    return 2 * GATE * frames


def _crops(n, seed):
    seeds = seed[:n] if isinstance(seed, list) else range(seed, seed + n)
    return np.stack([synth.text_page(31, 200, 3, seed=s)[..., 0] / np.float32(255) for s in seeds])


def _sharpened(weights):
    w = dict(weights)
    w["fc_12/kernel"] = w["fc_12/kernel"] * np.float32(SHARPEN)
    w["fc_12/bias"] = w["fc_12/bias"] * np.float32(SHARPEN)
    return w


@pytest.fixture(scope="module")
def crnn_ctx(ctx, crnn_weights):
    ctx.crnn_set_rnn_steps_to_discard(2)
    ctx.load_crnn(_sharpened(crnn_weights))
    assert ctx.crnn_classes() == 37
    yield ctx
    ctx.load_crnn(crnn_weights)


def _logits(c, x):
    """fc_12's output (M, 50, C) of the crops, as the decode's launch read it"""
    c.crnn_set_taps(["ctc"])
    try:
        c.crnn_forward(x)
        taps = c.crnn_taps()
    finally:
        c.crnn_set_taps([])
    return taps["ctc"]["in"][0].reshape(len(x), T, -1)


def _statement(logits, discard, beam_width, top_paths):
    from oracle import crnn as ocrnn

    lg = logits[:, discard:].astype(np.float64)
    return bs.beam_search_batch(cs.log_q(ocrnn.softmax_f64(lg)), beam_width, top_paths, rank=lg)


def _check(c, x, beam_width, top_paths, what):
    lw = c.crnn_label_width()
    labels, log_prob = c.crnn_beam(x, beam_width, top_paths)
    assert labels.shape == (len(x), top_paths, lw) and labels.dtype == np.int32
    assert log_prob.shape == (len(x), top_paths) and log_prob.dtype == np.float32
    want_l, want_p, margin = _statement(_logits(c, x), T - lw, beam_width, top_paths)
    safe = margin > margin_bound(lw)
    print(f"\n{what}: compared {int(safe.sum())} of {len(x)} crops, smallest margin / bound = {margin.min() / margin_bound(lw):.3g}")
    assert np.array_equal(labels[safe], want_l[safe]), what
    assert safe.sum() >= max(1, len(x) // 2), what
    # the values: the float32 forward algorithm against the float64 one (the gate of tests/test_ctc_loss_gpu.py)
    fin = np.isfinite(want_p[safe])
    assert np.array_equal(np.isfinite(log_prob[safe]), fin)
    err = np.abs(log_prob[safe][fin] - want_p[safe][fin])
    assert (err <= GATE * lw * np.maximum(1.0, np.abs(want_p[safe][fin]))).all(), what
    _check_rows(c, x, labels, log_prob)
    return labels, log_prob


def _check_rows(c, x, labels, log_prob):
    """log_prob is -crnn_ctc_loss of its row, bit for bit, and sorted; rows are -1 padded on the right; missing rows -inf"""
    m, k, lw = labels.shape
    assert (np.diff(log_prob, axis=1) <= 0).all()
    lengths = (labels >= 0).sum(-1)
    assert all((row[:n] >= 0).all() and (row[n:] == -1).all() for rows, ns in zip(labels, lengths) for row, n in zip(rows, ns))
    assert labels.max() < c.crnn_classes() - 1
    assert np.isfinite(log_prob[:, 0]).all()
    for j in range(k):
        there = log_prob[:, j] != -np.inf
        assert (lengths[~there, j] == 0).all()
        if there.any():
            loss = c.crnn_ctc_loss(x[there], labels[there, j], lengths[there, j], np.full(int(there.sum()), lw))
            assert np.array_equal(log_prob[there, j], -loss)
    for rows, lp in zip(labels, log_prob):  # distinct readings
        assert len({tuple(r) for r, v in zip(rows, lp) if v != -np.inf}) == int((lp != -np.inf).sum())


@pytest.mark.parametrize("top_paths", [1, 3])
@pytest.mark.parametrize("beam_width", [4, 16, 64])
@pytest.mark.parametrize("m", [1, 5, 40])
def test_labels_equal_the_statement(crnn_ctx, m, beam_width, top_paths):
    _check(crnn_ctx, _crops(m, SEEDS[beam_width]), beam_width, top_paths, f"m={m} B={beam_width} K={top_paths}")


def test_batch_and_position_invariance(crnn_ctx):
    """a crop's beam result is the same bits alone, in a batch of 40 and at another position; the greedy decode of the same
    context is unchanged by an interleaved beam call"""
    x = _crops(40, seed=100)
    greedy = crnn_ctx.crnn_forward(x)
    labels, log_prob = crnn_ctx.crnn_beam(x, 16, 3)
    assert np.array_equal(crnn_ctx.crnn_forward(x), greedy)
    for i in (0, 7, 39):
        la, lp = crnn_ctx.crnn_beam(x[i:i + 1], 16, 3)
        assert np.array_equal(la[0], labels[i]) and np.array_equal(lp[0].view(np.uint32), log_prob[i].view(np.uint32))
    perm = np.roll(np.arange(40), 11)
    la, lp = crnn_ctx.crnn_beam(x[perm], 16, 3)
    assert np.array_equal(la, labels[perm]) and np.array_equal(lp.view(np.uint32), log_prob[perm].view(np.uint32))
    # the best reading is at least as probable as the greedy one wherever the greedy one is in the beam's view
    lw = crnn_ctx.crnn_label_width()
    g_loss = crnn_ctx.crnn_ctc_loss(x, greedy, (greedy >= 0).sum(-1), np.full(40, lw))
    same = (labels[:, 0] == greedy).all(-1)
    assert np.array_equal(log_prob[same, 0], -g_loss[same])


@pytest.mark.parametrize("discard", [0, 5])
def test_wide_alphabet_and_other_discards(ctx, crnn_weights, discard):
    """96 classes (more than the 64 lanes; the class pruning keeps 4 resp. 16 of 95) and rnn_steps_to_discard 0 and 5; seeds
    chosen as SEEDS, margin / bound above 1.8 on the oracle's logits"""
    import keras_ocr_amd

    try:
        ctx.crnn_set_rnn_steps_to_discard(discard)
        ctx.load_crnn(_sharpened(keras_ocr_amd.weights.synthetic_crnn_weights(4321, n_classes=96)))
        assert ctx.crnn_classes() == 96 and ctx.crnn_label_width() == T - discard
        x = _crops(9, WIDE_SEEDS[discard])
        for beam_width, top_paths in [(4, 1), (16, 3)]:
            labels, _ = _check(ctx, x, beam_width, top_paths, f"96 classes, discard {discard}, B={beam_width} K={top_paths}")
            assert labels.shape == (9, top_paths, T - discard)
    finally:
        ctx.crnn_set_rnn_steps_to_discard(2)
        ctx.load_crnn(crnn_weights)


def test_bad_arguments_name_the_argument(crnn_ctx):
    x = _crops(1, seed=1)
    for beam_width, top_paths, name in [(0, 1, "beam_width"), (65, 1, "beam_width"), (4, 5, "top_paths"), (4, 0, "top_paths")]:
        with pytest.raises(ValueError, match=name):
            crnn_ctx.crnn_beam(x, beam_width, top_paths)
        if beam_width:  # 0 turns the beam off
            with pytest.raises(ValueError, match=name):
                crnn_ctx.set_beam(beam_width, top_paths)
    lib, h = crnn_ctx._lib, crnn_ctx._h  # pylint: disable=protected-access
    lab, lp = np.zeros((1, 1, 48), np.int32), np.zeros((1, 1), np.float32)
    for beam_width, top_paths, name in [(0, 1, b"beam_width"), (65, 1, b"beam_width"), (4, 5, b"top_paths")]:
        rc = lib.kocr_crnn_beam(h, x.ctypes.data, 1, beam_width, top_paths, lab.ctypes.data, lp.ctypes.data, 0)
        assert rc == -1 and name in lib.kocr_last_error(h)  # KOCR_EINVAL
    assert crnn_ctx.get_beam() == (0, 1)
    with pytest.raises(ValueError, match="beam off"):
        crnn_ctx.recognize_boxes(np.full((1, 40, 220, 3), 200, np.uint8), [np.array([[[2, 2], [210, 2], [210, 33], [2, 33]]], np.float32)])
        crnn_ctx.recognition_beams()


# ---- end to end -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipe(craft_weights, crnn_weights):
    import keras_ocr_amd
    from oracle import craft as ocraft, tools as otools

    page = synth.text_page(96, 128, 5, seed=21)[None]
    big = np.stack([otools.resize_image(p, 2, 2048)[0] for p in page])
    calibrated = keras_ocr_amd.weights.calibrate_craft_head(craft_weights, ocraft.detector_predict(craft_weights, big),
                                                            text_frac=0.10, link_frac=0.04)
    c = keras_ocr_amd.Context(0)
    det = keras_ocr_amd.detection.Detector(weights=calibrated, ctx=c)
    rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=c)
    yield keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)
    c.close()


def _padded(pages):
    from oracle import tools as otools

    resized = [otools.resize_image(p, 2, 2048)[0] for p in pages]
    hmax, wmax = max(r.shape[0] for r in resized), max(r.shape[1] for r in resized)
    return np.stack([otools.pad(r, width=wmax, height=hmax) for r in resized])


def test_pipeline_equals_the_stages(pipe):
    ctx = pipe.detector._ctx  # pylint: disable=protected-access
    pages = [synth.text_page(96, 128, 5, seed=21), synth.text_page(80, 100, 4, seed=22)]
    kwargs = {"beam_width": 16, "top_paths": 3, "batch_size": 7}
    plain = pipe.recognize(pages)
    beamed = pipe.recognize(pages, recognition_kwargs=kwargs)
    assert ctx.get_beam() == (0, 1)
    assert sum(len(g) for g in plain) >= 4
    assert all(np.array_equal(a[1], b[1]) for g, h in zip(plain, beamed) for a, b in zip(g, h))
    assert [t for g in pipe.recognize(pages) for t, _ in g] == [t for g in plain for t, _ in g]
    batch = _padded(pages)
    boxes = pipe.detector.detect(batch)
    stages = pipe.recognizer.recognize_from_boxes(batch, boxes, beam_width=16, top_paths=3)
    assert [[alt for alt, _ in g] for g in beamed] == stages
    for alternatives in (alt for g in stages for alt in g):
        assert 1 <= len(alternatives) <= 3 and all(isinstance(t, str) and isinstance(v, float) for t, v in alternatives)
        assert [v for _, v in alternatives] == sorted((v for _, v in alternatives), reverse=True)
    # one size, mixed sizes and float images take three branches of recognize_from_boxes
    taller = np.pad(batch[1], ((0, 2), (0, 0), (0, 0)))
    mixed = pipe.recognizer.recognize_from_boxes([batch[0], taller], boxes, beam_width=16, top_paths=3)
    assert mixed[0] == stages[0]
    assert mixed[1:] == pipe.recognizer.recognize_from_boxes([taller], boxes[1:], beam_width=16, top_paths=3)
    as_float = pipe.recognizer.recognize_from_boxes(list(batch.astype(np.float32)), boxes, beam_width=16, top_paths=3)
    assert [[len(a) for a in g] for g in as_float] == [[len(a) for a in g] for g in stages]
    assert all(len(a) == 1 for g in pipe.recognizer.recognize_from_boxes(batch, boxes, beam_width=16) for a in g)
    # the stage-wise pipeline (float pages) returns the same structure
    floats = pipe.recognize([p.astype(np.float32) for p in pages], recognition_kwargs=kwargs)
    plain_floats = pipe.recognize([p.astype(np.float32) for p in pages])
    assert [len(g) for g in floats] == [len(g) for g in plain_floats] and sum(len(g) for g in floats) >= 4
    assert all(np.array_equal(a[1], b[1]) for g, h in zip(plain_floats, floats) for a, b in zip(g, h))
    assert all(isinstance(alt, list) and alt for g in floats for alt, _ in g)
    # with scores: the score is the greedy decode's
    scored = pipe.recognize_with_scores(pages, recognition_kwargs=kwargs)
    greedy = pipe.recognize_with_scores(pages)
    for g, h, b in zip(scored, greedy, beamed):
        assert [alt for alt, _, _ in g] == [alt for alt, _ in b]
        assert all(a[2].log_word == c[2].log_word and a[2].detection == c[2].detection for a, c in zip(g, h))
        for (alt, _, score), (text, _, _) in zip(g, h):
            hit = [v for t, v in alt if t == text]
            assert not hit or np.float32(hit[0]) == np.float32(score.log_word)
    # a single crop
    crop = batch[0][:31, :200]
    one = pipe.recognizer.recognize(crop, beam_width=16, top_paths=3)
    assert isinstance(one, list) and 1 <= len(one) <= 3 and isinstance(pipe.recognizer.recognize(crop), str)
    alt, score = pipe.recognizer.recognize(crop, return_scores=True, beam_width=16, top_paths=3)
    assert alt == one and score.detection is None
    for bad, name in [({"beam_width": 0}, "beam_width"), ({"beam_width": 65}, "beam_width"), ({"beam_width": 4, "top_paths": 5}, "top_paths")]:
        with pytest.raises(ValueError, match=name):
            pipe.recognize(pages, recognition_kwargs=bad)
        with pytest.raises(ValueError, match=name):
            pipe.recognizer.recognize(crop, **bad)


def test_beam_off_launches_what_it_always_launched(pipe):
    """the beam is one more profiler row, ctc_beam, once per recogniser batch; every other row and count is the plain call's"""
    ctx = pipe.detector._ctx  # pylint: disable=protected-access
    pages = [synth.text_page(96, 128, 5, seed=21), synth.text_page(80, 100, 4, seed=22)]

    def rows(kwargs):
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            pipe.recognize(pages, recognition_kwargs=kwargs)
            return {name: row["launches"] for name, row in ctx.profile_report().items()}
        finally:
            ctx.profile_enable(False)

    off, on = rows(None), rows({"beam_width": 16, "top_paths": 3})
    assert "ctc_beam" not in off and off["ctc_greedy"] >= 1
    assert on.pop("ctc_beam") == off["ctc_greedy"]
    assert on == off == rows({"batch_size": 4})
