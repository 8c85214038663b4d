"""Patterns on the GPU ("Patterns"; csrc/crnn_kernels.hip: pattern_viterbi_kernel, pattern_rescore_kernel)
on the frozen (case, pattern) pairs of tests/pattern_cases.py.  tests/test_patterns_cpu.py shows with the float64 statement
alone that every pair compared here is decidable, an exact tie that only the tie rule resolves, or without a fit.

  1. statement     kocr_crnn_decode_logits_patterns against tests/pattern_statement.py: labels exact, log_path within the gate,
                   log_prob == -loss of the row bit for bit, no-fit rows -1 / -inf, the tie pairs by the stated rule;
  2. invariance    a crop alone, in a batch of 40, at another position, in chunks of 3 crops and of 1; a mixed pattern_of
                   (with -1) against the uniform runs; 1030 boxes through kocr_recognize_boxes_patterns;
  3. switch off    index -1, with or without loaded tables: the bits, the profiler rows and the launch counts of before; on:
                   only the new rows, once per recogniser batch;
  4. end to end    Pipeline.recognize / recognize_from_boxes / the stage-wise route / recognize_tiled; the refusals."""
import functools
import re

import numpy as np
import pytest

from tests import decode_cases as dc
from tests import pattern_cases as pc
from tests import synth

pytestmark = pytest.mark.gpu

GATE = dc.GATE
T = dc.T
NEW_ROWS = {"lexicon_logq", "pattern_viterbi", "pattern_rescore"}


def _id(cfg):
    return f"C{cfg[0]}-d{cfg[1]}"


@functools.lru_cache(maxsize=None)
def _weights(classes, sharp=False):
    import keras_ocr_amd

    w = dict(keras_ocr_amd.weights.synthetic_crnn_weights(4321, n_classes=classes))
    if sharp:  # like the orientation tests' recogniser: decodes are not empty
        w["fc_12/kernel"] = w["fc_12/kernel"] * np.float32(2)
        w["fc_12/bias"] = w["fc_12/bias"] * np.float32(2)
    return w


@pytest.fixture(scope="module")
def recogniser(ctx, crnn_weights):
    """at(classes, discard): the session's context with a recogniser of that many classes, that discard and the patterns of
    pattern_cases.PATTERNS[classes] loaded; returns (ctx, the names)"""
    state = {}

    def at(classes, discard):
        if state.get("classes") != classes:
            ctx.load_crnn(_weights(classes))
            state["classes"] = classes
        ctx.crnn_set_rnn_steps_to_discard(discard)
        pats = pc.compiled(classes)
        ctx.set_patterns(*pats.tables())
        assert ctx.pattern_count() == len(pats) and ctx.get_pattern() == -1
        return ctx, pats.names

    yield at
    ctx.set_patterns(None)
    ctx.set_lexicon_scratch(0)
    ctx.crnn_set_rnn_steps_to_discard(2)
    ctx.load_crnn(crnn_weights)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _run(c, names, entries):
    logits = np.stack([p["case"]["logits"] for p in entries])
    return logits, c.crnn_decode_logits_patterns(logits, [names.index(p["pattern"]) for p in entries])


# ---- 1. against the statement ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", pc.CONFIGS, ids=_id)
def test_decode_equals_the_statement(recogniser, cfg):
    c, names = recogniser(*cfg)
    entries = pc.of_config(*cfg)
    frames = T - cfg[1]
    logits, (labels, log_path, log_prob) = _run(c, names, entries)
    assert labels.shape == (len(entries), frames) and labels.dtype == np.int32
    lengths = (labels >= 0).sum(-1)
    loss = c.crnn_decode_logits(logits, loss_labels=(np.maximum(labels, 0), lengths, np.full(len(entries), frames)))["loss"]
    for i, p in enumerate(entries):
        value, want = pc.decode(p["name"])
        print(p["name"], p["kind"], float(log_path[i]), value, float(log_prob[i]))
        if p["kind"] == "nofit":
            assert (labels[i] == -1).all() and log_path[i] == -np.inf and log_prob[i] == -np.inf, p["name"]
            continue
        got = labels[i][:lengths[i]].tolist()
        assert (labels[i][lengths[i]:] == -1).all() and got == want, (p["name"], got, want)
        assert abs(float(log_path[i]) - value) <= GATE * frames * max(1.0, abs(value)), (p["name"], log_path[i], value)
        assert np.array_equal(_bits(log_prob[i:i + 1]), _bits(-loss[i:i + 1])), (p["name"], log_prob[i], loss[i])
        assert log_prob[i] >= log_path[i] - GATE * frames * max(1.0, abs(value))  # every alignment against the best one
        if p["kind"] == "tie":
            assert got != pc.decode(p["name"], True)[1], p["name"]  # the stated rule, not the opposite one
    assert sum(p["kind"] == "tie" for p in entries) >= 1


# ---- 2. invariance ---------------------------------------------------------------------------------------------------------

def _crop_bytes(c, classes, frames, nodes, states):
    """what one crop takes of the scratch budget (include/kocr.h): its table, and its back-pointers when they leave LDS"""
    fixed = (2 * nodes + 4 * states + 2 * 256) * 4
    table = frames * classes * 4
    fixed += table if fixed + table <= 65536 else 0
    bp = frames * nodes * 2
    return table + (0 if fixed + bp <= 65536 else (bp + 255) // 256 * 256)


@pytest.mark.parametrize("cfg", [(37, 2), (96, 2), (96, 40)], ids=_id)
def test_a_crop_is_the_same_bits_alone_in_a_batch_and_in_any_chunk(recogniser, cfg):
    c, names = recogniser(*cfg)
    entries = pc.of_config(*cfg)
    frames, classes = T - cfg[1], cfg[0]
    batch = [entries[i % len(entries)] for i in range(40)]
    logits, whole = _run(c, names, batch)
    assert np.isfinite(whole[1]).sum() >= 30
    for i in range(len(entries)):  # alone, and at another position (i + len(entries))
        alone = _run(c, names, [batch[i]])[1]
        assert _same([r[i:i + 1] for r in whole], alone) and _same([r[i + len(entries):i + len(entries) + 1] for r in whole], alone), batch[i]["name"]
    pats = pc.compiled(classes)
    used = {names.index(p["pattern"]) for p in batch}
    nodes = max(len(pats.delta[k]) + pc.kp.label_nodes(pats.delta[k]) for k in used)
    states = max(len(pats.delta[k]) for k in used)
    per_crop = _crop_bytes(c, classes, frames, nodes, states)
    c.profile_enable(True)
    try:
        for chunk, budget in ((3, 3 * per_crop + 64), (1, 1), (40, 0)):
            c.set_lexicon_scratch(budget)
            c.profile_reset()
            got = _run(c, names, batch)[1]
            rows = {k: v["launches"] for k, v in c.profile_report().items()}
            assert _same(whole, got), chunk
            assert rows == {k: -(-40 // chunk) for k in NEW_ROWS}, (chunk, rows)
    finally:
        c.profile_enable(False)
        c.set_lexicon_scratch(0)


@pytest.mark.parametrize("cfg", [(37, 2), (96, 2)], ids=_id)
def test_a_mixed_batch_equals_the_uniform_runs(recogniser, cfg):
    c, names = recogniser(*cfg)
    entries = pc.of_config(*cfg)
    logits = np.stack([p["case"]["logits"] for p in entries])
    of = np.array([-1 if i % 4 == 3 else names.index(p["pattern"]) for i, p in enumerate(entries)], np.int32)
    mixed = c.crnn_decode_logits_patterns(logits, of)
    for k in sorted(set(of.tolist())):
        rows = np.flatnonzero(of == k)
        if k < 0:
            assert (mixed[0][rows] == -1).all() and (mixed[1][rows] == -np.inf).all() and (mixed[2][rows] == -np.inf).all()
            continue
        c.set_pattern(k)
        try:
            uniform = c.crnn_decode_logits_patterns(logits)  # the context's switch
        finally:
            c.set_pattern(-1)
        assert _same([r[rows] for r in mixed], [r[rows] for r in uniform]), names[k]
    assert (of == -1).any()


@pytest.fixture(scope="module")
def plain37(recogniser):
    """37 classes, discard 2, sharpened; patterns: digits, letters+, code, any"""
    c, _ = recogniser(37, 2)
    c.load_crnn(_weights(37, True))
    pats = pc.kp.Patterns(pc.ALPHABETS[37], {"digits": r"\d*", "letters+": r"[a-z]+", "code": r"\d{2}[a-z]\d{2}", "eleven": r".{11}"})
    c.set_patterns(*pats.tables())
    yield c, pats
    c.set_patterns(None)
    c.load_crnn(_weights(37))


def _boxes(n, seed, h=96, w=128):
    rng = np.random.default_rng(seed)
    x0, y0 = rng.integers(0, w - 50, n), rng.integers(0, h - 20, n)
    bw, bh = rng.integers(20, 48, n), rng.integers(8, 18, n)
    return np.stack([np.array([[a, b], [a + p, b], [a + p, b + q], [a, b + q]], np.float32) for a, b, p, q in zip(x0, y0, bw, bh)])


def test_recognize_boxes_patterns_across_the_batch_edge(plain37):
    """1030 boxes with alternating patterns (and none): rows 1024 .. 1029 equal their own small-batch results, the label rows
    are those of the plain call"""
    c, pats = plain37
    page = synth.text_page(96, 128, 5, seed=21)[None]
    boxes = _boxes(1030, 71)
    of = (np.arange(1030) % 5 - 1).astype(np.int32)  # -1, 0, 1, 2, 3, -1, ...
    labels, plab, path, prob = c.recognize_boxes(page, [boxes], pattern_of=of)
    assert np.array_equal(labels, c.recognize_boxes(page, [boxes]))
    tail = c.recognize_boxes(page, [boxes[1024:]], pattern_of=of[1024:])
    assert _same((labels[1024:], plab[1024:], path[1024:], prob[1024:]), tail)
    assert np.isfinite(prob[1024:]).any() and (plab[of == -1] == -1).all() and (prob[of == -1] == -np.inf).all()
    for i in range(1030):
        if of[i] >= 0 and np.isfinite(prob[i]):
            assert pats.accepts(int(of[i]), plab[i][plab[i] >= 0].tolist()), i
    # kocr_crnn_pattern over the same edge, and against the seam on its own logits
    crops = c.warp_crops(page, [boxes])
    got = c.crnn_pattern(crops, of)
    assert _same([r[1024:] for r in got], c.crnn_pattern(crops[1024:], of[1024:]))
    c.crnn_set_taps(["ctc"])
    try:
        c.crnn_forward(crops[1024:])  # the batch the 1030-crop call runs them in
        logits = c.crnn_taps()["ctc"]["in"][0].reshape(6, T, 37)
    finally:
        c.crnn_set_taps([])
    assert _same([r[1024:] for r in got], c.crnn_decode_logits_patterns(logits, of[1024:]))
    assert _same((plab, path, prob), got)  # the two routes batch the crops alike
    c.set_pattern(2)
    try:
        assert _same(c.crnn_pattern(crops[1020:]), c.crnn_pattern(crops[1020:], np.full(10, 2)))
    finally:
        c.set_pattern(-1)


# ---- 3. the switch ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipe(plain37, craft_weights):
    import keras_ocr_amd
    from oracle import craft as ocraft
    from oracle import tools as otools

    c, _ = plain37
    page = synth.text_page(96, 128, 5, seed=21)[None]
    big = np.stack([otools.resize_image(p, 2, 2048)[0] for p in page])
    calibrated = keras_ocr_amd.weights.calibrate_craft_head(craft_weights, ocraft.detector_predict(craft_weights, big), text_frac=0.10,
                                                            link_frac=0.04)
    det = keras_ocr_amd.detection.Detector(weights=calibrated, ctx=c)
    rec = keras_ocr_amd.recognition.Recognizer(weights=_weights(37, True), ctx=c)
    rec.set_patterns({"digits": r"\d*", "letters+": r"[a-z]+", "code": r"\d{2}[a-z]\d{2}", "eleven": r".{11}"})
    return keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)


PAGES = [synth.text_page(96, 128, 5, seed=21), synth.text_page(96, 128, 6, seed=24)]


def _pipeline(c, **kw):
    ims = [np.ascontiguousarray(p) for p in PAGES]
    return c.pipeline(ims, [96, 96], [128, 128], [192, 192], [256, 256], 192, 256, **kw)


def test_the_switch_off_launches_and_returns_what_it_did(pipe):
    c = pipe.detector._ctx  # pylint: disable=protected-access
    tables = pipe.recognizer.patterns.tables()
    page = PAGES[0][None]
    boxes = [_boxes(7, 72)]

    def run(call):
        c.profile_reset()
        out = call()
        return out, {name: row["launches"] for name, row in c.profile_report().items()}

    def boxes_call(**kw):  # (labels, log_word, chars, beam labels, beam log_prob[, pattern labels, log_path, log_prob])
        out = c.recognize_boxes(page, boxes, return_scores=True, beam=(4, 2), **kw)
        return list(out[:5]), out[5:]

    def pipeline_call(**kw):  # (boxes, labels, scores[, pattern])
        out = _pipeline(c, return_scores=True, **kw)
        plain = [np.concatenate([np.asarray(b, np.float32).reshape(-1, 8) for b in out[0]]), out[1], np.concatenate(out[2][0]), *out[2][1:]]
        return plain, out[3] if len(out) > 3 else ()

    c.profile_enable(True)
    try:
        for call in (boxes_call, pipeline_call):
            c.set_patterns(None)
            (bare, none), bare_rows = run(call)
            c.set_patterns(*tables)
            assert c.get_pattern() == -1
            (off, none_off), off_rows = run(call)
            (on, (plab, path, prob)), on_rows = run(lambda: call(pattern=2))  # pylint: disable=cell-var-from-loop
            assert c.get_pattern() == -1 and len(none) == len(none_off) == 0
            assert _same(bare, off) and bare_rows == off_rows and not NEW_ROWS & set(off_rows), (bare_rows, off_rows)
            assert _same(bare, on), "the plain results are the same bits"
            assert {k: v for k, v in on_rows.items() if k not in NEW_ROWS} == off_rows
            assert {k: on_rows.get(k) for k in NEW_ROWS} == {k: 1 for k in NEW_ROWS}, on_rows
            assert len(plab) == len(path) == len(prob) == len(bare[1] if call is pipeline_call else bare[0]) >= 4
            assert np.isfinite(prob).any()
    finally:
        c.profile_enable(False)
        c.set_patterns(*tables)


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------

class _Foreign:
    """a detector that is not libkocr-backed as far as Pipeline can tell: the stage-wise route"""

    def __init__(self, detector):
        self._inner = detector

    def detect(self, images, **kwargs):
        return self._inner.detect(images=images, **kwargs)


def test_pipeline_passes_the_pattern_through(pipe):
    import keras_ocr_amd

    rec = pipe.recognizer
    assert rec.patterns.names == ["digits", "letters+", "code", "eleven"]
    for name in ("digits", "code", "letters+"):
        kw = {"pattern": name}
        regex = rec.patterns.regex[rec.patterns.names.index(name)]
        off = pipe.recognize(PAGES)
        on = pipe.recognize(PAGES, recognition_kwargs=kw)
        assert sum(len(p) for p in off) >= 4
        for a, b in zip(off, on):  # the same boxes
            assert len(a) == len(b) and all(np.array_equal(x[1], y[1]) for x, y in zip(a, b))
        words = [[w for w, _ in page] for page in on]
        fitted = [w for page in words for w in page if w[0] is not None]
        assert fitted and all(re.fullmatch(regex, t) and np.isfinite(v) and v <= 0 for t, v in fitted), name
        assert all(w == (None, -np.inf) for page in words for w in page if w[0] is None)
        # Detector.detect, then recognize_from_boxes on its boxes (detector-input pixels: the scale is 2)
        padded = [np.asarray(rec._ctx.resize_pad(p[None], (p.shape[1] * 2, p.shape[0] * 2))[0]) for p in PAGES]  # pylint: disable=protected-access
        groups = pipe.detector.detect(np.stack(padded))
        assert all(np.array_equal(np.asarray(g, np.float32).reshape(-1, 4, 2) / 2, np.array([b for _, b in page], np.float32).reshape(-1, 4, 2))
                   for g, page in zip(groups, on))
        assert rec.recognize_from_boxes(padded, groups, pattern=name) == words
        assert rec.recognize_from_boxes(padded, groups, pattern=[[name] * len(g) for g in groups]) == words
        mixed = rec.recognize_from_boxes(padded, groups, pattern=[[None if i % 2 else name for i in range(len(g))] for g in groups])
        assert mixed == [[(None, -np.inf) if i % 2 else w for i, w in enumerate(page)] for page in words]
        # the stage-wise route and the tiled one
        foreign = keras_ocr_amd.pipeline.Pipeline(detector=_Foreign(pipe.detector), recognizer=rec)
        staged = foreign.recognize(PAGES, recognition_kwargs=kw)
        assert [[w for w, _ in page] for page in staged] == words
        assert all(np.array_equal(x[1], y[1]) for a, b in zip(staged, on) for x, y in zip(a, b))
        tiled = pipe.recognize_tiled(PAGES, tile=128, overlap=32, recognition_kwargs=kw)
        tiled_off = pipe.recognize_tiled(PAGES, tile=128, overlap=32)
        for a, b, whole in zip(tiled_off, tiled, on):
            assert len(a) == len(b) and all(np.array_equal(x[1], y[1]) for x, y in zip(a, b))
            assert all(w == (None, -np.inf) or re.fullmatch(regex, w[0]) for w, _ in b)
            if len(b) == len(whole) and all(np.array_equal(x[1], y[1]) for x, y in zip(b, whole)):
                assert [w for w, _ in b] == [w for w, _ in whole]
        scored = pipe.recognize_with_scores(PAGES, recognition_kwargs=kw)
        assert [[w for w, _, _ in page] for page in scored] == words
    one = rec.recognize(np.ascontiguousarray(PAGES[0][:31]), pattern="digits")
    assert one == (None, -np.inf) or re.fullmatch(r"\d*", one[0])
    assert rec.recognize(np.ascontiguousarray(PAGES[0][:31]), pattern="digits", return_scores=True)[0] == one
    assert [[t for t, _ in page] for page in pipe.recognize(PAGES)] == [[t for t, _ in page] for page in off]  # off again
    assert rec._ctx.get_pattern() == -1  # pylint: disable=protected-access


def test_refusals(pipe):
    import keras_ocr_amd

    rec = pipe.recognizer
    c = rec._ctx  # pylint: disable=protected-access
    lib, h = c._lib, c._h  # pylint: disable=protected-access
    err = lambda: lib.kocr_last_error(h).decode()  # noqa: E731
    page = PAGES[0][None]
    boxes = [_boxes(5, 73)]
    crop = np.ascontiguousarray(PAGES[0][:31])
    tables = rec.patterns.tables()
    # Python: one reading per word; the pattern states the characters itself
    for kw in (dict(beam_width=4), dict(lexicon_top=2), dict(charset="digits"), dict(orientation="flip")):
        with pytest.raises(ValueError, match=f"pattern and {next(iter(kw))} cannot be combined"):
            rec.recognize_from_boxes(page, boxes, pattern="digits", **kw)
        with pytest.raises(ValueError, match="pattern"):
            pipe.recognize(PAGES, recognition_kwargs=dict(pattern="digits", **kw))
        if "orientation" not in kw:
            with pytest.raises(ValueError, match=f"pattern and {next(iter(kw))} cannot be combined"):
                rec.recognize(crop, pattern="digits", **kw)
    with pytest.raises(ValueError, match=r"unknown pattern 'iban'.*digits"):
        pipe.recognize(PAGES, recognition_kwargs={"pattern": "iban"})
    with pytest.raises(ValueError, match="one name for every box"):
        pipe.recognize(PAGES, recognition_kwargs={"pattern": ["digits"]})
    with pytest.raises(ValueError, match="pattern in recognition_kwargs makes every text"):
        pipe.recognize_lines(PAGES, recognition_kwargs={"pattern": "digits"})
    with pytest.raises(NotImplementedError, match="uint8"):
        rec.recognize_from_boxes(page.astype(np.float32), boxes, pattern="digits")
    with pytest.raises(NotImplementedError, match="uint8"):
        pipe.recognize([p.astype(np.float32) for p in PAGES], recognition_kwargs={"pattern": "digits"})
    with pytest.raises(NotImplementedError, match="pattern decodes across ranks"):
        keras_ocr_amd.dist.ShardedPipeline(pipe).recognize(PAGES, recognition_kwargs={"pattern": "digits"})
    with pytest.raises(ValueError, match=r"pattern 'p': the anchor"):
        rec.set_patterns({"p": "^a"})
    with pytest.raises(ValueError, match="cannot spell the character '/'"):
        rec.set_patterns({"date": r"\d{2}/\d{2}"})
    assert rec.patterns.names[0] == "digits" and c.pattern_count() == 4
    # the context
    with pytest.raises(ValueError, match="box 3 has pattern 4 outside"):
        c.recognize_boxes(page, boxes, pattern_of=[0, 1, -1, 4, 0])
    with pytest.raises(ValueError, match="box 0 has pattern -2"):
        c.recognize_boxes(page, boxes, pattern_of=[-2, 1, -1, 1, 0])
    with pytest.raises(ValueError, match="one pattern per box"):
        c.recognize_boxes(page, boxes, pattern_of=[0, 1])
    with pytest.raises(ValueError, match="crop 1 has pattern 9"):
        c.crnn_decode_logits_patterns(np.zeros((2, T, 37), np.float32), [0, 9])
    with pytest.raises(ValueError, match="no pattern is switched on"):
        c.crnn_decode_logits_patterns(np.zeros((2, T, 37), np.float32))
    with pytest.raises(ValueError, match="index 4 outside"):
        c.set_pattern(4)
    with pytest.raises(ValueError, match="orientation and pattern cannot be combined"):
        c.recognize_boxes(page, boxes, pattern=0, orientation=("flip", 1.5))
    assert c.get_pattern() == -1
    c.set_pattern(1)
    try:
        c.set_orientation(0)
        assert lib.kocr_set_orientation(h, 1, 1.5) == -1 and "cannot be combined with a pattern" in err()
        c.set_charsets(np.ones((1, 36), np.uint8))
        c.set_charset(0)
        with pytest.raises(Exception, match="active character set"):
            c.recognize_boxes(page, boxes)
        with pytest.raises(ValueError, match="active character set"):
            c.crnn_decode_logits_patterns(np.zeros((1, T, 37), np.float32))
        c.set_charsets(None)
        # a refused table changes nothing
        delta, accept, n = tables
        bad = delta.copy()
        bad[0, 0] = 99
        with pytest.raises(ValueError, match="pattern 0: state 0, class 0 moves to 99"):
            c.set_patterns(bad, accept, n)
        with pytest.raises(ValueError, match="classes 36 is not the recogniser's 37"):
            c.set_patterns(delta[:, :35], accept, n)
        with pytest.raises(ValueError, match="pattern 0 is not trimmed: state 0 reaches no accepting state"):
            c.set_patterns(delta, np.zeros_like(accept), n)
        with pytest.raises(ValueError, match="KOCR_PATTERNS_MAX"):
            c.set_patterns(np.zeros((65, 36), np.int32), np.ones(65, np.uint8), np.ones(65, np.int32))
        with pytest.raises(ValueError, match="257 states"):
            c.set_patterns(np.zeros((257, 36), np.int32), np.ones(257, np.uint8), [257])
        assert c.pattern_count() == 4 and c.get_pattern() == 1
        assert lib.kocr_set_patterns(h, None, None, None, 1, 37) == -1 and "null" in err()
        assert lib.kocr_set_patterns(None, None, None, None, 0, 0) == -1 and lib.kocr_pattern_count(None) == -1
        # results produced with the switch off, and none at all
        c.set_pattern(-1)
        c.recognize_boxes(page, boxes)
        with pytest.raises(ValueError, match="produced with the pattern off"):
            c.recognition_patterns()
        # loading a recogniser of another class count unloads the tables and switches off
        c.set_pattern(1)
        c.load_crnn(_weights(96))
        try:
            assert c.pattern_count() == 0 and c.get_pattern() == -1
            with pytest.raises(ValueError, match="no patterns are loaded"):
                c.crnn_decode_logits_patterns(np.zeros((1, T, 96), np.float32), [0])
        finally:
            c.load_crnn(_weights(37, True))
    finally:
        c.set_charsets(None)
        rec.set_patterns(dict(zip(rec.patterns.names, rec.patterns.regex)))
    assert c.pattern_count() == 4 and c.get_pattern() == -1
    fresh = keras_ocr_amd.Context(0)
    try:
        rc = lib.kocr_set_patterns(fresh._h, tables[0].ctypes.data, tables[1].ctypes.data, tables[2].ctypes.data, 4, 37)  # pylint: disable=protected-access
        assert rc == keras_ocr_amd._lib.KOCR_ENOWEIGHTS and "kocr_load_crnn" in lib.kocr_last_error(fresh._h).decode()  # pylint: disable=protected-access
        fresh.set_patterns(None)  # unloading needs no recogniser
    finally:
        fresh.close()
