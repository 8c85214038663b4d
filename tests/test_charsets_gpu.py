"""Character sets on the GPU ("Character sets"; csrc/crnn_kernels.hip: the MASKED instantiations of
ctc_kernel, ctc_scores_kernel, ctc_beam_kernel, lexicon_logq_kernel, lexicon_select_kernel) on the frozen (case, set) pairs of
tests/charset_cases.py.  tests/test_charset_statement_cpu.py shows with the float64 statement alone that every pair compared
here is decidable.

  1. statement     crnn_decode_logits(set_of=) against tests/charset_statement.py: rows and indices exact, floats within the
                   bounds of tests/test_decode_edges_gpu.py for the same quantities (its GATE and crnn_layer_check.check_ctc);
  2. kernels       the masked call on raw logits == the unconstrained call on logits with -inf written, bit for bit; set -1 ==
                   the call of today;
  3. independence  mixed sets in one batch (3 and 1024 crops) == the per-set uniform runs, row for row;
  4. batch edge    1030 crops through kocr_crnn_forward under the switch and through kocr_recognize_boxes_charsets with
                   alternating sets, the lexicon in several chunks;
  5. orientation   recognize_boxes(set_of=, orientation=) == crop stage, masked decode with each set twice, choice;
  6. pipeline      Pipeline.recognize / recognize_tiled / return_scores with recognition_kwargs={"charset": ...};
  7. launches      the profiler rows and launch counts of a masked and an unmasked kocr_recognize_boxes are the same;
  8. refusals."""
import functools

import numpy as np
import pytest

from tests import charset_cases as cc
from tests import charset_statement as st
from tests import crnn_layer_check as lc
from tests import decode_cases as dc
from tests import lexicon_statement as ls
from tests import scores_statement as ss
from tests import synth

pytestmark = pytest.mark.gpu

GATE = dc.GATE
T = dc.T


def _id(cfg):
    return f"C{cfg[0]}-d{cfg[1]}"


@functools.lru_cache(maxsize=None)
def _weights(classes):
    import keras_ocr_amd

    return keras_ocr_amd.weights.synthetic_crnn_weights(4321, n_classes=classes)


@pytest.fixture(scope="module")
def recogniser(ctx, crnn_weights):
    """at(classes, discard): the session's context with a recogniser of that many classes, that discard, lexicon(classes) and
    the sets of charset_cases.of_config(classes, discard) as sets 0 .. S - 1; returns (ctx, entries)"""
    state = {}

    def at(classes, discard):
        if state.get("classes") != classes:
            ctx.load_crnn(_weights(classes))
            ctx.set_lexicon(*dc.rows(dc.lexicon(classes)))
            state["classes"] = classes
        ctx.crnn_set_rnn_steps_to_discard(discard)
        entries = cc.of_config(classes, discard)
        ctx.set_charsets(cc.table(entries, classes))
        assert ctx.charset_count() == len(entries) and ctx.get_charset() == -1
        return ctx, entries

    yield at
    ctx.set_charsets(None)
    ctx.set_lexicon(None)
    ctx.set_lexicon_scratch(0)
    ctx.crnn_set_rnn_steps_to_discard(2)
    ctx.load_crnn(crnn_weights)


def _stack(entries):
    return np.stack([p["case"]["logits"] for p in entries])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _within_gate(got, want, frames):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    if not np.array_equal(got[~fin], want[~fin]):
        return False
    return bool((np.abs(got[fin] - want[fin]) <= GATE * frames * np.maximum(1.0, np.abs(want[fin]))).all())


def _written(entries):
    """the entries' logits with -inf written at the masked classes (float32)"""
    return np.stack([st.masked(p["case"]["logits"], p["set"]).astype(np.float32) for p in entries])


# ---- 1. against the statement ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", cc.CONFIGS, ids=_id)
def test_decode_scores_and_lexicon_equal_the_statement(recogniser, cfg):
    c, entries = recogniser(*cfg)
    frames, C = T - cfg[1], cfg[0]
    logits = _stack(entries)
    out = c.crnn_decode_logits(logits, return_probs=True, scores=True, top_words=dc.TOP_WORDS, return_values=True,
                               set_of=np.arange(len(entries)))
    words = dc.lexicon(C)
    needs = np.array([ls.frames_needed(w) for w in words])
    for i, p in enumerate(entries):
        lg = dc.decoded(p["case"])
        assert np.array_equal(out["labels"][i], st.greedy(lg, p["set"])), p["name"]
        outside = [k for k in range(C - 1) if k not in p["set"]]
        assert (out["probs"][i][:, outside] == 0).all(), p["name"]  # exactly 0
        worst, _ = lc.check_ctc(_written([p]), out["probs"][i:i + 1], cfg[1])
        assert worst <= 1.0, (p["name"], worst)
        assert np.array_equal(_bits(out["chars"][i]), _bits(ss.char_scores(out["probs"][i:i + 1])[0])), p["name"]
        assert _within_gate(out["log_word"][i:i + 1], [st.log_word(lg, p["set"])], frames), p["name"]
        want = cc.lexicon_values(p["name"])
        assert np.array_equal(np.isfinite(want), needs <= frames)
        assert _within_gate(out["lex_values"][i], want, frames), p["name"]  # a masked word stays finite: not removed
        if p["lexicon"]:
            want_i, want_p, _, _ = ls.top_words_ties(want[None], dc.TOP_WORDS)
            assert np.array_equal(out["lex_index"][i], want_i[0]), (p["name"], out["lex_index"][i], want_i[0])
            assert _within_gate(out["lex_log_prob"][i], want_p[0], frames), p["name"]
    assert sum(p["lexicon"] for p in entries) >= 3
    # the loss stays unmasked: the same bits with and without the sets
    rows, lengths = out["labels"], (out["labels"] >= 0).sum(-1)
    loss_args = dict(loss_labels=(rows, lengths, np.full(len(entries), frames)))
    assert np.array_equal(_bits(c.crnn_decode_logits(logits, set_of=np.arange(len(entries)), **loss_args)["loss"]),
                          _bits(c.crnn_decode_logits(logits, **loss_args)["loss"]))


BEAM_RUNS = [(cfg, pair) for cfg in cc.CONFIGS for pair in dc.BEAM_PAIRS if any(pair in p["beam"] for p in cc.of_config(*cfg))]


@pytest.mark.parametrize("cfg, pair", BEAM_RUNS, ids=lambda v: _id(v) if v in cc.CONFIGS else f"B{v[0]}-K{v[1]}")
def test_beam_equals_the_statement(recogniser, cfg, pair):
    """rows equal the statement's (the saturated crops: row 0, as tests/test_decode_edges_gpu.py judges them), values within
    the gate, every label in the set, log_prob == -loss of the row on the -inf-written logits bit for bit"""
    c, every = recogniser(*cfg)
    sets = [i for i, p in enumerate(every) if pair in p["beam"]]
    entries = [every[i] for i in sets]
    frames = T - cfg[1]
    logits = _stack(entries)
    out = c.crnn_decode_logits(logits, beam=pair, set_of=sets)
    labels, log_prob = out["beam_labels"], out["beam_log_prob"]
    assert labels.shape == (len(entries), pair[1], frames)
    for i, p in enumerate(entries):
        want_l, want_p, _ = cc.beam(p["name"], *pair)
        rows = slice(0, 1) if p["judge"] == "lead" else slice(None)
        assert np.array_equal(labels[i, rows], want_l[rows]), (p["name"], pair, labels[i, :3, :12], want_l[:3, :12])
        assert _within_gate(log_prob[i, rows], want_p[rows], frames), (p["name"], pair, log_prob[i, :3], want_p[:3])
        assert set(labels[i][labels[i] >= 0].tolist()) <= set(p["set"]), p["name"]
        if p["kind"] in ("all", "word") and p["judge"] == "lead":  # the set holds the word: the best path is the decode
            assert np.array_equal(labels[i, 0], out["labels"][i]), p["name"]
    written = _written(entries)
    lengths = (labels >= 0).sum(-1)
    for j in range(pair[1]):
        there = log_prob[:, j] != -np.inf
        assert (lengths[~there, j] == 0).all()
        if there.any():
            loss = c.crnn_decode_logits(written[there], loss_labels=(labels[there, j], lengths[there, j], np.full(int(there.sum()), frames)))["loss"]
            assert np.array_equal(_bits(log_prob[there, j]), _bits(-loss))


# ---- 2. against the kernels themselves -------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", cc.CONFIGS, ids=_id)
def test_masked_call_equals_the_unconstrained_call_on_written_logits(recogniser, cfg):
    c, entries = recogniser(*cfg)
    logits, written = _stack(entries), _written(entries)
    assert np.isinf(written).any() and np.isfinite(logits).all()
    sets = np.arange(len(entries))
    kwargs = dict(return_probs=True, scores=True, top_words=dc.ALL_WORDS, return_values=True)
    assert _same(c.crnn_decode_logits(logits, set_of=sets, **kwargs), c.crnn_decode_logits(written, **kwargs))
    plain = c.crnn_decode_logits(logits, return_probs=True)  # ctc_kernel, without the scores
    assert _same(c.crnn_decode_logits(logits, return_probs=True, set_of=sets), c.crnn_decode_logits(written, return_probs=True))
    assert not np.array_equal(plain["labels"], c.crnn_decode_logits(logits, set_of=sets)["labels"])
    compared = 0
    for pair in dc.BEAM_PAIRS:  # the beam whenever beam_width <= |A|: both sides then extend by the same classes
        sel = [i for i, p in enumerate(entries) if pair[0] <= len(p["set"]) and pair in p["beam"]]
        if sel:
            compared += len(sel)
            assert _same(c.crnn_decode_logits(logits[sel], beam=pair, set_of=sets[sel]), c.crnn_decode_logits(written[sel], beam=pair)), pair
    assert compared >= 4
    # set -1, and the switch at -1 with a table loaded: the call of today, bit for bit
    full = dict(kwargs, beam=(16, 3) if cfg[1] != 40 else (64, 3))
    today = c.crnn_decode_logits(logits, **full)
    assert _same(c.crnn_decode_logits(logits, set_of=np.full(len(entries), -1), **full), today)
    for kind in ("all", "miss"):  # the uniform switch: the per-crop list with one set; all classes allowed: today's bits
        s = next(i for i, p in enumerate(entries) if p["kind"] == kind)
        c.set_charset(s)
        try:
            uniform = c.crnn_decode_logits(logits, **full)
            assert _same(uniform, c.crnn_decode_logits(logits, set_of=np.full(len(entries), s), **full))
        finally:
            c.set_charset(-1)
        assert _same(uniform, today) == (kind == "all")
    assert _same(c.crnn_decode_logits(logits, **full), today)
    c.set_charsets(None)
    assert _same(c.crnn_decode_logits(logits, **full), today)  # ... and without a table


# ---- 3. independence -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [3, 1024])
def test_a_mixed_batch_equals_the_per_set_runs(recogniser, m):
    c, entries = recogniser(96, 2)
    S = len(entries)
    rng = np.random.default_rng(50 + m)
    which = rng.integers(0, S, m)
    sets = rng.integers(-1, S, m).astype(np.int32)
    if m == 3:
        sets[:] = [S - 1, -1, 0]
    logits = _stack(entries)[which]
    kwargs = dict(return_probs=m == 3, scores=True, beam=(16, 3), top_words=3, return_values=True)
    mixed = c.crnn_decode_logits(logits, set_of=sets, **kwargs)
    assert len(set(sets.tolist())) == (3 if m == 3 else S + 1)
    try:
        for s in sorted(set(sets.tolist())):
            c.set_charset(s)
            rows = np.flatnonzero(sets == s)
            uniform = c.crnn_decode_logits(logits, **kwargs)  # the whole batch under one set: the rows of that set
            assert _same({k: v[rows] for k, v in mixed.items()}, {k: v[rows] for k, v in uniform.items()}), s
            if m == 3:
                alone = c.crnn_decode_logits(logits[rows], **kwargs)
                assert _same({k: v[rows] for k, v in mixed.items()}, alone), s
    finally:
        c.set_charset(-1)


# ---- 4. the 1024-crop batch edge -------------------------------------------------------------------------------------------

DIGITS = tuple(range(10))
LETTERS = tuple(range(10, 36))


@pytest.fixture(scope="module")
def plain37(recogniser):
    """37 classes, discard 2, sharpened like the orientation tests' recogniser so that decodes are not empty; sets: digits,
    letters"""
    c, _ = recogniser(37, 2)
    w = dict(_weights(37))
    w["fc_12/kernel"] = w["fc_12/kernel"] * np.float32(2)
    w["fc_12/bias"] = w["fc_12/bias"] * np.float32(2)
    c.load_crnn(w)
    allowed = np.zeros((2, 36), np.uint8)
    allowed[0, list(DIGITS)] = 1
    allowed[1, list(LETTERS)] = 1
    c.set_charsets(allowed)
    yield c
    c.set_charsets(None)
    c.load_crnn(_weights(37))


def _boxes(n, seed, h=96, w=128):
    rng = np.random.default_rng(seed)
    x0, y0 = rng.integers(0, w - 50, n), rng.integers(0, h - 20, n)
    bw, bh = rng.integers(20, 48, n), rng.integers(8, 18, n)
    return np.stack([np.array([[a, b], [a + p, b], [a + p, b + q], [a, b + q]], np.float32) for a, b, p, q in zip(x0, y0, bw, bh)])


def test_crnn_forward_under_the_switch_across_the_batch_edge(plain37):
    c = plain37
    page = synth.text_page(96, 128, 5, seed=21)
    crops = c.warp_crops(page[None], [_boxes(1030, 60)])
    off, off_probs = c.crnn_forward(crops, return_probs=True)
    c.set_charset(0)
    try:
        labels, probs = c.crnn_forward(crops, return_probs=True)
        tail, tail_probs = c.crnn_forward(crops[1024:], return_probs=True)
        scored = c.crnn_forward_scores(crops)
        beams = c.crnn_beam(crops[1020:], 4, 2)
    finally:
        c.set_charset(-1)
    assert labels.shape == (1030, 48) and set(labels[labels >= 0].tolist()) <= set(DIGITS) and (labels[1024:] >= 0).any()
    assert (probs[..., list(LETTERS)] == 0).all() and (off_probs[..., list(LETTERS)] > 0).any()
    assert np.array_equal(labels[1024:], tail) and np.array_equal(_bits(probs[1024:]), _bits(tail_probs))
    assert not np.array_equal(labels[1024:], off[1024:])
    assert np.array_equal(scored[0], labels) and set(beams[0][beams[0] >= 0].tolist()) <= set(DIGITS)
    after, after_probs = c.crnn_forward(crops, return_probs=True)
    assert np.array_equal(after, off) and np.array_equal(_bits(after_probs), _bits(off_probs))  # off again: as before


def test_recognize_boxes_charsets_across_the_batch_edge(plain37):
    """1030 boxes with alternating sets, scores and a lexicon match in chunks of 100 crops: every row equals the row of the
    uniform run under its own set -- rows 1024 .. 1029 included"""
    c = plain37
    page = synth.text_page(96, 128, 5, seed=21)[None]
    boxes = [_boxes(1030, 61)]
    sets = (np.arange(1030) % 3 - 1).astype(np.int32)  # -1, 0, 1, -1, ...
    c.set_lexicon_scratch(4 * c.lexicon_size() * 100)
    try:
        mixed = c.recognize_boxes(page, boxes, return_scores=True, lexicon_top=2, set_of=sets)
        for s in (-1, 0, 1):
            c.set_charset(s)
            uniform = c.recognize_boxes(page, boxes, return_scores=True, lexicon_top=2)
            rows = np.flatnonzero(sets == s)
            assert (rows >= 1024).any()
            for got, want in zip(mixed, uniform):
                assert np.array_equal(_bits(got[rows]), _bits(want[rows])), s
            if s >= 0:
                assert set(uniform[0][uniform[0] >= 0].tolist()) <= set((DIGITS, LETTERS)[s])
        c.set_charset(-1)
        off = c.recognize_boxes(page, boxes, return_scores=True, lexicon_top=2)
        assert any(not np.array_equal(_bits(a[1024:]), _bits(b[1024:])) for a, b in zip(mixed, off))
        assert np.array_equal(off[0], c.recognize_boxes(page, boxes))
    finally:
        c.set_charset(-1)
        c.set_lexicon_scratch(0)


# ---- 5. orientation --------------------------------------------------------------------------------------------------------

def test_orientation_reads_both_candidates_under_the_box_set(plain37):
    c = plain37
    page = synth.text_page(96, 128, 5, seed=21)[None]
    boxes = [_boxes(9, 62)]
    sets = np.array([0, 1, -1, 1, 0, 0, -1, 1, 1], np.int32)
    labels, log_word, chars, turns, quads, pairs = c.recognize_boxes(page, boxes, return_scores=True, orientation=("flip", 1.5), set_of=sets)
    crops, turns2, quads2 = c.warp_crops_turned(page, boxes, "flip")
    c.crnn_set_taps(["ctc"])
    try:
        c.crnn_forward(crops)
        logits = c.crnn_taps()["ctc"]["in"][0].reshape(len(crops), T, 37)
    finally:
        c.crnn_set_taps([])
    both = c.crnn_decode_logits(logits, scores=True, set_of=np.repeat(sets, 2))
    want = c.orient_select(both["labels"].reshape(9, 2, 48), both["log_word"].reshape(9, 2), both["chars"].reshape(9, 2, 48),
                           turns2.reshape(9, 2), quads2.reshape(9, 2, 4, 2))
    for got, exp in zip((labels, log_word, chars, turns, quads, pairs), want):
        assert np.array_equal(_bits(got), _bits(exp))
    for i, s in enumerate(sets):
        if s >= 0:
            assert set(labels[i][labels[i] >= 0].tolist()) <= set((DIGITS, LETTERS)[s])
    off = c.recognize_boxes(page, boxes, return_scores=True, orientation=("flip", 1.5))
    assert not np.array_equal(off[0], labels)


# ---- 6. pipeline -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipe(plain37, craft_weights):
    import keras_ocr_amd
    from oracle import craft as ocraft
    from oracle import tools as otools

    page = synth.text_page(96, 128, 5, seed=21)[None]
    big = np.stack([otools.resize_image(p, 2, 2048)[0] for p in page])
    calibrated = keras_ocr_amd.weights.calibrate_craft_head(craft_weights, ocraft.detector_predict(craft_weights, big), text_frac=0.10,
                                                            link_frac=0.04)
    w = dict(_weights(37))
    w["fc_12/kernel"] = w["fc_12/kernel"] * np.float32(2)
    w["fc_12/bias"] = w["fc_12/bias"] * np.float32(2)
    det = keras_ocr_amd.detection.Detector(weights=calibrated, ctx=plain37)
    rec = keras_ocr_amd.recognition.Recognizer(weights=w, ctx=plain37)
    rec.set_charsets({"digits": "0123456789", "letters": "abcdefghijklmnopqrstuvwxyz"})
    return keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)


def test_pipeline_passes_the_charset_through(pipe):
    rec = pipe.recognizer
    assert rec.charsets == ["digits", "letters"]
    pages = [synth.text_page(96, 128, 5, seed=21), synth.text_page(96, 128, 6, seed=24)]
    digits = {"charset": "digits"}
    off = pipe.recognize(pages)
    on = pipe.recognize(pages, recognition_kwargs=digits)
    assert sum(len(p) for p in off) >= 4
    groups = [np.array([b for _, b in page], np.float32).reshape(-1, 4, 2) for page in on]
    for a, b in zip(off, on):  # the same boxes
        assert len(a) == len(b) and all(np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    texts = [[t for t, _ in page] for page in on]
    assert texts != [[t for t, _ in page] for page in off]
    assert all(set(t) <= set("0123456789") for page in texts for t in page) and any(t for page in texts for t in page)
    # ... the texts of recognize_from_boxes on the detector's own boxes (detector-input pixels: the scale is 2)
    padded = [np.asarray(pipe.detector._ctx.resize_pad(p[None], (p.shape[1] * 2, p.shape[0] * 2))[0]) for p in pages]  # pylint: disable=protected-access
    scaled = [g * 2 for g in groups]
    assert rec.recognize_from_boxes(padded, scaled, charset="digits") == texts
    per_box = [["digits"] * len(g) for g in scaled]
    assert rec.recognize_from_boxes(padded, scaled, charset=per_box) == texts
    mixed = [[None if i % 2 else "digits" for i in range(len(g))] for g in scaled]
    free = rec.recognize_from_boxes(padded, scaled)
    assert rec.recognize_from_boxes(padded, scaled, charset=mixed) == [[f if i % 2 else t for i, (t, f) in enumerate(zip(ts, fs))]
                                                                     for ts, fs in zip(texts, free)]
    # scores, lines, tiles: the same texts
    scored = pipe.recognize_with_scores(pages, recognition_kwargs=digits)
    assert [[t for t, _, _ in page] for page in scored] == texts
    tiled = pipe.recognize_tiled(pages, tile=128, overlap=32, recognition_kwargs=digits)
    tiled_off = pipe.recognize_tiled(pages, tile=128, overlap=32)
    for a, b in zip(tiled_off, tiled):
        assert len(a) == len(b) and all(np.array_equal(x[1], y[1]) for x, y in zip(a, b))
    assert all(set(t) <= set("0123456789") for page in tiled for t, _ in page)
    tiled_scored = pipe.recognize_tiled(pages, tile=128, overlap=32, recognition_kwargs=digits, return_scores=True)
    assert [[w[0] for w in page] for page in tiled_scored] == [[t for t, _ in page] for page in tiled]
    assert set(rec.recognize(np.ascontiguousarray(pages[0][:31]), charset="digits")) <= set("0123456789")
    assert [[t for t, _ in page] for page in pipe.recognize(pages)] == [[t for t, _ in page] for page in off]  # off again: as before
    assert rec._ctx.get_charset() == -1  # pylint: disable=protected-access
    with pytest.raises(ValueError, match=r"unknown character set 'hex'.*digits"):
        pipe.recognize(pages, recognition_kwargs={"charset": "hex"})
    with pytest.raises(ValueError, match="'A'"):
        rec.set_charsets({"upper": "ABC"})
    assert rec.charsets == ["digits", "letters"] and rec._ctx.charset_count() == 2  # pylint: disable=protected-access
    rec.set_charsets({"upper": "ABC"}, lowercase=True)
    assert rec.charsets == ["upper"] and set("".join(t for page in pipe.recognize(pages, recognition_kwargs={"charset": "upper"})
                                                     for t, _ in page)) <= set("abc")
    rec.set_charsets({"digits": "0123456789", "letters": "abcdefghijklmnopqrstuvwxyz"})


# ---- 7. no extra launch ----------------------------------------------------------------------------------------------------

def test_a_masked_run_launches_what_an_unmasked_run_launches(plain37):
    c = plain37
    page = synth.text_page(96, 128, 5, seed=21)[None]
    boxes = [_boxes(7, 63)]

    def launches(**kw):
        c.profile_reset()
        c.recognize_boxes(page, boxes, **kw)
        return {name: row["launches"] for name, row in c.profile_report().items()}

    c.profile_enable(True)
    try:
        for kw in (dict(), dict(return_scores=True, beam=(4, 2)), dict(return_scores=True, lexicon_top=2)):
            off = launches(**kw)
            c.set_charset(1)
            on = launches(**kw)
            c.set_charset(-1)
            per_box = launches(set_of=np.array([0, 1, -1, 0, 1, -1, 0], np.int32), **kw)
            assert on == off and per_box == off, (kw, off, on, per_box)
            assert "ctc_scores" in off or "ctc_greedy" in off
        assert {"ctc_scores", "lexicon_logq", "lexicon_score", "lexicon_select"} <= set(off)
    finally:
        c.set_charset(-1)
        c.profile_enable(False)


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals(plain37):
    import keras_ocr_amd

    c = plain37
    KOCR_ENOWEIGHTS = keras_ocr_amd._lib.KOCR_ENOWEIGHTS  # pylint: disable=protected-access
    lib, h = c._lib, c._h  # pylint: disable=protected-access
    err = lambda: lib.kocr_last_error(h).decode()  # noqa: E731
    page = synth.text_page(96, 128, 5, seed=21)[None]
    boxes = [_boxes(5, 64)]
    with pytest.raises(ValueError, match="box 3 has set 2 outside"):
        c.recognize_boxes(page, boxes, set_of=[0, 1, -1, 2, 0])
    with pytest.raises(ValueError, match="box 0 has set -2"):
        c.recognize_boxes(page, boxes, set_of=[-2, 1, -1, 1, 0])
    with pytest.raises(ValueError, match="one character set per box"):
        c.recognize_boxes(page, boxes, set_of=[0, 1])
    with pytest.raises(ValueError, match="crop 1 has set 5"):
        c.crnn_decode_logits(np.zeros((2, T, 37), np.float32), set_of=[0, 5])
    with pytest.raises(ValueError, match="set 2 outside"):
        c.set_charset(2)
    with pytest.raises(ValueError, match="set -2 outside"):
        c.set_charset(-2)
    assert c.get_charset() == -1
    # a refused table changes nothing
    c.set_charset(1)
    two = np.zeros((2, 36), np.uint8)
    two[0, 3] = 1
    with pytest.raises(ValueError, match="set 1 is empty"):
        c.set_charsets(two)
    with pytest.raises(ValueError, match="classes 36 is not the recogniser's 37"):
        c.set_charsets(np.ones((1, 35), np.uint8))
    with pytest.raises(ValueError, match="KOCR_CHARSETS_MAX"):
        c.set_charsets(np.ones((257, 36), np.uint8))
    assert c.charset_count() == 2 and c.get_charset() == 1
    assert lib.kocr_set_charsets(h, None, 1, 37) == -1 and "null" in err()
    assert lib.kocr_set_charsets(None, None, 0, 0) == -1 and lib.kocr_charset_count(None) == -1
    c.set_charsets(np.ones((256, 36), np.uint8))  # the most there may be; a new table switches off
    assert c.charset_count() == 256 and c.get_charset() == -1
    # loading a recogniser of another class count unloads the table and switches off
    c.set_charset(255)
    c.load_crnn(_weights(96))
    try:
        assert c.charset_count() == 0 and c.get_charset() == -1
        with pytest.raises(ValueError, match="set 0 outside"):
            c.set_charset(0)
        with pytest.raises(ValueError, match="crop 0 has set 0"):
            c.crnn_decode_logits(np.zeros((1, T, 96), np.float32), set_of=[0])
        assert c.crnn_decode_logits(np.zeros((1, T, 96), np.float32), set_of=[-1])["labels"].shape == (1, 48)
    finally:
        w = dict(_weights(37))
        w["fc_12/kernel"] = w["fc_12/kernel"] * np.float32(2)
        w["fc_12/bias"] = w["fc_12/bias"] * np.float32(2)
        c.load_crnn(w)
        allowed = np.zeros((2, 36), np.uint8)
        allowed[0, list(DIGITS)] = 1
        allowed[1, list(LETTERS)] = 1
        c.set_charsets(allowed)
    fresh = keras_ocr_amd.Context(0)
    try:
        rc = lib.kocr_set_charsets(fresh._h, allowed.ctypes.data, 2, 37)  # pylint: disable=protected-access
        assert rc == KOCR_ENOWEIGHTS and "kocr_load_crnn" in lib.kocr_last_error(fresh._h).decode()  # pylint: disable=protected-access
        fresh.set_charsets(None)  # unloading needs no recogniser
    finally:
        fresh.close()
