"""CPU suite: the shapes of everything Pipeline returns, for every combination of optional results it accepts --
{scores on / off} x {neither, beam, lexicon} x {characters on / off} -- over its three routes: the fused one (a double of
``Context.pipeline``), the stage-wise one (duck-typed detector and recogniser) and the one for zero images.  Public
methods only: tuple lengths, where the Nones are, every array's shape and dtype, and the assembled values."""
import itertools
import math
import re

import numpy as np
import pytest

import keras_ocr_amd as k
from keras_ocr_amd import layout, lexicon as lexicon_module, scores as scores_module
from keras_ocr_amd.results import Results
from keras_ocr_amd.scores import Score

ALPHABET = k.recognition.DEFAULT_ALPHABET
WORDS = ["ab", "c", "cab"]
K = 2                                        # top_paths / lexicon_top
SHAPES = [(10, 20), (11, 22), (12, 24)]      # page i has h % 3 words: 1, 2, 0
SCALE = 2
COMBOS = list(itertools.product((False, True), (None, "beam", "lexicon"), (False, True)))


def _truth():
    """Per page a list of words; every number is a multiple of 1/8, so float32 holds it exactly."""
    pages, r = [], 0
    for h, w in SHAPES:
        words = []
        for j in range(h % 3):
            text = ALPHABET[h % 36] + ALPHABET[j]
            box = np.array([[0, 0], [SCALE * w, 0], [SCALE * w, SCALE * h], [0, SCALE * h]], np.float32) + j  # detector-input px
            last = r == 2
            words.append({
                "text": text, "box": box, "detection": 0.5 + 0.125 * j, "log_word": -0.25 * (r + 1), "chars": [0.875, 0.75],
                "beam": [(text, -0.5 * (r + 1))] + ([] if last else [(text + "z", -0.5 * (r + 1) - 1)]),
                "lexicon": [(WORDS[r % 3], -0.125 * (r + 1))] + ([] if last else [(WORDS[(r + 1) % 3], -0.125 * (r + 1) - 2)]),
                "characters": (np.stack([box, box + 8]), np.array([0.5, 0.75], np.float32)),
            })
            r += 1
        pages.append(words)
    return pages


TRUTH = _truth()
ROWS = [word for page in TRUTH for word in page]
M = len(ROWS)


def _label_row(text, width=48):
    row = np.full(width, -1, np.int32)
    row[:len(text)] = [ALPHABET.index(c) for c in text]
    return row


class _Context:
    """``Context.pipeline`` as the library answers it: ``(boxes, labels[, scores][, beam | lexicon][, characters])``."""

    def __init__(self):
        self.seen = []

    def pipeline(self, images, hs, ws, dhs, dws, hmax, wmax, micro_batch=0, on_device=False, return_scores=False, beam=None,
                 lexicon_top=None, char_boxes=None, **kw):
        assert [(int(h), int(w)) for h, w in zip(hs, ws)] == SHAPES and list(dhs) == [SCALE * h for h, _ in SHAPES]
        self.seen.append({"return_scores": return_scores, "beam": beam, "lexicon_top": lexicon_top, "char_boxes": char_boxes})
        boxes = [np.stack([w["box"] for w in page]) if page else np.array([]) for page in TRUTH]
        out = [boxes, np.stack([_label_row(w["text"]) for w in ROWS])]
        if return_scores:
            chars = np.zeros((M, 48), np.float32)
            chars[:, :2] = [w["chars"] for w in ROWS]
            out.append(([np.array([w["detection"] for w in page], np.float32) for page in TRUTH],
                        np.array([w["log_word"] for w in ROWS], np.float32), chars))
        if lexicon_top is not None:
            index, log_prob = np.full((M, lexicon_top), -1, np.int32), np.full((M, lexicon_top), -np.inf, np.float32)
            for r, w in enumerate(ROWS):
                for j, (word, value) in enumerate(w["lexicon"]):
                    index[r, j], log_prob[r, j] = WORDS.index(word), value
            out.append((index, log_prob))
        elif beam is not None:
            labels, log_prob = np.full((M, beam[1], 48), -1, np.int32), np.full((M, beam[1]), -np.inf, np.float32)
            for r, w in enumerate(ROWS):
                for j, (text, value) in enumerate(w["beam"]):
                    labels[r, j], log_prob[r, j] = _label_row(text), value
            out.append((labels, log_prob))
        if char_boxes:
            out.append([[w["characters"] for w in page] for page in TRUTH])
        return tuple(out)


class _Detector:
    """A duck-typed detector: no libkocr context, so Pipeline takes the stage-wise route."""

    def detect(self, images, return_scores=False, char_boxes=None, **kw):
        assert images.shape == (len(SHAPES), SCALE * 12, SCALE * 24, 3)
        out = ([np.stack([w["box"] for w in page]) if page else np.array([]) for page in TRUTH],)
        if return_scores:
            out += ([np.array([w["detection"] for w in page], np.float32) for page in TRUTH],)
        if char_boxes:
            out += ([[layout.Characters(*w["characters"]) for w in page] for page in TRUTH],)
        return out if len(out) > 1 else out[0]


class _DetectorWithoutCharacters:
    def detect(self, images, return_scores=False, **kw):
        raise AssertionError("refused before it is called")


class _Recognizer:
    alphabet = ALPHABET
    lexicon = lexicon_module.Lexicon(WORDS, ALPHABET)

    def recognize_from_boxes(self, images, box_groups, return_scores=False, beam_width=None, top_paths=1, lexicon_top=None):
        assert [len(b) for b in box_groups] == [len(page) for page in TRUTH]
        if beam_width is not None:
            assert top_paths == K
            return [[list(w["beam"]) for w in page] for page in TRUTH]
        if lexicon_top is not None:
            return [[list(w["lexicon"]) for w in page] for page in TRUTH]
        if return_scores:
            return [[(w["text"], _score(w, detection=False)) for w in page] for page in TRUTH]
        return [[w["text"] for w in page] for page in TRUTH]


def _score(w, detection=True):
    return scores_module.Score(w["detection"] if detection else None, math.exp(w["log_word"]), w["log_word"],
                               np.array(w["chars"], np.float32))


def _fused():
    det = object.__new__(k.detection.Detector)
    rec = object.__new__(k.recognition.Recognizer)
    det._ctx = rec._ctx = _Context()  # pylint: disable=protected-access
    rec.alphabet, rec.blank_label_idx, rec.lexicon = ALPHABET, len(ALPHABET), lexicon_module.Lexicon(WORDS, ALPHABET)
    return k.pipeline.Pipeline(detector=det, recognizer=rec, scale=SCALE, max_size=2048)


def _stagewise(monkeypatch):
    # tools.resize_image runs on the GPU; nothing here depends on its pixels
    monkeypatch.setattr(k.tools, "resize_image", lambda image, max_scale, max_size: (
        np.zeros((image.shape[0] * max_scale, image.shape[1] * max_scale, 3), np.uint8), max_scale))
    return k.pipeline.Pipeline(detector=_Detector(), recognizer=_Recognizer(), scale=SCALE, max_size=2048)


def _pages():
    return [np.zeros((h, w, 3), np.uint8) for h, w in SHAPES]


def _kwargs(kind):
    return {None: None, "beam": {"beam_width": 4, "top_paths": K}, "lexicon": {"lexicon_top": K}}[kind]


def _same(a, b):
    """Equality of nested tuples / lists / arrays, array dtypes and shapes included."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape \
            and np.array_equal(a, b)
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b and type(a) is type(b)


def _texts(kind, pages):
    """What stands in the place of ``text`` for every word"""
    return [[w["text"] if kind is None else list(w[kind]) for w in page] for page in pages]


def _expected(kind, pages, with_scores=False, with_characters=False):
    """The assembled result: per page ``(text | alternatives, box[, score | characters])``, boxes in input-image pixels"""
    out = []
    for page, texts in zip(pages, _texts(kind, pages)):
        rows = []
        for w, text in zip(page, texts):
            row = (text, w["box"] * np.float32(1 / SCALE))
            if with_scores:
                row += (_score(w),)
            if with_characters:
                row += (layout.Characters(w["characters"][0] * np.float32(1 / SCALE), w["characters"][1]),)
            rows.append(row)
        out.append(rows)
    return out


# length of recognize_raw's result and the positions that hold None, before the characters
LAYOUT = {(False, None): (2, ()), (True, None): (3, ()), (False, "beam"): (4, (2,)), (True, "beam"): (4, ()),
          (False, "lexicon"): (5, (2, 3)), (True, "lexicon"): (5, (3,))}


def _check_raw(pipe, out, with_scores, kind, with_characters, pages):
    rows = [w for page in pages for w in page]
    m = len(rows)
    length, nones = LAYOUT[with_scores, kind]
    assert isinstance(out, tuple) and len(out) == length + with_characters
    assert tuple(i for i, v in enumerate(out) if v is None) == nones
    boxes, labels = out[:2]
    assert isinstance(boxes, list) and len(boxes) == len(pages)
    for group, page in zip(boxes, pages):
        if page:
            assert group.dtype == np.float32 and group.shape == (len(page), 4, 2)
        else:
            assert group.dtype == np.float64 and group.shape == (0,)   # np.array([]) through adjust_boxes
    assert labels.dtype == np.int32 and labels.shape == (m, 48)
    if with_scores:
        detection, log_word, chars = out[2]
        assert isinstance(detection, list) and [(d.dtype, d.shape) for d in detection] == [(np.float32, (len(p),)) for p in pages]
        assert (log_word.dtype, log_word.shape, chars.dtype, chars.shape) == (np.float32, (m,), np.float32, (m, 48))
    if kind == "beam":
        beam_labels, beam_log_prob = out[3]
        assert (beam_labels.dtype, beam_labels.shape) == (np.int32, (m, K, 48))
        assert (beam_log_prob.dtype, beam_log_prob.shape) == (np.float32, (m, K))
    if kind == "lexicon":
        index, log_prob = out[4]
        assert (index.dtype, index.shape, log_prob.dtype, log_prob.shape) == (np.int32, (m, K), np.float32, (m, K))
    if with_characters:
        characters = out[-1]
        assert isinstance(characters, list) and [len(page) for page in characters] == [len(page) for page in pages]
        for c in (c for page in characters for c in page):
            assert isinstance(c, layout.Characters)
            assert (c.boxes.dtype, c.boxes.shape, c.scores.dtype, c.scores.shape) == (np.float32, (2, 4, 2), np.float32, (2,))
    assembled = pipe.assemble(*out[:length])
    assert _same(assembled, _expected(kind, pages, with_scores))
    if with_characters:
        want = _expected(kind, pages, with_characters=True)
        assert _same([[c for c in page] for page in out[-1]], [[row[-1] for row in page] for page in want])


@pytest.mark.parametrize("with_scores,kind,with_characters", COMBOS)
def test_fused_route(with_scores, kind, with_characters):
    pipe = _fused()
    out = pipe.recognize_raw(_pages(), None, None, None, _kwargs(kind), with_scores, char_boxes=True if with_characters else None)
    _check_raw(pipe, out, with_scores, kind, with_characters, TRUTH)
    seen, = pipe.detector._ctx.seen  # pylint: disable=protected-access
    assert seen["return_scores"] == with_scores and bool(seen["char_boxes"]) == with_characters
    assert seen["beam"] == ((4, K) if kind == "beam" else None) and seen["lexicon_top"] == (K if kind == "lexicon" else None)


@pytest.mark.parametrize("with_scores,kind,with_characters", COMBOS)
def test_stagewise_route(monkeypatch, with_scores, kind, with_characters):
    pipe = _stagewise(monkeypatch)
    out = pipe.recognize_raw(_pages(), None, None, None, _kwargs(kind), with_scores, char_boxes=True if with_characters else None)
    _check_raw(pipe, out, with_scores, kind, with_characters, TRUTH)


@pytest.mark.parametrize("with_scores,kind,with_characters", COMBOS)
def test_zero_images_route(with_scores, kind, with_characters):
    pipe = _fused()
    out = pipe.recognize_raw([], None, None, None, _kwargs(kind), with_scores, char_boxes=True if with_characters else None)
    _check_raw(pipe, out, with_scores, kind, with_characters, [])
    assert pipe.detector._ctx.seen == []  # pylint: disable=protected-access


@pytest.mark.parametrize("route", ["fused", "stagewise", "zero"])
@pytest.mark.parametrize("kind", [None, "beam", "lexicon"])
def test_public_methods(monkeypatch, route, kind):
    pipe = _stagewise(monkeypatch) if route == "stagewise" else _fused()
    images, pages = ([], []) if route == "zero" else (_pages(), TRUTH)
    assert _same(pipe.recognize(images, recognition_kwargs=_kwargs(kind)), _expected(kind, pages))
    assert _same(pipe.recognize_with_scores(images, recognition_kwargs=_kwargs(kind)), _expected(kind, pages, with_scores=True))
    if kind is None:
        assert _same(pipe.recognize_characters(images), _expected(None, pages, with_characters=True))
        assert _same(pipe.recognize_characters(images, peak_threshold=0.5), _expected(None, pages, with_characters=True))


REFUSALS = {
    "evaluate": "evaluate scores one text per word: {key} in recognition_kwargs makes every text a list of alternatives",
    "recognize_lines": "recognize_lines joins one text per word: {key} in recognition_kwargs makes every text a list of alternatives",
    "recognize_characters": "recognize_characters pairs one text per word with its characters: {key} in recognition_kwargs makes "
                            "every text a list of alternatives",
}


@pytest.mark.parametrize("method", sorted(REFUSALS))
@pytest.mark.parametrize("key", ["beam_width", "lexicon_top"])
def test_methods_that_need_one_text_per_word_refuse_alternatives(method, key):
    pipe = _fused()
    args = (_pages(), [[]] * len(SHAPES)) if method == "evaluate" else (_pages(),)
    with pytest.raises(ValueError) as err:
        getattr(pipe, method)(*args, recognition_kwargs={key: 2})
    assert str(err.value) == REFUSALS[method].format(key=key)
    assert pipe.detector._ctx.seen == []  # pylint: disable=protected-access


def test_a_detector_without_char_boxes_is_refused(monkeypatch):
    pipe = _stagewise(monkeypatch)
    pipe.detector = _DetectorWithoutCharacters()
    message = ("char_boxes: the detector (_DetectorWithoutCharacters.detect) cannot give character boxes "
               "(it takes no char_boxes argument)")
    with pytest.raises(TypeError, match=re.escape(message)):
        pipe.recognize_raw(_pages(), char_boxes=True)
    with pytest.raises(TypeError, match=re.escape(message)):
        pipe.recognize_characters(_pages())


@pytest.mark.parametrize("route", ["fused", "stagewise"])
def test_lexicon_top_refusals(monkeypatch, route):
    pipe = _stagewise(monkeypatch) if route == "stagewise" else _fused()
    both = {"lexicon_top": 2, "beam_width": 4}
    for call in (pipe.recognize, pipe.recognize_with_scores, pipe.recognize_raw):
        with pytest.raises(ValueError) as err:
            call(_pages(), recognition_kwargs=both)
        assert str(err.value) == "lexicon_top and beam_width cannot be combined: ask for one of the two"
    pipe.recognizer.lexicon = None
    for call in (pipe.recognize, pipe.recognize_with_scores, pipe.recognize_raw):
        with pytest.raises(ValueError) as err:
            call(_pages(), recognition_kwargs={"lexicon_top": 2})
        assert str(err.value) == "lexicon_top needs a loaded lexicon: call recognizer.set_lexicon(words) first"
        with pytest.raises(ValueError):
            call([], recognition_kwargs={"lexicon_top": 2})


# ---- one label width on every route ------------------------------------------------------------------------------------------
# The label rows -- and the character-score, beam and pattern rows beside them -- have ONE width on every route of
# ``Pipeline._recognize``: the recogniser's (50 - rnn_steps_to_discard; 48 for the default build).  It is read with
# ``pipeline.label_width_of``: the recogniser's ``_ctx.crnn_label_width()`` where its context has one, else its ``label_width``
# attribute.  A duck-typed recogniser that reports NEITHER (``_Recognizer`` above) keeps the stage-wise route's
# ``max(48, longest text)`` columns, and (0, 48) for no images: nothing else is known about it.
WIDTHS = (1, 45, 48, 50)
LW_PAGES = [np.zeros((10, 12, 3), np.uint8), np.zeros((8, 12, 3), np.uint8)]
LW_BOXES = [np.arange(16, dtype=np.float32).reshape(2, 4, 2), np.arange(8, dtype=np.float32).reshape(1, 4, 2)]


class _Ctx:
    """What ``label_width_of`` asks of a libkocr context"""

    def __init__(self, width):
        self.width = width

    def crnn_label_width(self):
        return self.width


class _Det:
    def detect(self, images, return_scores=False, **kw):
        boxes = [b.copy() for b in LW_BOXES[:len(images)]]
        return (boxes, [np.full(len(b), 0.9, np.float32) for b in boxes]) if return_scores else boxes


class _Rec:
    """A duck-typed recogniser: every word reads ``text``; alternatives, pattern readings and scores as the public
    ``Recognizer.recognize_from_boxes`` returns them.  ``how``: "ctx" (the width from ``_ctx.crnn_label_width()``), "attribute"
    (``label_width``) or None (it reports none)."""
    alphabet = ALPHABET

    def __init__(self, width, how, text):
        self.text = text
        self._ctx = _Ctx(width) if how == "ctx" else object()  # patterns need some context; this one reports no width
        if how == "attribute":
            self.label_width = width

    def _pattern_names(self, _name):
        return ["serial"]

    def recognize_from_boxes(self, images, box_groups, return_scores=False, beam_width=None, top_paths=1, pattern=None, **kw):
        t = self.text
        if beam_width is not None:
            word = [(t, -0.5)] + [(t[:-1], -1.5)] * (top_paths - 1)
        elif pattern is not None:
            word = (t, -0.25)
        elif return_scores:
            word = (t, Score(None, 0.5, np.log(0.5), np.full(len(t), 0.75, np.float32)))
        else:
            word = t
        return [[word] * len(boxes) for boxes in box_groups]


@pytest.fixture
def no_gpu_resize(monkeypatch):
    monkeypatch.setattr(k.tools, "resize_image", lambda image, max_scale, max_size, **kw: (
        np.zeros((image.shape[0] * max_scale, image.shape[1] * max_scale, 3), np.uint8), max_scale))


def _widths(pipe, pages):
    """label, char-score, beam-label and pattern-label widths (and the row count) over three calls of ``pipe._recognize``"""
    plain = pipe._recognize(pages, None, None, None, None, return_scores=True)  # pylint: disable=protected-access
    beam = pipe._recognize(pages, None, None, None, {"beam_width": 4, "top_paths": 2})  # pylint: disable=protected-access
    pattern = pipe._recognize(pages, None, None, None, {"pattern": "serial"})  # pylint: disable=protected-access
    m = len(plain.labels)
    assert plain.labels.dtype == np.int32 and plain.labels.ndim == 2
    assert plain.scores[2].shape[0] == m == len(plain.scores[1])
    assert beam.beam[0].shape[:2] == (m, 2) == beam.beam[1].shape and beam.labels.shape == plain.labels.shape
    assert pattern.pattern[0].shape[0] == m == len(pattern.pattern[1]) == len(pattern.pattern[2])
    assert pattern.labels.shape == plain.labels.shape
    return m, (plain.labels.shape[1], plain.scores[2].shape[1], beam.beam[0].shape[2], pattern.pattern[0].shape[1])


@pytest.mark.parametrize("width", WIDTHS)
def test_results_empty_has_the_width_it_is_given(width):
    out = Results.empty(scores=True, beam=(4, 2), pattern=True, label_width=width)
    assert out.labels.shape == (0, width) and out.scores[2].shape == (0, width)
    assert out.beam[0].shape == (0, 2, width) and out.pattern[0].shape == (0, width)


@pytest.mark.parametrize("how", ["ctx", "attribute"])
@pytest.mark.parametrize("width", WIDTHS)
def test_no_images_route(width, how):
    pipe = k.pipeline.Pipeline(detector=_Det(), recognizer=_Rec(width, how, "a"))
    assert _widths(pipe, []) == (0, (width,) * 4)


@pytest.mark.parametrize("how", ["ctx", "attribute"])
@pytest.mark.parametrize("width", WIDTHS)
def test_stagewise_route_has_the_width(no_gpu_resize, width, how):
    """Duck-typed stages; the texts are as long as a row of that width can be (and no longer than 3)"""
    text = "abc"[:width]
    pipe = k.pipeline.Pipeline(detector=_Det(), recognizer=_Rec(width, how, text))
    assert _widths(pipe, LW_PAGES) == (3, (width,) * 4)
    raw = pipe.recognize_raw(LW_PAGES)
    assert raw[1].shape == (3, width) and (raw[1][:, :len(text)] == [ALPHABET.index(c) for c in text]).all()
    assert (raw[1][:, len(text):] == -1).all()
    assert [[t for t, _ in page] for page in pipe.recognize(LW_PAGES)] == [[text, text], [text]]


def test_stagewise_route_refuses_a_text_longer_than_the_reported_width(no_gpu_resize):
    pipe = k.pipeline.Pipeline(detector=_Det(), recognizer=_Rec(1, "attribute", "ab"))
    with pytest.raises(ValueError, match="label width of 1"):
        pipe.recognize_raw(LW_PAGES)


@pytest.mark.parametrize("text, want", [("abc", 48), ("a" * 53, 53)])
def test_a_recogniser_that_reports_no_width_keeps_max_48_longest(no_gpu_resize, text, want):
    """A duck-typed recogniser with neither a context that has ``crnn_label_width()`` nor a ``label_width`` attribute keeps
    what the stage-wise route always built: ``max(48, longest text)`` columns, and (0, 48) for no images"""
    pipe = k.pipeline.Pipeline(detector=_Det(), recognizer=_Rec(None, None, text))
    assert k.pipeline.label_width_of(pipe.recognizer) is None
    assert _widths(pipe, LW_PAGES) == (3, (want,) * 4)
    assert _widths(pipe, []) == (0, (48,) * 4)


class _FusedCtx(_Ctx):
    """``Context.pipeline`` at the C-ABI seam: rows of the context's width, the extras that were asked for"""

    def pipeline(self, images, hs, ws, dhs, dws, hmax, wmax, micro_batch=0, return_scores=False, beam=None, lexicon_top=None,
                 pattern=None, **kw):
        boxes = [b.copy() for b in LW_BOXES[:len(images)]]
        m, w = sum(len(b) for b in boxes), self.width
        out = Results(boxes, np.full((m, w), -1, np.int32))
        out.labels[:, 0] = 3
        if return_scores:
            out.scores = ([np.full(len(b), 0.9, np.float32) for b in boxes], np.zeros(m, np.float32), np.zeros((m, w), np.float32))
        if beam is not None:
            out.beam = (np.full((m, beam[1], w), -1, np.int32), np.zeros((m, beam[1]), np.float32))
        if pattern is not None:
            out.pattern = (np.full((m, w), -1, np.int32), np.zeros(m, np.float32), np.zeros(m, np.float32))
        return out.render_context()


@pytest.mark.parametrize("width", WIDTHS)
def test_parsed_context_route(width):
    """The real Pipeline / Detector / Recognizer classes over one mocked context: the fused route hands the context's rows
    on as they are, and the call without images gives zero rows of the same width"""
    ctx = _FusedCtx(width)
    det = object.__new__(k.detection.Detector)
    rec = object.__new__(k.recognition.Recognizer)
    det._ctx = rec._ctx = ctx  # pylint: disable=protected-access
    rec.alphabet = ALPHABET
    rec._pattern_names = lambda _name: ["serial"]  # pylint: disable=protected-access
    pipe = k.pipeline.Pipeline(detector=det, recognizer=rec)
    assert k.pipeline.label_width_of(rec) == width
    assert _widths(pipe, LW_PAGES) == (3, (width,) * 4)
    assert _widths(pipe, []) == (0, (width,) * 4)
    assert [[t for t, _ in page] for page in pipe.recognize(LW_PAGES)] == [["3", "3"], ["3"]]
