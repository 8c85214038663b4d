"""Host-side mirror of ``keras_ocr.recognition.Recognizer`` (reference
``keras_ocr/recognition.py:353-545``).  The Keras models are replaced by libkocr."""
import dataclasses
import string
import typing

import numpy as np

from . import _lib, charsets as _charsets, layout as _layout, lexicon as _lexicon, patterns as _patterns, scores as _scores, tools, weights as _weights
from .extras import Extras, only_uint8
from .results import Results, decode_labels

DEFAULT_BUILD_PARAMS = {  # recognition.py:13-23
    "height": 31,
    "width": 200,
    "color": False,
    "filters": (64, 128, 256, 256, 512, 512, 512),
    "rnn_units": (128, 128),
    "dropout": 0.25,
    "rnn_steps_to_discard": 2,
    "pool_size": 2,
    "stn": True,
}

DEFAULT_ALPHABET = string.digits + string.ascii_lowercase

PRETRAINED_WEIGHTS: typing.Dict[str, typing.Any] = {  # recognition.py:27-44
    "kurapan": {
        "alphabet": DEFAULT_ALPHABET,
        "build_params": DEFAULT_BUILD_PARAMS,
        "weights": {
            "notop": {
                "url": "https://github.com/faustomorales/keras-ocr/releases/download/v0.8.4/crnn_kurapan_notop.h5",
                "filename": "crnn_kurapan_notop.h5",
                "sha256": "027fd2cced3cbea0c4f5894bb8e9e85bac04f11daf96b8fdcf1e4ee95dcf51b9",
            },
            "top": {
                "url": "https://github.com/faustomorales/keras-ocr/releases/download/v0.8.4/crnn_kurapan.h5",
                "filename": "crnn_kurapan.h5",
                "sha256": "a7d8086ac8f5c3d6a0a828f7d6fbabcaf815415dd125c32533013f85603be46d",
            },
        },
    }
}


# build parameters this implementation can vary (recognition.py:187-198): the transformer on / off and the number of leading
# RNN steps dropped; everything else is the geometry the kernels are written for
_VARIABLE_BUILD_PARAMS = ("stn", "rnn_steps_to_discard")


def _check_build_params(build_params):
    """DEFAULT_BUILD_PARAMS, `stn=False` and any `rnn_steps_to_discard` in [0, 50) are implemented; a different value of any
    other parameter raises NotImplementedError naming it (recognition.py:187-198 takes them all)."""
    unknown = sorted(set(build_params) - set(DEFAULT_BUILD_PARAMS))
    if unknown:
        raise TypeError(f"build_model() got unexpected build parameter(s) {unknown}")
    merged = dict(DEFAULT_BUILD_PARAMS, **build_params)
    for key, default in DEFAULT_BUILD_PARAMS.items():
        value = merged[key]
        if key in _VARIABLE_BUILD_PARAMS:
            continue
        if (tuple(value) if isinstance(value, (list, tuple)) else value) != default and key != "dropout":  # dropout: inference no-op
            raise NotImplementedError(
                f"keras-ocr_amd: build parameter {key}={value!r} is not implemented (only {key}={default!r}); "
                f"the parameters that may differ from DEFAULT_BUILD_PARAMS are {_VARIABLE_BUILD_PARAMS} and dropout")
    steps = int(merged["rnn_steps_to_discard"])
    if not 0 <= steps < 50:
        raise ValueError("rnn_steps_to_discard must lie in [0, 50): the model has 200 // 4 = 50 RNN steps")
    return bool(merged["stn"]), steps


class _Model:
    def __init__(self, ctx, probs):
        self._ctx = ctx
        self._probs = probs
        self.input_shape = (None, 31, 200, 1)

    def predict(self, X, **kwargs):  # pylint: disable=invalid-name,unused-argument
        if self._probs:
            return self._ctx.crnn_forward(X, return_probs=True)[1]
        return self._ctx.crnn_forward(X)


def _integral(a, what):
    """float / int array -> int64, ValueError unless every value is an integer (Keras feeds lengths and labels as float)."""
    a = np.asarray(a)
    if a.dtype.kind in "iub":
        return a.astype(np.int64)
    f = a.astype(np.float64)
    if not np.all(np.isfinite(f)) or np.any(f != np.round(f)) or np.any(np.abs(f) > 2 ** 31 - 1):
        raise ValueError(f"{what} must hold integers")
    return f.astype(np.int64)


def _ctc_host_inputs(y_true, input_length, label_length, m):
    """Keras's (M, Lmax) labels and (M, 1) lengths -> int32 labels (entries from label_length on replaced by -1: they are
    ignored, so they need not be integers) and int32 lengths; ValueError on anything that is not an integer."""
    ll = np.reshape(_integral(label_length, "label_length"), -1)
    il = np.reshape(_integral(input_length, "input_length"), -1)
    if ll.shape != (m,) or il.shape != (m,):
        raise ValueError(f"input_length and label_length must have shape (M, 1) with M = {m}")
    y = np.asarray(y_true)
    if y.ndim != 2 or y.shape[0] != m:
        raise ValueError(f"y_true must have shape (M, max_string_length) with M = {m}, got {y.shape}")
    keep = np.arange(y.shape[1])[np.newaxis, :] < np.clip(ll, 0, None)[:, np.newaxis]
    labels = np.full(y.shape, -1, np.int64)
    for i in range(m):
        if keep[i].any():
            row = _integral(y[i][keep[i]], f"y_true (sample {i})")
            if np.any(np.abs(row) > 2 ** 31 - 1):
                raise ValueError(f"y_true (sample {i}) holds a label outside int32")
            labels[i][keep[i]] = row
    for what, a in (("label_length", ll), ("input_length", il)):
        if np.any(np.abs(a) > 2 ** 31 - 1):
            raise ValueError(f"{what} outside int32")
    return labels.astype(np.int32), il.astype(np.int32), ll.astype(np.int32)


def ctc_batch_cost(y_true, y_pred, input_length, label_length, ctx=None):
    """keras.backend.ctc_batch_cost (the loss of recognition.py:340-347) on the GPU.

    y_true (M, max_string_length) labels, float or int, padded after label_length (the reference pads with -1); y_pred
    (M, T, C) probabilities (blank = C - 1); input_length, label_length (M, 1).  Returns the loss (M, 1) float32: the
    negative log of the summed probability of every alignment, with Keras's log(y_pred + 1e-7).
    A length outside its range or a label outside [0, C - 2] raises ValueError naming the sample; a label that does not
    fit with a blank between its repeats gives +inf."""
    ctx = ctx or _lib.default_context()
    y = np.asarray(y_pred, dtype=np.float32)
    if y.ndim != 3:
        raise ValueError(f"y_pred must have shape (M, T, C), got {y.shape}")
    labels, il, ll = _ctc_host_inputs(y_true, input_length, label_length, y.shape[0])
    return ctx.ctc_batch_cost(y, labels, ll, il)[:, np.newaxis]


def rgb2gray_u8(image):
    """cv2.cvtColor(image, cv2.COLOR_RGB2GRAY) of a uint8 image: OpenCV's 15-bit fixed-point coefficients, rounded."""
    im = np.asarray(image)
    if im.ndim != 3 or im.shape[-1] not in (3, 4):
        raise ValueError(f"an RGB image of shape (H, W, 3) is required, got {im.shape}")
    im = im[..., :3].astype(np.int64)
    return ((im[..., 0] * 9798 + im[..., 1] * 19235 + im[..., 2] * 3735 + (1 << 14)) >> 15).astype(np.uint8)


def _to_gray(image):
    im = np.asarray(image)
    if im.dtype == np.uint8:
        return rgb2gray_u8(im)
    if im.ndim != 3 or im.shape[-1] not in (3, 4):
        raise ValueError(f"an RGB image of shape (H, W, 3) is required, got {im.shape}")
    f = im[..., :3].astype(np.float32)  # cv2.cvtColor of a float image: the float coefficients
    return f[..., 0] * np.float32(0.299) + f[..., 1] * np.float32(0.587) + f[..., 2] * np.float32(0.114)


def batch_generator(image_generator, alphabet, max_string_length, batch_size=8, lowercase=False):
    """Recognizer.get_batch_generator (recognition.py:406-465) for a gray model: yields
    ((images (B,H,W,1) float32 /255, labels (B, max_string_length) -1 padded, input_length (B,1), label_length (B,1)), y)
    and, when the samples are (image, sentence, weight) tuples, the weights as a third element.  Batches are taken with the
    reference's zip(image_generator, range(batch_size)), so one sample is drawn and dropped between batches as there.  The
    reference's four assertions hold.  Unlike the reference, an exhausted generator ends the iteration, and a last batch
    shorter than batch_size gets input_length and y of its own length."""
    while True:
        batch = [sample for sample, _ in zip(image_generator, range(batch_size))]
        if not batch:
            return
        images = np.array([_to_gray(sample[0])[..., np.newaxis].astype("float32") / 255 for sample in batch])
        sentences = [sample[1].strip() for sample in batch]
        if lowercase:
            sentences = [sentence.lower() for sentence in sentences]
        for c in "".join(sentences):
            assert c in alphabet, f"Found illegal character: {c}"
        assert all(sentences), "Found a zero length sentence."
        assert all(len(sentence) <= max_string_length for sentence in sentences), \
            "A sentence is longer than this model can predict."
        assert all("  " not in sentence for sentence in sentences), (
            "Strings with multiple sequential spaces are not permitted. "
            "See https://github.com/faustomorales/keras-ocr/issues/54")
        label_length = np.array([len(sentence) for sentence in sentences])[:, np.newaxis]
        labels = np.array([[alphabet.index(c) for c in sentence] + [-1] * (max_string_length - len(sentence))
                           for sentence in sentences])
        input_length = np.ones((len(batch), 1)) * max_string_length
        y = np.zeros((len(batch), 1))
        if len(batch[0]) == 3:
            sample_weights = np.array([sample[2] for sample in batch])
            yield (images, labels, input_length, label_length), y, sample_weights
        else:
            yield (images, labels, input_length, label_length), y


_INFERENCE_ONLY = "keras-ocr_amd is inference-only: training (fit / compile) is not implemented"


class _TrainingModel:
    """recognizer.training_model (recognition.py:334-349): [crops, labels, input_length, label_length] -> CTC loss (M, 1)."""

    output_shape = (None, 1)

    def __init__(self, ctx):
        self._ctx = ctx

    @property
    def input_shape(self):
        return [(None, 31, 200, 1), (None, self._ctx.crnn_label_width()), (None, 1), (None, 1)]

    def predict(self, x, batch_size=None, **kwargs):  # pylint: disable=unused-argument
        """x = [X (M,31,200,1), labels (M, label width), input_length (M,1), label_length (M,1)]; batch_size and the other
        Keras predict arguments do not change the result."""
        X, y_true, input_length, label_length = x  # pylint: disable=invalid-name
        labels, il, ll = _ctc_host_inputs(y_true, input_length, label_length, np.shape(X)[0])
        return self._ctx.crnn_ctc_loss(X, labels, ll, il)[:, np.newaxis]

    def fit(self, *args, **kwargs):
        raise NotImplementedError(_INFERENCE_ONLY)

    def compile(self, *args, **kwargs):
        raise NotImplementedError(_INFERENCE_ONLY)


class _Backbone:
    """recognizer.backbone (recognition.py:319-320): crops -> the BiLSTM features (M, 50, 256)."""

    input_shape = (None, 31, 200, 1)
    output_shape = (None, 50, 256)

    def __init__(self, ctx):
        self._ctx = ctx

    def predict(self, X, **kwargs):  # pylint: disable=invalid-name,unused-argument
        return self._ctx.crnn_features(X)


class Recognizer:
    """A text recogniser using the CRNN architecture (recognition.py:353-404).

    Args:
        alphabet: the alphabet the model recognises.
        weights: ``"kurapan"`` (pretrained file from the keras-ocr cache directory), ``None``
            (random initialisation: seeded synthetic weights) or a ``dict`` of Keras-named arrays.
        build_params: ``DEFAULT_BUILD_PARAMS``, optionally with ``stn=False`` (no spatial transformer, recognition.py:243)
            and / or another ``rnn_steps_to_discard`` (recognition.py:328); a different ``color`` / size / filter set raises
            ``NotImplementedError`` naming the parameter.
    """

    def __init__(self, alphabet=None, weights="kurapan", build_params=None, ctx=None):
        assert alphabet or weights, "At least one of alphabet or weights must be provided."
        if weights is not None and not isinstance(weights, dict):
            build_params = build_params or PRETRAINED_WEIGHTS[weights]["build_params"]
            alphabet = alphabet or PRETRAINED_WEIGHTS[weights]["alphabet"]
        build_params = build_params or DEFAULT_BUILD_PARAMS
        stn, discard = _check_build_params(dict(build_params))
        if alphabet is None:
            alphabet = DEFAULT_ALPHABET
        self.alphabet = alphabet
        self.blank_label_idx = len(alphabet)
        self._ctx = ctx or _lib.default_context()
        if isinstance(weights, dict):
            state = weights
        elif weights is not None:
            weights_dict = PRETRAINED_WEIGHTS[weights]
            if alphabet == weights_dict["alphabet"]:
                cfg = weights_dict["weights"]["top"]
                state = _weights.read_keras_h5(
                    tools.download_and_verify(url=cfg["url"], filename=cfg["filename"], sha256=cfg["sha256"]), kind="crnn")
            else:
                print("Provided alphabet does not match pretrained alphabet. Using backbone weights only.")
                cfg = weights_dict["weights"]["notop"]
                state = _weights.read_keras_h5(
                    tools.download_and_verify(url=cfg["url"], filename=cfg["filename"], sha256=cfg["sha256"]), kind="crnn")
                state.update(_weights.synthetic_fc12(len(alphabet) + 1))
        else:
            state = _weights.synthetic_crnn_weights(n_classes=len(alphabet) + 1)
        if state["fc_12/bias"].shape[0] != len(alphabet) + 1:
            raise ValueError("fc_12 does not match the alphabet length")
        if not stn:  # recognition.py:243: the model is built without the localisation network; its tensors are not loaded
            state = {k: v for k, v in state.items() if not k.startswith("stn_")}
        elif "stn_conv_1/kernel" not in state:
            raise ValueError("build_params['stn'] is True but the weights carry no stn_* tensors")
        # the load first: a refused weight set must leave a shared context's label width as the recogniser serving there set it
        self._ctx.load_crnn(state)
        self._ctx.crnn_set_rnn_steps_to_discard(discard)
        self.build_params = dict(DEFAULT_BUILD_PARAMS, **dict(build_params))
        self.model = _Model(self._ctx, probs=True)
        self.prediction_model = _Model(self._ctx, probs=False)
        self.backbone = _Backbone(self._ctx)
        self.training_model = _TrainingModel(self._ctx)
        self.lexicon = None
        self.charsets = None
        self.patterns = None

    def set_patterns(self, patterns, lowercase=False):
        """The patterns for ``pattern=`` ("Patterns"): a mapping name -> regular expression, e.g.
        ``{"date": r"\\d{2}/\\d{2}/\\d{4}"}``, or a ``patterns.Patterns`` built with this recogniser's alphabet; compiled on
        the host (``patterns.py`` lists the syntax), loaded into the context once, resident like a lexicon;
        ``Recognizer.patterns`` holds them.  ``None`` unloads.  ``lowercase``: lower-case the literal characters first.
        ValueError naming the pattern and the position for unsupported syntax, naming the character for a literal the alphabet
        cannot spell, naming the count for more than 64 patterns, 256 states or 4096 label nodes, and for an empty language."""
        if patterns is None:
            self._ctx.set_patterns(None)
            self.patterns = None
            return
        pats = patterns if isinstance(patterns, _patterns.Patterns) else _patterns.Patterns(self.alphabet, patterns, lowercase=lowercase)
        if pats.classes != len(self.alphabet) + 1 or pats.alphabet != self.alphabet:
            raise ValueError(f"the patterns were built for an alphabet of {pats.classes} classes (blank included), the recogniser "
                             f"has {len(self.alphabet) + 1}: class count / alphabet mismatch")
        self._ctx.set_patterns(*pats.tables())
        self.patterns = pats

    def _pattern_names(self, pattern):
        """The loaded names for a ``pattern=`` argument (None when none is asked for); ValueError without loaded patterns"""
        if pattern is None:
            return None
        if self.patterns is None or self._ctx.pattern_count() != len(self.patterns):
            raise ValueError("pattern needs loaded patterns: call Recognizer.set_patterns({name: regex}) first (the patterns are "
                             "unloaded when a recogniser of another class count is loaded on their context)")
        return self.patterns.names

    def set_charsets(self, charsets, lowercase=False):
        """The character sets for ``charset=`` ("Character sets"): a mapping name -> characters, e.g.
        ``{"digits": "0123456789"}``; the table is loaded into the context once and stays there like a lexicon, and
        ``Recognizer.charsets`` holds the names.  ``None`` unloads.  ``lowercase``: lower-case the characters first.
        ValueError naming the set and the character for one outside the alphabet, for an empty set and for more than 256."""
        if charsets is None:
            self._ctx.set_charsets(None)
            self.charsets = None
            return
        names, allowed = _charsets.table(charsets, self.alphabet, lowercase=lowercase)
        self._ctx.set_charsets(allowed)
        self.charsets = names

    def _charset_names(self, charset):
        """The loaded names for a ``charset=`` argument (None when none is asked for); ValueError without a loaded table"""
        if charset is None:
            return None
        if self.charsets is None or self._ctx.charset_count() != len(self.charsets):
            raise ValueError("charset needs loaded character sets: call Recognizer.set_charsets({name: characters}) first (the "
                             "sets are unloaded when a recogniser of another class count is loaded on their context)")
        return self.charsets

    def set_lexicon(self, words, lowercase=False):
        """The word list for ``lexicon_top=`` ("Lexicon"): an iterable of strings or a
        ``lexicon.Lexicon`` built with this recogniser's alphabet; it is loaded into the context once and stays there like
        weights.  ``None`` unloads.  ValueError naming the word for one the alphabet cannot spell, an empty or an over-long
        one; naming the class counts for a Lexicon of another alphabet."""
        if words is None:
            self._ctx.set_lexicon(None)
            self.lexicon = None
            return
        lex = words if isinstance(words, _lexicon.Lexicon) else _lexicon.Lexicon(words, self.alphabet, lowercase=lowercase)
        if lex.classes != len(self.alphabet) + 1 or lex.alphabet != self.alphabet:
            raise ValueError(f"the lexicon was built for an alphabet of {lex.classes} classes (blank included), the recogniser "
                             f"has {len(self.alphabet) + 1}: class count / alphabet mismatch")
        if not len(lex):
            raise ValueError("the lexicon has no words")
        self._ctx.set_lexicon(lex.labels, lex.lengths)
        self.lexicon = lex

    def get_batch_generator(self, image_generator, batch_size=8, lowercase=False):
        """Recognizer.get_batch_generator (recognition.py:406-465): batches for training_model.predict; see
        batch_generator."""
        return batch_generator(image_generator, self.alphabet, self.training_model.input_shape[1][1], batch_size=batch_size,
                               lowercase=lowercase)

    def compile(self, *args, **kwargs):
        """Recognizer.compile (recognition.py:539-545): training is not implemented."""
        raise NotImplementedError(_INFERENCE_ONLY)

    def _decode(self, rows):
        return decode_labels(self.alphabet, rows)

    def recognize(self, image, return_scores=False, beam_width=None, top_paths=1, lexicon_top=None, charset=None, pattern=None):
        """Recognizer.recognize (recognition.py:467-489): one pre-cropped RGB image -> string; ``return_scores=True``:
        ``(text, score)``, a ``scores.Score`` whose ``detection`` is None.

        ``beam_width=B`` (1..64; default None: the greedy decode above, untouched): instead of the string, a list of up to
        ``top_paths`` alternatives ``(text, log_prob)``, best first, from a CTC prefix beam search (DESIGN.md section 4,
        "Beam search"); ``log_prob`` is the exact log-probability of the text, ``-ctc loss``.  With ``return_scores`` the
        result is ``(alternatives, score)``, the score still that of the greedy decode.

        ``lexicon_top=K`` (1..64, after ``set_lexicon``): instead of the string, a list of up to K ``(word, log_prob)``, the
        lexicon's words of the highest exact CTC log-probability given the crop, best first (DESIGN.md section 4,
        "Lexicon").  Not together with ``beam_width`` (ValueError).

        ``charset=name`` (after ``set_charsets``; default None: unconstrained): the crop is decoded as if the recogniser could
        only answer the characters of that set -- the text, its scores, the beam alternatives and the lexicon values all
        follow ("Character sets").  ValueError listing the loaded names for an unknown one.

        ``pattern=name`` (after ``set_patterns``; default None): instead of the string, ``(text, log_prob)`` -- the best
        reading of the crop that the regular expression accepts and its exact CTC log-probability (DESIGN.md section 4,
        "Patterns"); ``(None, -inf)`` when no accepted text fits the crop's frames.  Not together with ``beam_width``,
        ``lexicon_top`` or ``charset`` (ValueError)."""
        extras = Extras.from_arguments(self, return_scores, beam_width, top_paths, lexicon_top, charset=charset, pattern=pattern)
        image = tools.read_and_fit(filepath_or_array=image, width=200, height=31, cval=0)
        if image.shape[-1] == 3:
            # gray conversion on the GPU: warp the full 31x200 rectangle onto itself (identity map)
            box = np.array([[0, 0], [200, 0], [200, 31], [0, 31]], np.float32)
            crops = self._ctx.warp_crops(image[np.newaxis], [box[np.newaxis]], 31, 200)
        else:
            crops = image[np.newaxis, ..., 0].astype("float32") / 255
        with extras.charset_scope(self._ctx):
            return self._words(self._recognize_crops(crops, extras))[0]

    def _recognize_crops(self, crops, extras):
        """The ``Results`` of crops on the host: the decode [with its scores], and the alternatives or matches asked for;
        ``extras.pattern``: the index every crop is decoded under"""
        out = Results(None, None)
        if extras.pattern is not None:
            out.pattern = self._ctx.crnn_pattern(crops, np.full(len(crops), extras.pattern, np.int32))
            out.labels = out.pattern[0]
        if extras.scores:
            out.labels, *scores = self._ctx.crnn_forward_scores(crops)
            out.scores = (None, *scores)
        if extras.beam is not None:
            out.beam = self._ctx.crnn_beam(crops, *extras.beam)
        elif extras.lexicon_top is not None:
            out.lexicon = self._ctx.crnn_lexicon(crops, extras.lexicon_top)
        elif not extras.scores and extras.pattern is None:
            out.labels = self._ctx.crnn_forward(crops)
        return out

    def recognize_from_boxes(self, images, box_groups, return_scores=False, beam_width=None, top_paths=1, lexicon_top=None,
                             orientation=None, tall_ratio=1.5, return_orientation=False, charset=None, pattern=None,
                             **kwargs) -> typing.List[typing.List[str]]:
        """Recognizer.recognize_from_boxes (recognition.py:491-537); ``return_scores=True``: per image a list of
        ``(text, score)``, ``score`` a ``scores.Score`` whose ``detection`` is None.  ``beam_width`` / ``top_paths``: as
        ``recognize`` -- every text becomes its list of ``(text, log_prob)`` alternatives; ``lexicon_top``: as ``recognize`` --
        every text becomes its list of ``(word, log_prob)`` lexicon matches.

        ``orientation="flip"`` / ``"any"`` ("Orientation"; default None: off): every box is read in two
        orientations on the GPU -- as detected and upside down, or, with ``"any"``, down and up the page for a box whose
        height is at least ``tall_ratio`` times its width -- and each text (and score) is that of the reading with the larger
        exact CTC log-probability, an empty reading losing to a non-empty one.  ``return_orientation=True`` (needs
        ``orientation``): every word becomes ``(text[, score], layout.Orientation(turns, box, log_words))``.  Not together
        with ``beam_width`` or ``lexicon_top`` (ValueError naming both); uint8 images only (NotImplementedError).

        ``charset`` (after ``set_charsets``; DESIGN.md section 4, "Character sets"): a name -- every box is decoded under
        that set -- or per image a list with one name or None (unconstrained) per box: an amount and a name on one page.
        It combines with every other argument; with ``orientation`` both readings of a box use its set.  Per-box lists
        need uint8 images (NotImplementedError).

        ``pattern`` (after ``set_patterns``; DESIGN.md section 4, "Patterns"): a name -- every box is decoded under that
        regular expression -- or per image a list with one name or None per box: a date and an amount on one page.  Every
        text becomes ``(text, log_prob)``, the best accepted reading and its exact CTC log-probability, ``(None, -inf)``
        where nothing fits or the box has no pattern.  Not together with ``beam_width``, ``lexicon_top``, ``charset`` or
        ``orientation`` (ValueError); uint8 images only (NotImplementedError)."""
        del kwargs  # Keras predict kwargs (batch_size, verbose, ...) have no effect on results
        extras = Extras.from_arguments(self, return_scores, beam_width, top_paths, lexicon_top, orientation, tall_ratio, return_orientation,
                                       charset, pattern, box_groups)
        with extras.charset_scope(self._ctx):
            return self._recognize_from_boxes(images, box_groups, dataclasses.replace(extras, charset=None))

    def _recognize_from_boxes(self, images, box_groups, extras):
        """recognize_from_boxes under the context's character-set switch"""
        assert len(box_groups) == len(images), "You must provide the same number of box groups as images."
        images = [tools.read(image) for image in images]
        if extras.orientation is not None:
            only_uint8(images, "orientation")
        if not sum(len(b) for b in box_groups):
            asked = extras.scores or extras.beam or extras.lexicon_top or extras.return_orientation or extras.patterned
            return [[] for _ in images] if asked else [[]] * len(images)
        start_end: typing.List[typing.Tuple[int, int]] = []
        for boxes in box_groups:
            start = 0 if not start_end else start_end[-1][1]
            start_end.append((start, start + len(boxes)))
        images = [np.asarray(image) for image in images]
        if extras.set_of is not None:
            only_uint8(images, "charset")
        if extras.patterned:
            only_uint8(images, "pattern")
        if any(im.dtype != np.uint8 for im in images):
            # float images (recognition.py:507-526 works in the image's own type): gray conversion and the crop warp in
            # float ON THE GPU (kocr_warp_crops_f32, round 5), the division by 255 of :524, the recogniser
            crops = []
            for image, boxes in zip(images, box_groups):
                if len(boxes):
                    im = np.asarray(image, np.float32)
                    crops.append(self._ctx.warp_crops_f32((im if im.ndim == 3 else im[..., np.newaxis])[np.newaxis], [boxes], 31, 200))
            out = self._recognize_crops(np.concatenate(crops) / np.float32(255), extras)
        elif len({im.shape for im in images}) == 1:
            # one size (what Pipeline / Detector hand over): crops never leave HBM
            out = self._ctx._recognize_boxes(np.stack(images), box_groups, extras)  # pylint: disable=protected-access
        else:
            # the reference loops per image, so sizes may differ: one call per image
            out = Results.concatenate([self._ctx._recognize_boxes(image[np.newaxis], [boxes], dataclasses.replace(  # pylint: disable=protected-access
                extras, set_of=None if extras.set_of is None else extras.set_of[start:end],
                pattern_of=None if extras.pattern_of is None else extras.pattern_of[start:end]))
                for image, boxes, (start, end) in zip(images, box_groups, start_end) if len(boxes)])
        words = self._words(out)
        if extras.return_orientation:
            how = _layout.orientations_of(*out.orientation)
            words = [(*word, o) if extras.scores else (word, o) for word, o in zip(words, how)]
        return [words[start:end] for start, end in start_end]

    def recognize_from_boxes_windowed(self, images, box_groups, aspect=10.0, overlap=40, return_scores=False, return_windows=False):
        """``recognize_from_boxes`` with long words read in overlapping windows ("Long words";
        include/kocr_windows.h): a box whose width exceeds ``aspect`` times its height is cut along its long side into 31 x 200
        windows that overlap by ``overlap`` crop pixels, the windows' frames are stitched into one sequence on the GPU and
        that sequence is decoded; every other box is read as ever, bit for bit.  Per image a list of texts, or of
        ``(text, score)`` with ``return_scores`` (``score`` a ``scores.Score`` whose ``detection`` is None, ``log_word`` the exact
        CTC log-probability over the whole sequence); ``return_windows=True`` appends every word's window count.  ValueError
        for ``aspect`` < 200 / 31, an ``overlap`` that is no multiple of 8 in [16, 96], a box of more than 2048 frames, or a
        switch of the context that cannot be combined with it; uint8 images only (NotImplementedError)."""
        assert len(box_groups) == len(images), "You must provide the same number of box groups as images."
        tools.window_args(aspect, overlap, 50 - self._ctx.crnn_label_width())
        images = [np.asarray(tools.read(image)) for image in images]
        only_uint8(images, "windowed")
        runs = []  # one call for images of one size, else one per image (as recognize_from_boxes)
        if len({im.shape for im in images}) == 1:
            runs.append(self._ctx.recognize_boxes_windowed(np.stack(images), box_groups, aspect, overlap))
        else:
            runs.extend(self._ctx.recognize_boxes_windowed(im[np.newaxis], [boxes], aspect, overlap) for im, boxes in zip(images, box_groups))
        words = []
        for labels, log_word, chars, _, windows in runs:
            texts = self._decode(labels) if len(labels) else []
            row = list(zip(texts, _scores.assemble(labels, log_word, chars))) if return_scores else texts
            if return_windows:
                row = [(*w, int(k)) if return_scores else (w, int(k)) for w, k in zip(row, windows)]
            words.extend(row)
        out, start = [], 0
        for boxes in box_groups:
            out.append(words[start:start + len(boxes)])
            start += len(boxes)
        return out

    def _words(self, out):
        """A ``Results``' crops as what recognize_from_boxes returns for each: the text, or its alternatives (``beam``), or
        its matches (``lexicon``) [paired with the ``Score`` of the greedy decode]"""
        words, scores = out.words(self.alphabet, self.lexicon)
        return words if scores is None else list(zip(words, scores))
