"""The one record that carries what detection and recognition produce, the optional results included, between the C calls
and the public return values; it owns the legacy tuple layouts of those return values and the empty value of every extra."""
import dataclasses
import typing

import numpy as np

from . import scores as _scores


def empty_scores(label_width=48, detection=None):
    return detection, np.zeros(0, np.float32), np.zeros((0, label_width), np.float32)


def empty_beam(top_paths, label_width=48):
    return np.zeros((0, top_paths, label_width), np.int32), np.zeros((0, top_paths), np.float32)


def empty_lexicon(top_words):
    return np.zeros((0, top_words), np.int32), np.zeros((0, top_words), np.float32)


def empty_pattern(label_width=48):
    return np.zeros((0, label_width), np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32)


def empty_orientation():
    return np.zeros(0, np.int32), np.zeros((0, 4, 2), np.float32), np.zeros((0, 2), np.float32)


def decode_labels(alphabet, labels):
    """Label rows -> strings, skipping the blank (= len(alphabet)) and the -1 padding (recognition.py:527-534).

    One table lookup and one UTF-32 decode for the whole batch: iterating 600 x 48 numpy scalars costs 4 ms
    per call, during which the GPU sits idle."""
    labels = np.asarray(labels)
    if labels.size == 0:
        return [""] * len(labels)
    n = len(alphabet)
    if (labels.ndim != 2 or any(len(c) != 1 or c == "\0" or 0xD800 <= ord(c) <= 0xDFFF for c in alphabet)
            or labels.min() < -1 or labels.max() > n):
        # multi-character entries, lone surrogates (no UTF-32 encoding), a single row, or indices the reference's own
        # expression would wrap / reject: evaluate that expression
        skip = (n, -1)
        rows = labels.tolist() if labels.ndim == 2 else [labels.tolist()] if labels.ndim == 1 else labels.reshape(-1, labels.shape[-1]).tolist()
        return ["".join([alphabet[i] for i in row if i not in skip]) for row in rows]
    table = np.array([ord(c) for c in alphabet] + [0], "<u4")
    text = table[np.where(labels < 0, n, labels)].tobytes().decode("utf-32-le")
    w = labels.shape[1]
    return [text[i * w:(i + 1) * w].replace("\0", "") for i in range(labels.shape[0])]


@dataclasses.dataclass
class Results:
    """What one call produced for N images with n_i boxes each, M = sum n_i crops in image order.  A stage that did not run
    leaves its field (or its part of ``scores``) None; an extra that was not asked for is None.

    boxes: per image an (n_i, 4, 2) float32 array [tl, tr, br, bl] (``np.array([])`` for an image without boxes).
    labels: (M, label width) int32 decoded label rows, -1 padded; the label width is the recogniser's (50 - its
        rnn_steps_to_discard: 48 by default) on every route, the empty one included.
    scores: ``(detection, log_word, char_scores)`` -- per image an (n_i,) float32 array, the maximum of the text map over each
        box's component; (M,) float32, the log-probability of every alignment of the crop's own (greedy) decode; (M, label
        width) float32, per decoded label the peak probability of its run, 0 behind the decode.
    beam: ``(labels (M, K, label width) int32, log_prob (M, K) float32)`` as ``Context.crnn_beam``, best first; rows that do
        not exist are all -1 with -inf.
    lexicon: ``(index (M, K) int32, log_prob (M, K) float32)`` as ``Context.crnn_lexicon``, best first, -1 / -inf where fewer
        words are feasible.
    characters: per image a list of one entry per box, its characters from tl towards tr: a ``(quads (K, 4, 2) float32, scores
        (K,) float32)`` pair below ``Detector`` / ``Pipeline``, a ``layout.Characters`` from there on.
    orientation: ``(turns (M,) int32, quads (M, 4, 2) float32, log_words (M, 2) float32)`` as
        ``Context.recognition_orientation``: with it, labels and the recogniser's scores are those of each word's better
        reading, ``quads[m]`` is [tl, tr, br, bl] of the text as read and ``log_words[m]`` the two candidates' values.  While it
        is None every layout below is what it was; where present it comes last (before ``pattern``).
    pattern: ``(labels (M, label width) int32, log_path (M,) float32, log_prob (M,) float32)`` as ``Context.crnn_pattern``: each
        crop's best reading that its pattern accepts ("Patterns"), -1 / -inf where nothing fits or the crop
        has no pattern.  While it is None every layout below is what it was; where present it comes last of all.

    For zero images (``empty``) or zero crops the extras are zero-row arrays of these shapes and dtypes."""
    boxes: typing.Any
    labels: typing.Any
    scores: typing.Any = None
    beam: typing.Any = None
    lexicon: typing.Any = None
    characters: typing.Any = None
    orientation: typing.Any = None
    pattern: typing.Any = None

    @classmethod
    def empty(cls, scores=False, beam=None, lexicon=None, characters=False, label_width=48, orientation=False, pattern=False):
        """The results of zero images; ``beam`` = (beam_width, top_paths), ``lexicon`` = top_words; ``label_width``: the
        recogniser's (None: it reports none, the default build's 48)"""
        label_width = 48 if label_width is None else int(label_width)
        return cls([], np.zeros((0, label_width), np.int32), empty_scores(label_width, []) if scores else None,
                   empty_beam(beam[1], label_width) if beam else None, empty_lexicon(lexicon) if lexicon else None,
                   [] if characters else None, empty_orientation() if orientation else None,
                   empty_pattern(label_width) if pattern else None)

    def words(self, alphabet, lexicon=None):
        """The crops as the public per-word values, and their ``Score`` column (None without ``scores``): a ``(text,
        log_prob)`` pair for pattern rows, ``(None, -inf)`` where nothing fits; a list of up to K ``(word, log_prob)`` matches
        for lexicon rows, the words looked up in ``lexicon.words``; a list of up to K ``(text, log_prob)`` alternatives for
        beam rows; else the decoded string.  Entries that do not exist (-1, -inf) are dropped."""
        if self.pattern is not None:
            texts = decode_labels(alphabet, self.pattern[0])
            values = [(text, float(v)) if v != -np.inf else (None, -np.inf) for text, v in zip(texts, np.asarray(self.pattern[2]))]
        elif self.lexicon is not None:
            known = lexicon.words
            values = [[(known[i], float(v)) for i, v in zip(row, vals) if i >= 0]
                      for row, vals in zip(np.asarray(self.lexicon[0]).tolist(), np.asarray(self.lexicon[1]))]
        elif self.beam is not None:
            beam_labels, beam_log_prob = np.asarray(self.beam[0]), np.asarray(self.beam[1])
            m, k = beam_log_prob.shape
            texts = decode_labels(alphabet, beam_labels.reshape(m * k, -1)) if m * k else []
            values = [[(texts[i * k + j], float(beam_log_prob[i, j])) for j in range(k) if beam_log_prob[i, j] != -np.inf]
                      for i in range(m)]
        else:
            values = decode_labels(alphabet, self.labels)
        if self.scores is None:
            return values, None
        det, log_word, chars = self.scores
        if det is not None:
            det = np.concatenate([np.asarray(d, np.float32).reshape(-1) for d in det]) if len(det) else np.zeros(0, np.float32)
        return values, _scores.assemble(self.labels, log_word, chars, det)

    def render_context(self):
        """``Context.pipeline``'s layout: ``(boxes, labels[, scores][, beam | lexicon][, characters][, orientation][, pattern])``,
        nothing padded"""
        alternatives = self.beam if self.lexicon is None else self.lexicon
        return tuple([self.boxes, self.labels] +
                     [v for v in (self.scores, alternatives, self.characters, self.orientation, self.pattern) if v is not None])

    @classmethod
    def parse_context(cls, out, scores=False, beam=False, lexicon=False, characters=False, orientation=False, pattern=False):
        """``render_context``'s inverse, given which extras were asked for (with both ``beam`` and ``lexicon``: the lexicon)"""
        wanted = (True, True, scores, beam and not lexicon, lexicon, characters, orientation, pattern)
        if len(out) != sum(map(bool, wanted)):
            raise ValueError(f"{len(out)} results do not fit scores={scores}, beam={beam}, lexicon={lexicon}, characters={characters}"
                             + (f", orientation={orientation}" if orientation else "") + (f", pattern={pattern}" if pattern else ""))
        values = iter(out)
        return cls(*[next(values) if w else None for w in wanted])

    def render_raw(self):
        """``Pipeline.recognize_raw``'s layout: ``(boxes, labels[, scores_or_None[, beam_or_None[, lexicon]]][, characters]
        [, orientation][, pattern])`` -- as short as the extras allow, None in the place of an earlier extra that was not asked for"""
        extras = [self.scores, self.beam, self.lexicon]
        while extras and extras[-1] is None:
            extras.pop()
        return (self.boxes, self.labels, *extras) + (() if self.characters is None else (self.characters,)) + \
            (() if self.orientation is None else (self.orientation,)) + (() if self.pattern is None else (self.pattern,))

    def render_detection(self):
        """``Context.get_boxes`` / ``detect``: the boxes, or ``(boxes[, detection scores][, characters])`` with an extra"""
        if self.scores is None and self.characters is None:
            return self.boxes
        return (self.boxes,) + (() if self.scores is None else (self.scores[0],)) + (() if self.characters is None else (self.characters,))

    def render_recognition(self):
        """``Context.recognize_boxes``: the labels, or ``(labels[, log_word, char_scores][, beam pair][, lexicon pair][, turns,
        quads, log_words][, pattern labels, log_path, log_prob])``, flat"""
        if self.scores is None and self.beam is None and self.lexicon is None and self.orientation is None and self.pattern is None:
            return self.labels
        return (self.labels, *(self.scores or (None,))[1:], *(self.beam or ()), *(self.lexicon or ()), *(self.orientation or ()),
                *(self.pattern or ()))

    @classmethod
    def concatenate(cls, parts):
        """The crops of several ``Context.recognize_boxes`` calls, one behind the other (no boxes: those belong to the caller)"""
        def join(field):
            values = [getattr(part, field) for part in parts]
            return None if values[0] is None else tuple(None if v[0] is None else np.concatenate(v) for v in zip(*values))
        return cls(None, np.concatenate([part.labels for part in parts]), join("scores"), join("beam"), join("lexicon"),
                   orientation=join("orientation"), pattern=join("pattern"))
