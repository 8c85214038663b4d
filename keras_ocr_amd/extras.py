"""What one call asked for beyond boxes and texts, as one record: it owns the refusals of arguments that cannot be combined,
the order in which they are raised, the empty result and the flags of ``Results.parse_context``."""
import contextlib
import dataclasses
import typing

import numpy as np

from . import _lib, charsets as _charsets, lexicon as _lexicon, patterns as _patterns
from .results import Results

# who validates: Pipeline (the names are keys of recognition_kwargs), Recognizer (its arguments), Context (its keywords)
KWARGS, ARGUMENTS, CONTEXT = "kwargs", "arguments", "context"

_UINT8_ONLY = {
    "orientation": "orientation: only uint8 images are read in two orientations (the float crop path has no turned set-up)",
    "pattern": "pattern: patterns need uint8 images (the float crop path decodes plain crops)",
    "charset": "charset: per-box character sets need uint8 images (the float crop path decodes plain crops)",
    "recognize_tiled": "recognize_tiled: only uint8 images are read in tiles (the tile copy moves RGB bytes)",
    "windowed": "windowed reading: only uint8 images are read in windows (the float crop path has no window plan)",
}


def only_uint8(images, feature):
    """NotImplementedError with ``feature``'s own text unless every image is uint8"""
    if any(np.asarray(image).dtype != np.uint8 for image in images):
        raise NotImplementedError(_UINT8_ONLY[feature])


def _pattern_and(name):
    return ValueError(f"pattern and {name} cannot be combined: " + (
        "the pattern states the characters itself" if name in ("charset", "set_of") else "ask for one of the two"))


@dataclasses.dataclass(frozen=True, eq=False)
class Extras:
    """scores: whether they are asked for; beam: ``(beam_width, top_paths)`` or None; lexicon_top: the matches per word, or None.
    char_boxes: None, or the rule of the character boxes: ``_lib.char_rule``'s dict at the Context; above it the caller's own
        value (True or a dict of rule parameters), handed down as it came -- the Context validates it.
    orientation: ``(name, tall_ratio)`` or None (at the Context ``(mode code, tall_ratio)``); return_orientation: whether
        ``recognize_from_boxes`` adds each word's ``layout.Orientation``.
    charset / pattern: the index of the one set / pattern for every box, or None; set_of / pattern_of: the flat per-box
        indices (-1: none), or None.
    min_area_rect: the rule of getBoxes for this call, or None."""
    scores: bool = False
    beam: typing.Any = None
    lexicon_top: typing.Any = None
    char_boxes: typing.Any = None
    orientation: typing.Any = None
    return_orientation: bool = False
    charset: typing.Any = None
    set_of: typing.Any = None
    pattern: typing.Any = None
    pattern_of: typing.Any = None
    min_area_rect: typing.Any = None

    characters = property(lambda self: self.char_boxes is not None)
    patterned = property(lambda self: self.pattern is not None or self.pattern_of is not None)

    @classmethod
    def asked(cls, recognition_kwargs, return_scores=False, char_boxes=None):
        """recognize()'s ``recognition_kwargs`` [and ``return_scores`` / ``char_boxes``] as they came, nothing checked;
        every other key is a Keras predict argument and has no effect on results"""
        kwargs = recognition_kwargs or {}
        return cls(scores=return_scores,
                   beam=None if kwargs.get("beam_width") is None else (kwargs["beam_width"], kwargs.get("top_paths", 1)),
                   lexicon_top=kwargs.get("lexicon_top"),
                   char_boxes=None if char_boxes is None or char_boxes is False else char_boxes,
                   orientation=None if kwargs.get("orientation") is None else (kwargs["orientation"], kwargs.get("tall_ratio", 1.5)),
                   charset=kwargs.get("charset"), pattern=kwargs.get("pattern"))

    @classmethod
    def from_recognition_kwargs(cls, recognizer, recognition_kwargs, return_scores=False, char_boxes=None, tiled=False):
        """``asked`` and validated, ``charset`` and ``pattern`` resolved through ``recognizer``; ``tiled``: for recognize_tiled"""
        return cls.asked(recognition_kwargs, return_scores, char_boxes).validate(KWARGS, recognizer, tiled=tiled)

    @classmethod
    def from_arguments(cls, recognizer, return_scores=False, beam_width=None, top_paths=1, lexicon_top=None, orientation=None,
                       tall_ratio=1.5, return_orientation=False, charset=None, pattern=None, box_groups=None):
        """``Recognizer.recognize``'s arguments (``box_groups`` None: ``charset`` and ``pattern`` are names) or
        ``recognize_from_boxes``' (names, or per image a list of one name or None per box), validated"""
        return cls(scores=return_scores, beam=None if beam_width is None else (beam_width, top_paths), lexicon_top=lexicon_top,
                   orientation=None if orientation is None else (orientation, tall_ratio), return_orientation=return_orientation,
                   charset=charset, pattern=pattern).validate(ARGUMENTS, recognizer, box_groups)

    def one_text_per_word(self, why):
        """ValueError for ``beam_width`` / ``lexicon_top`` / ``pattern``: the caller needs every ``text`` to be one string"""
        for key, value in (("beam_width", self.beam), ("lexicon_top", self.lexicon_top)):
            if value is not None:
                raise ValueError(f"{why}: {key} in recognition_kwargs makes every text a list of alternatives")
        if self.pattern is not None:
            raise ValueError(f"{why}: pattern in recognition_kwargs makes every text a (text, log_prob) pair")

    def charset_scope(self, ctx):
        """The scope of the one character set for every box alone; none: no call on ``ctx``, which may then be None"""
        return contextlib.nullcontext() if self.charset is None else ctx._extras_scope(Extras(charset=self.charset))  # pylint: disable=protected-access

    def _resolved(self, key, layer, recognizer, box_groups):
        """``charset`` / ``pattern`` (``key``): the name(s) -> the index for every box and the per-box indices"""
        name = getattr(self, key)
        module, hook, things, short = {"charset": (_charsets, "_charset_names", "character sets", "sets"),
                                       "pattern": (_patterns, "_pattern_names", "patterns", "patterns")}[key]
        if layer == KWARGS:
            if name is None:
                return self
            if not hasattr(recognizer, hook) or getattr(recognizer, "_ctx", None) is None:
                raise TypeError(f"{key}: the recognizer ({type(recognizer).__name__}) has no {things} (it is not libkocr-backed)")
            if not isinstance(name, str):
                raise ValueError(f"{key} in recognition_kwargs is one name for every box, got {name!r} (per-box {short}: "
                                 "Recognizer.recognize_from_boxes)")
        names = getattr(recognizer, hook)(name)  # ValueError when nothing is loaded
        one, per_box = (module.index_of(names, name), None) if box_groups is None else module.per_box(names, name, box_groups)
        return dataclasses.replace(self, **{key: one, {"charset": "set_of", "pattern": "pattern_of"}[key]: per_box})

    def checked_lexicon_top(self):
        if self.lexicon_top is None:
            return None
        if self.beam is not None:
            raise ValueError("lexicon_top and beam_width cannot be combined: ask for one of the two")
        return _lexicon.top_arg(self.lexicon_top)

    def checked_beam(self):
        return None if self.beam is None else _lib.beam_args(*self.beam)

    def checked_orientation(self, layer=KWARGS):
        """The orientation with its tall_ratio as a float (at the Context: its mode as the code); beam alternatives, lexicon
        matches, character boxes and pattern readings describe ONE reading"""
        if self.orientation is None:
            return None
        others = {"beam" if layer == CONTEXT else "beam_width": self.beam, "lexicon_top": self.lexicon_top, "char_boxes": self.char_boxes,
                  "pattern": True if layer == CONTEXT and self.patterned else None}
        for name, value in others.items():
            if value is not None and value is not False:
                raise ValueError(f"orientation and {name} cannot be combined: ask for one of the two")
        code, ratio = _lib.orientation_args(*self.orientation)
        return (code if layer == CONTEXT else self.orientation[0]), ratio

    def validate(self, layer=CONTEXT, recognizer=None, box_groups=None, tiled=False):
        """The record with every argument checked and normalised, or the refusal that comes first.  Where two refusals apply
        to one call, the earlier row of this table is raised; K = Pipeline (``from_recognition_kwargs``), A = Recognizer
        (``from_arguments``), C = Context:

        ==  =====  ==========================================================================================================
         1  K A    pattern with beam_width / lexicon_top (K: "a pattern gives one reading per word"), charset, orientation
         2  K A    the pattern name(s): not libkocr-backed (K, TypeError), not one name (K), nothing loaded, unknown
         3  K A    the charset name(s), likewise (A without boxes, ``Recognizer.recognize``: in row 7)
         4  K A    lexicon_top with beam_width; lexicon_top out of range
         5  A      lexicon_top without a loaded lexicon
         6  K A C  beam_width / top_paths out of range
         7  A      ``Recognizer.recognize``'s charset name (row 3)
         8  K      tiled, with character boxes: beam_width / lexicon_top / pattern (one text per word), return_scores
         9  K A C  orientation with beam_width (C: beam), lexicon_top, char_boxes, pattern (C); orientation / tall_ratio invalid
        10  A      return_orientation without orientation
        11  C      pattern or pattern_of with set_of; pattern with pattern_of
        12  K      lexicon_top without a loaded lexicon (the route for zero images included)
        ==  =====  ==========================================================================================================

        Before row 1 come the one-text-per-word refusals of ``Pipeline.evaluate``, ``recognize_lines``, ``recognize_table`` and
        ``recognize_characters`` (``one_text_per_word``); behind row 12 whatever needs the images (``only_uint8``)."""
        x = self
        if layer != CONTEXT:
            if x.pattern is not None and layer == KWARGS:
                dataclasses.replace(x, pattern=None).one_text_per_word("a pattern gives one reading per word")
            for name, value in (("beam_width", x.beam), ("lexicon_top", x.lexicon_top), ("charset", x.charset), ("orientation", x.orientation)):
                if x.pattern is not None and value is not None:
                    raise _pattern_and(name)
            x = x._resolved("pattern", layer, recognizer, box_groups)
            if layer == KWARGS or box_groups is not None:
                x = x._resolved("charset", layer, recognizer, box_groups)
            x = dataclasses.replace(x, lexicon_top=x.checked_lexicon_top())
            if layer == ARGUMENTS and x.lexicon_top is not None and (
                    recognizer.lexicon is None or recognizer._ctx.lexicon_size() != len(recognizer.lexicon)):  # pylint: disable=protected-access
                raise ValueError("lexicon_top needs a loaded lexicon: call Recognizer.set_lexicon(words) first (a lexicon is "
                                 "unloaded when a recogniser of another class count is loaded on its context)")
        x = dataclasses.replace(x, beam=x.checked_beam())
        if layer == ARGUMENTS and box_groups is None:
            x = x._resolved("charset", layer, recognizer, box_groups)
        if tiled and x.characters:
            x.one_text_per_word("character boxes pair one text per word with its characters")
            if x.scores:
                raise ValueError("return_scores and char_boxes cannot be combined: ask for one of the two")
        x = dataclasses.replace(x, orientation=x.checked_orientation(layer))
        if x.return_orientation and x.orientation is None:
            raise ValueError("return_orientation=True needs orientation='flip' or 'any'")
        if x.patterned and x.set_of is not None and layer == CONTEXT:
            raise _pattern_and("set_of")
        if x.pattern is not None and x.pattern_of is not None:
            raise ValueError("pattern and pattern_of cannot be combined: one pattern for every box, or one per box")
        if layer == KWARGS and x.lexicon_top is not None and getattr(recognizer, "lexicon", None) is None:
            raise ValueError("lexicon_top needs a loaded lexicon: call recognizer.set_lexicon(words) first")
        return x

    def empty_results(self, label_width):
        """The ``Results`` of zero images under this record"""
        return Results.empty(self.scores, self.beam, self.lexicon_top, self.characters, label_width=label_width,
                             orientation=self.orientation is not None, pattern=self.patterned)

    def flags(self):
        """What ``Results.parse_context`` takes behind the tuple"""
        return (self.scores, self.beam is not None, self.lexicon_top is not None, self.characters, self.orientation is not None,
                self.patterned)
