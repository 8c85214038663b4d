"""CPU suite: the per-call extras.  Part 1: where two or more refusals apply to one call, the one that is raised -- a table
of public calls over the doubles of ``test_result_shapes_cpu`` (fused, stage-wise and zero-image routes) and over a
``Recognizer`` without a context; every row was first confirmed on the commit before ``extras.Extras`` existed.  Part 2:
``Context._extras_scope`` on a stub of the library that records every ``kocr_set_*`` / ``kocr_get_*`` call."""
import numpy as np
import pytest

import keras_ocr_amd as k
from tests.test_result_shapes_cpu import SHAPES, _fused, _pages, _stagewise

ALTERNATIVES = "{key} in recognition_kwargs makes every text a list of alternatives"
BOTH = "lexicon_top and beam_width cannot be combined: ask for one of the two"
NO_LEXICON = "lexicon_top needs a loaded lexicon: call recognizer.set_lexicon(words) first"
ONE_TEXT = {
    "evaluate": "evaluate scores one text per word: ",
    "recognize_lines": "recognize_lines joins one text per word: ",
    "recognize_table": "recognize_table joins one text per word: ",
    "recognize_characters": "recognize_characters pairs one text per word with its characters: ",
}

# (method, keyword arguments, whether the recogniser has its lexicon, exception, message)
PIPELINE_ROWS = [
    # pattern's refusals before the charset lookup (and before the pattern's own)
    ("recognize", {"recognition_kwargs": {"pattern": "nope", "charset": "nope"}}, True, ValueError,
     "pattern and charset cannot be combined: the pattern states the characters itself"),
    ("recognize_raw", {"recognition_kwargs": {"pattern": "nope", "charset": "nope", "beam_width": 0}}, True, ValueError,
     "a pattern gives one reading per word: " + ALTERNATIVES.format(key="beam_width")),
    ("recognize_with_scores", {"recognition_kwargs": {"pattern": "nope", "orientation": "sideways", "lexicon_top": 2}}, False, ValueError,
     "a pattern gives one reading per word: " + ALTERNATIVES.format(key="lexicon_top")),
    ("recognize", {"recognition_kwargs": {"pattern": "nope", "orientation": "sideways"}}, True, ValueError,
     "pattern and orientation cannot be combined: ask for one of the two"),
    # "lexicon_top and beam_width" before "needs a loaded lexicon", and before either argument's range
    ("recognize", {"recognition_kwargs": {"lexicon_top": 2, "beam_width": 4}}, False, ValueError, BOTH),
    ("recognize_raw", {"recognition_kwargs": {"lexicon_top": 0, "beam_width": 0, "orientation": "any"}}, False, ValueError, BOTH),
    # the ranges before the orientation's refusals, those before the missing lexicon
    ("recognize", {"recognition_kwargs": {"lexicon_top": 0, "orientation": "any"}}, False, ValueError, "lexicon_top 0 outside [1, 64]"),
    ("recognize", {"recognition_kwargs": {"beam_width": 0, "orientation": "any"}}, True, ValueError, "beam_width 0 outside [1, 64]"),
    ("recognize_raw", {"recognition_kwargs": {"beam_width": 4, "orientation": "sideways"}, "char_boxes": True}, True, ValueError,
     "orientation and beam_width cannot be combined: ask for one of the two"),
    ("recognize_raw", {"recognition_kwargs": {"lexicon_top": 2, "orientation": "sideways"}, "char_boxes": True}, False, ValueError,
     "orientation and lexicon_top cannot be combined: ask for one of the two"),
    ("recognize_raw", {"recognition_kwargs": {"orientation": "sideways"}, "char_boxes": True}, True, ValueError,
     "orientation and char_boxes cannot be combined: ask for one of the two"),
    ("recognize", {"recognition_kwargs": {"lexicon_top": 2, "orientation": "sideways"}}, False, ValueError,
     "orientation and lexicon_top cannot be combined: ask for one of the two"),
    ("recognize", {"recognition_kwargs": {"lexicon_top": 2, "tall_ratio": 0}}, False, ValueError, NO_LEXICON),
    # the one-text-per-word refusals before anything else
    *[(method, {"recognition_kwargs": {"beam_width": 0, "lexicon_top": 2, "orientation": "sideways"}}, False, ValueError,
       text + ALTERNATIVES.format(key="beam_width")) for method, text in ONE_TEXT.items()],
    *[(method, {"recognition_kwargs": {"lexicon_top": 0, "pattern": "nope", "charset": "nope"}}, False, ValueError,
       text + ALTERNATIVES.format(key="lexicon_top")) for method, text in ONE_TEXT.items()],
    *[(method, {"recognition_kwargs": {"pattern": "nope", "charset": "nope", "orientation": "sideways"}}, True, ValueError,
       text + "pattern in recognition_kwargs makes every text a (text, log_prob) pair") for method, text in ONE_TEXT.items()],
    ("recognize_characters", {"recognition_kwargs": {"orientation": "any", "charset": "nope"}, "no_such_rule": 1}, True, ValueError,
     "orientation and char_boxes cannot be combined: ask for one of the two"),
    # tiled pages: character boxes want one text per word and no scores, before the orientation's refusals
    ("recognize_tiled", {"recognition_kwargs": {"beam_width": 4, "orientation": "any"}, "char_boxes": True, "return_scores": True},
     True, ValueError, "character boxes pair one text per word with its characters: " + ALTERNATIVES.format(key="beam_width")),
    ("recognize_tiled", {"recognition_kwargs": {"orientation": "any"}, "char_boxes": True, "return_scores": True}, True, ValueError,
     "return_scores and char_boxes cannot be combined: ask for one of the two"),
    ("recognize_tiled", {"recognition_kwargs": {"lexicon_top": 2, "beam_width": 4}, "char_boxes": True, "return_scores": True},
     False, ValueError, BOTH),
    ("recognize_tiled", {"recognition_kwargs": {"lexicon_top": 2}, "tile": 7}, False, ValueError, NO_LEXICON),
]


@pytest.mark.parametrize("route", ["fused", "stagewise", "zero"])
@pytest.mark.parametrize("method,kwargs,lexicon,error,message", PIPELINE_ROWS)
def test_precedence_in_pipeline(monkeypatch, route, method, kwargs, lexicon, error, message):
    pipe = _stagewise(monkeypatch) if route == "stagewise" else _fused()
    if not lexicon:
        pipe.recognizer.lexicon = None
    images = [] if route == "zero" else _pages()
    args = (images, [[]] * len(images)) if method == "evaluate" else (images,)
    with pytest.raises(error) as err:
        getattr(pipe, method)(*args, **kwargs)
    assert type(err.value) is error and str(err.value) == message
    assert getattr(getattr(pipe.detector, "_ctx", None), "seen", []) == []


@pytest.mark.parametrize("route", ["fused", "stagewise", "zero"])
def test_the_charset_lookup_comes_before_everything_behind_it(monkeypatch, route):
    pipe = _stagewise(monkeypatch) if route == "stagewise" else _fused()
    error, message = (TypeError, "charset: the recognizer (_Recognizer) has no character sets (it is not libkocr-backed)") \
        if route == "stagewise" else (ValueError, "charset in recognition_kwargs is one name for every box, got ['a'] (per-box sets: "
                                                  "Recognizer.recognize_from_boxes)")
    for call in (pipe.recognize, pipe.recognize_raw, pipe.recognize_tiled):
        with pytest.raises(error) as err:
            call([] if route == "zero" else _pages(), recognition_kwargs={"charset": ["a"], "lexicon_top": 2, "beam_width": 4})
        assert type(err.value) is error and str(err.value) == message
    assert getattr(getattr(pipe.detector, "_ctx", None), "seen", []) == []


LOADED = "needs a loaded lexicon: call Recognizer.set_lexicon(words) first (a lexicon is unloaded when a recogniser of another " \
         "class count is loaded on its context)"
NO_SETS = "charset needs loaded character sets: call Recognizer.set_charsets({name: characters}) first (the sets are unloaded " \
          "when a recogniser of another class count is loaded on their context)"
NO_PATTERNS = "pattern needs loaded patterns: call Recognizer.set_patterns({name: regex}) first (the patterns are unloaded when " \
              "a recogniser of another class count is loaded on their context)"
RECOGNIZER_ROWS = [
    ("recognize_from_boxes", {"pattern": "p", "beam_width": 0, "lexicon_top": 0, "charset": "c"},
     "pattern and beam_width cannot be combined: ask for one of the two"),
    ("recognize_from_boxes", {"pattern": "p", "lexicon_top": 0, "orientation": "sideways"},
     "pattern and lexicon_top cannot be combined: ask for one of the two"),
    ("recognize_from_boxes", {"pattern": "p", "charset": "c", "orientation": "sideways"},
     "pattern and charset cannot be combined: the pattern states the characters itself"),
    ("recognize_from_boxes", {"pattern": "p", "orientation": "sideways", "return_orientation": True},
     "pattern and orientation cannot be combined: ask for one of the two"),
    ("recognize_from_boxes", {"pattern": "p", "return_orientation": True}, NO_PATTERNS),
    ("recognize_from_boxes", {"charset": "c", "lexicon_top": 2, "beam_width": 4}, NO_SETS),  # the sets before the lexicon ...
    ("recognize", {"charset": "c", "lexicon_top": 2, "beam_width": 4}, BOTH),                # ... but not for one crop
    ("recognize", {"charset": "c", "beam_width": 0}, "beam_width 0 outside [1, 64]"),
    ("recognize", {"charset": "c", "beam_width": 4}, NO_SETS),
    ("recognize", {"pattern": "p", "beam_width": 0, "charset": "c"}, "pattern and beam_width cannot be combined: ask for one of the two"),
    ("recognize_from_boxes", {"lexicon_top": 2, "beam_width": 0, "orientation": "flip"}, BOTH),
    ("recognize_from_boxes", {"lexicon_top": 0, "orientation": "flip"}, "lexicon_top 0 outside [1, 64]"),
    ("recognize_from_boxes", {"lexicon_top": 2, "orientation": "flip"}, "lexicon_top " + LOADED),
    ("recognize_from_boxes", {"beam_width": 0, "orientation": "flip", "return_orientation": True}, "beam_width 0 outside [1, 64]"),
    ("recognize_from_boxes", {"beam_width": 4, "orientation": "sideways"},
     "orientation and beam_width cannot be combined: ask for one of the two"),
    ("recognize_from_boxes", {"return_orientation": True, "tall_ratio": 0}, "return_orientation=True needs orientation='flip' or 'any'"),
    ("recognize_from_boxes", {"return_orientation": True, "orientation": "any", "tall_ratio": 0}, "tall_ratio 0 must be finite and positive"),
]


@pytest.mark.parametrize("method,kwargs,message", RECOGNIZER_ROWS)
def test_precedence_in_recognizer(method, kwargs, message):
    """A ``Recognizer`` with nothing loaded and no context: every refusal here comes before the context is touched"""
    rec = object.__new__(k.recognition.Recognizer)
    rec.alphabet, rec.lexicon, rec.charsets, rec.patterns, rec._ctx = "abc", None, None, None, None  # pylint: disable=protected-access
    page = np.zeros((8, 8, 3), np.uint8)
    args = ([page], [np.zeros((1, 4, 2), np.float32)]) if method == "recognize_from_boxes" else (page,)
    with pytest.raises(ValueError) as err:
        getattr(rec, method)(*args, **kwargs)
    assert type(err.value) is ValueError and str(err.value) == message


def test_the_zero_image_route_still_refuses_a_missing_lexicon():
    pipe = _fused()
    pipe.recognizer.lexicon = None
    for call in (pipe.recognize, pipe.recognize_with_scores, pipe.recognize_raw):
        with pytest.raises(ValueError) as err:
            call([], recognition_kwargs={"lexicon_top": 2})
        assert str(err.value) == NO_LEXICON
    assert pipe.detector._ctx.seen == [] and len(SHAPES) == len(_pages())  # pylint: disable=protected-access


# ---- part 2: the scope over a context's switches, on a recording stub ---------------------------------------------------------
class _Library:
    """Every ``kocr_*`` call is recorded as ``(name, values)``; getters answer from ``state``; ``fail`` names a setter that
    answers KOCR_EINVAL; ``loaded``: what the three count getters answer"""

    def __init__(self, fail=None, loaded=1):
        self.calls, self.fail, self.loaded = [], fail, loaded
        self.state = {"kocr_get_char_boxes": (0, 0.4, 0.7, 0.2), "kocr_get_beam": (0, 1), "kocr_get_lexicon_match": (0,),
                      "kocr_get_orientation": (0, 1.5), "kocr_get_charset": (-1,), "kocr_get_pattern": (-1,)}

    def __getattr__(self, name):
        def call(handle, *args):
            assert handle == "handle"
            if name == "kocr_last_error":
                return b"refused"
            if name in self.state:  # a getter with out-parameters
                self.calls.append((name, ()))
                for arg, value in zip(args, self.state[name]):
                    arg._obj.value = value  # pylint: disable=protected-access
                return 0
            self.calls.append((name, args))
            if name in ("kocr_lexicon_size", "kocr_charset_count", "kocr_pattern_count"):
                return self.loaded
            return -1 if name == self.fail else 0
        return call


def _context(**kw):
    ctx = k.Context.__new__(k.Context)
    ctx._lib, ctx._h = _Library(**kw), "handle"  # pylint: disable=protected-access
    return ctx


def _names(ctx):
    return [name for name, _ in ctx._lib.calls]  # pylint: disable=protected-access


def _full():
    from keras_ocr_amd.extras import Extras
    return Extras(scores=True, beam=(4, 2), lexicon_top=3, char_boxes={"peak_threshold": 0.5}, orientation=("any", 2.0), charset=1,
                  pattern=2, min_area_rect="opencv", return_orientation=True, set_of=[0], pattern_of=[0])


SWITCHES = [  # in the table's order: field, value, getter, setter, the count getter of its "unloaded meanwhile" rule
    ("char_boxes", True, "kocr_get_char_boxes", "kocr_set_char_boxes", None),
    ("min_area_rect", "opencv", "kocr_get_min_area_rect", "kocr_set_min_area_rect", None),
    ("scores", True, "kocr_get_scores", "kocr_set_scores", None),
    ("beam", (4, 2), "kocr_get_beam", "kocr_set_beam", None),
    ("lexicon_top", 3, "kocr_get_lexicon_match", "kocr_set_lexicon_match", "kocr_lexicon_size"),
    ("orientation", ("any", 2.0), "kocr_get_orientation", "kocr_set_orientation", None),
    ("charset", 1, "kocr_get_charset", "kocr_set_charset", "kocr_charset_count"),
    ("pattern", 2, "kocr_get_pattern", "kocr_set_pattern", "kocr_pattern_count"),
]


def test_an_all_default_record_makes_no_call():
    from keras_ocr_amd.extras import Extras
    ctx = _context()
    for extras in (Extras(), Extras(scores=False, char_boxes=None, return_orientation=True, set_of=[1], pattern_of=[0])):
        with ctx._extras_scope(extras):  # pylint: disable=protected-access
            pass
    assert ctx._lib.calls == []  # pylint: disable=protected-access


@pytest.mark.parametrize("field,value,getter,setter,count", SWITCHES)
def test_a_single_field_touches_only_its_own_switch(field, value, getter, setter, count):
    from keras_ocr_amd.extras import Extras
    ctx = _context()
    with ctx._extras_scope(Extras(**{field: value})):  # pylint: disable=protected-access
        assert _names(ctx) == [getter, setter]
    restore = [setter, setter] if field == "char_boxes" else [setter]
    assert _names(ctx) == [getter, setter] + ([count] if count else []) + restore


def test_a_full_record_sets_in_the_tables_order_and_restores_in_reverse():
    ctx = _context()
    with ctx._extras_scope(_full()):  # pylint: disable=protected-access
        entered = list(ctx._lib.calls)  # pylint: disable=protected-access
        assert [name for name, _ in entered] == [name for _, _, get, set_, _ in SWITCHES for name in (get, set_)]
    left = ctx._lib.calls[len(entered):]  # pylint: disable=protected-access
    setters = [name for name, _ in left if "_set_" in name]
    assert setters == [set_ for _, _, _, set_, _ in reversed(SWITCHES)] + ["kocr_set_char_boxes"]
    values = dict(entered)
    assert values["kocr_set_beam"] == (4, 2) and values["kocr_set_lexicon_match"] == (3,) and values["kocr_set_scores"] == (1,)
    assert values["kocr_set_charset"] == (1,) and values["kocr_set_pattern"] == (2,) and values["kocr_set_min_area_rect"] == (1,)
    assert values["kocr_set_orientation"] == (2, 2.0) and values["kocr_set_char_boxes"] == (1, 0.5, 0.7, 0.2)
    # every switch gets back what its getter answered
    assert dict(left)["kocr_set_beam"] == (0, 1) and dict(left)["kocr_set_orientation"] == (0, 1.5)
    assert dict(left)["kocr_set_charset"] == (-1,) and dict(left)["kocr_set_pattern"] == (-1,) and dict(left)["kocr_set_lexicon_match"] == (0,)


def test_a_setter_that_fails_restores_those_already_set():
    ctx = _context(fail="kocr_set_lexicon_match")
    with pytest.raises(ValueError, match="refused"):
        with ctx._extras_scope(_full()):  # pylint: disable=protected-access
            raise AssertionError("the scope is not entered")
    names = _names(ctx)
    at = names.index("kocr_set_lexicon_match")
    assert names[:at + 1] == [name for _, _, get, set_, _ in SWITCHES[:5] for name in (get, set_)]
    assert names[at + 1:] == ["kocr_set_beam", "kocr_set_scores", "kocr_set_min_area_rect", "kocr_set_char_boxes", "kocr_set_char_boxes"]


def test_what_was_unloaded_meanwhile_is_not_restored():
    ctx = _context(loaded=0)  # the lexicon is gone; no table holds the old index -1 + 1 either
    ctx._lib.state.update({"kocr_get_charset": (0,), "kocr_get_pattern": (0,)})  # pylint: disable=protected-access
    with ctx._extras_scope(_full()):  # pylint: disable=protected-access
        entered = len(ctx._lib.calls)  # pylint: disable=protected-access
    left = _names(ctx)[entered:]
    assert [n for n in left if n in ("kocr_set_pattern", "kocr_set_charset", "kocr_set_lexicon_match")] == []
    assert [n for n in left if n.endswith(("_count", "_size"))] == ["kocr_pattern_count", "kocr_charset_count", "kocr_lexicon_size"]
    assert "kocr_set_orientation" in left and "kocr_set_beam" in left


def test_the_character_box_rule_comes_back_parameters_first():
    from keras_ocr_amd.extras import Extras
    ctx = _context()
    ctx._lib.state["kocr_get_char_boxes"] = (0, 0.25, 0.5, 0.125)  # pylint: disable=protected-access
    with ctx._extras_scope(Extras(char_boxes=True)):  # pylint: disable=protected-access
        pass
    calls = ctx._lib.calls  # pylint: disable=protected-access
    assert calls == [("kocr_get_char_boxes", ()), ("kocr_set_char_boxes", (1, 0.4, 0.7, 0.2)),
                     ("kocr_set_char_boxes", (1, 0.25, 0.5, 0.125)), ("kocr_set_char_boxes", (0, 0.25, 0.5, 0.125))]
