"""CPU suite: ``results.Results`` -- its two tuple layouts are inverse to each other where one has an inverse, the Nones of the
``recognize_raw`` layout stand where that method's contract puts them, and the empty values have the documented shapes."""
import itertools

import numpy as np
import pytest

from keras_ocr_amd.results import Results

COMBOS = list(itertools.product((False, True), (None, "beam", "lexicon"), (False, True)))


def _record(with_scores, kind, with_characters):
    """Every field a distinct object, so that a swapped position cannot go unnoticed"""
    return Results(boxes=["boxes"], labels=np.zeros((1, 48), np.int32), scores=("detection", "log_word", "chars") if with_scores else None,
                   beam=("beam labels", "beam log_prob") if kind == "beam" else None,
                   lexicon=("index", "log_prob") if kind == "lexicon" else None, characters=[["characters"]] if with_characters else None)


@pytest.mark.parametrize("with_scores,kind,with_characters", COMBOS)
def test_parse_inverts_render_context(with_scores, kind, with_characters):
    r = _record(with_scores, kind, with_characters)
    out = r.render_context()
    assert isinstance(out, tuple) and len(out) == 2 + with_scores + (kind is not None) + with_characters
    assert all(v is not None for v in out) and out[0] is r.boxes and out[1] is r.labels
    assert not with_characters or out[-1] is r.characters
    back = Results.parse_context(out, with_scores, kind == "beam", kind == "lexicon", with_characters)
    assert back == r and back.render_context() == out
    for field in ("boxes", "labels", "scores", "beam", "lexicon", "characters"):
        assert getattr(back, field) is getattr(r, field)
    with pytest.raises(ValueError, match="do not fit"):
        Results.parse_context(out + ("one more",), with_scores, kind == "beam", kind == "lexicon", with_characters)
    with pytest.raises(ValueError, match="do not fit"):
        Results.parse_context(out, not with_scores, kind == "beam", kind == "lexicon", with_characters)


@pytest.mark.parametrize("with_scores,kind,with_characters", COMBOS)
def test_render_raw_pads_with_none(with_scores, kind, with_characters):
    """recognize_raw: scores third or None; with a beam four elements, the beam fourth; with a lexicon five, the fourth None,
    the lexicon fifth; the characters behind whatever there is"""
    r = _record(with_scores, kind, with_characters)
    out = r.render_raw()
    head = out[:-1] if with_characters else out
    assert isinstance(out, tuple) and (not with_characters or out[-1] is r.characters)
    assert len(head) == {None: 2 + with_scores, "beam": 4, "lexicon": 5}[kind]
    assert head[0] is r.boxes and head[1] is r.labels
    if len(head) > 2:
        assert head[2] is r.scores
    if kind == "beam":
        assert head[3] is r.beam
    if kind == "lexicon":
        assert head[3] is None and head[4] is r.lexicon


def test_both_alternatives_requested_means_the_lexicon():
    out = (["boxes"], "labels", ("index", "log_prob"))
    assert Results.parse_context(out, beam=True, lexicon=True) == Results(["boxes"], "labels", lexicon=out[2])


def test_detection_and_recognition_layouts():
    assert Results(["b"], None).render_detection() == ["b"]
    assert Results(["b"], None, scores=("d", None, None)).render_detection() == (["b"], "d")
    assert Results(["b"], None, characters=["c"]).render_detection() == (["b"], ["c"])
    assert Results(["b"], None, scores=("d", None, None), characters=["c"]).render_detection() == (["b"], "d", ["c"])
    assert Results(None, "l").render_recognition() == "l"
    assert Results(None, "l", scores=(None, "w", "c")).render_recognition() == ("l", "w", "c")
    assert Results(None, "l", beam=("bl", "bp")).render_recognition() == ("l", "bl", "bp")
    assert Results(None, "l", scores=(None, "w", "c"), beam=("bl", "bp"), lexicon=("i", "p")).render_recognition() == \
        ("l", "w", "c", "bl", "bp", "i", "p")


def test_empty_values():
    e = Results.empty(scores=True, beam=(4, 3), lexicon=None, characters=True)
    assert e.boxes == [] and e.characters == [] and e.lexicon is None
    assert (e.labels.dtype, e.labels.shape) == (np.int32, (0, 48))
    assert e.scores[0] == [] and [(a.dtype, a.shape) for a in e.scores[1:]] == [(np.float32, (0,)), (np.float32, (0, 48))]
    assert [(a.dtype, a.shape) for a in e.beam] == [(np.int32, (0, 3, 48)), (np.float32, (0, 3))]
    e = Results.empty(lexicon=5)
    assert e.scores is None and e.beam is None and e.characters is None
    assert [(a.dtype, a.shape) for a in e.lexicon] == [(np.int32, (0, 5)), (np.float32, (0, 5))]
    assert e.render_raw()[2:4] == (None, None) and len(e.render_raw()) == 5


def test_concatenate_joins_every_field_by_name():
    def part(m):
        return Results(None, np.full((m, 48), m, np.int32), scores=(None, np.full(m, m, np.float32), np.full((m, 48), m, np.float32)),
                       lexicon=(np.full((m, 2), m, np.int32), np.full((m, 2), m, np.float32)))
    both = Results.concatenate([part(1), part(2)])
    assert both.boxes is None and both.beam is None and both.scores[0] is None
    assert both.labels.shape == (3, 48) and both.labels[:, 0].tolist() == [1, 2, 2]
    assert both.scores[1].tolist() == [1, 2, 2] and both.scores[2].shape == (3, 48)
    assert both.lexicon[0].shape == (3, 2) and both.lexicon[1][:, 0].tolist() == [1, 2, 2]
