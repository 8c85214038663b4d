"""Word orientation without a GPU ("Orientation"): the statement tests/orientation_statement.py by hand,
the choice rule on chosen rows, the Results record with and without the new field, and every refusal the Python layer makes
before it reaches the library."""
import numpy as np
import pytest

from tests import orientation_statement as st


def _rect(x0, y0, w, h):
    return np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]], np.float32)


def _rotated(cx, cy, w, h, degrees):
    a = np.radians(degrees)
    r = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    pts = np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]]) @ r.T + [cx, cy]
    return pts.astype(np.float32)


def _same_corners(quads, ob):
    key = lambda q: sorted(map(tuple, np.asarray(q).tolist()))  # noqa: E731
    return all(key(q) == key(ob) for q in quads)


def test_wide_box_flips_and_is_never_turned_sideways():
    from oracle import tools as otools

    box = _rect(10, 20, 60, 20)
    ob, _ = otools.get_rotated_box(box)
    for mode in st.MODES:
        turns, quads = st.candidates(box, mode)
        assert turns.tolist() == [0, 2]
        assert np.array_equal(quads[0], ob)  # turn 0 is today's ordered box, bit for bit
        assert np.array_equal(quads[1], ob[[2, 3, 0, 1]])
        assert quads.dtype == np.float32 and _same_corners(quads, ob)


def test_tall_box_is_read_down_and_up_the_page_only_in_mode_any():
    from oracle import tools as otools

    box = _rect(30, 5, 12, 80)
    ob, _ = otools.get_rotated_box(box)
    assert otools.get_rotated_width_height(ob) == (12, 80)
    turns, quads = st.candidates(box, "any")
    assert turns.tolist() == [1, 3]
    assert np.array_equal(quads[0], ob[[1, 2, 3, 0]]) and np.array_equal(quads[1], ob[[3, 0, 1, 2]])
    assert _same_corners(quads, ob)
    # turn 1 starts at the detector's tr and reads towards its br: down the page; turn 3 from bl towards tl: up the page
    assert quads[0][1][1] > quads[0][0][1] and quads[1][1][1] < quads[1][0][1]
    # the width and height of an odd turn are the swapped pair
    for q in quads:
        assert otools.get_rotated_width_height(q) == (80, 12)
    turns, quads = st.candidates(box, "flip")
    assert turns.tolist() == [0, 2]  # "flip" never gives odd turns
    assert otools.get_rotated_width_height(quads[1]) == (12, 80)


def test_a_box_exactly_at_the_ratio_counts_as_tall():
    assert st.candidates(_rect(0, 0, 20, 30), "any", 1.5)[0].tolist() == [1, 3]  # h == 1.5 w exactly
    assert st.candidates(_rect(0, 0, 20, 29), "any", 1.5)[0].tolist() == [0, 2]
    assert st.candidates(_rect(0, 0, 20, 29), "any", 1.45)[0].tolist() == [1, 3]
    assert st.candidates(_rect(0, 0, 20, 30), "flip", 1.5)[0].tolist() == [0, 2]
    with pytest.raises(ValueError):
        st.candidates(_rect(0, 0, 20, 30), "sideways")


def test_rotated_box_keeps_its_corners_and_swaps_its_sides():
    from oracle import tools as otools

    for w, h, want in ((60, 20, [0, 2]), (16, 70, [1, 3])):
        box = _rotated(64, 48, w, h, 30)
        ob, _ = otools.get_rotated_box(box)
        w0, h0 = otools.get_rotated_width_height(ob)
        turns, quads = st.candidates(box, "any")
        assert turns.tolist() == [int(h0 >= 1.5 * w0), int(h0 >= 1.5 * w0) + 2]
        assert _same_corners(quads, ob)
        for t, q in zip(turns, quads):
            assert np.array_equal(q, ob[[(i + t) % 4 for i in range(4)]])
            assert otools.get_rotated_width_height(q) == ((h0, w0) if t % 2 else (w0, h0))
            # every candidate is a rectangle walked in the same sense: consecutive corners share a side
            assert np.array_equal(np.roll(q, -2, axis=0), quads[1] if t == turns[0] else quads[0])
        del want


def test_crops_of_turn_0_are_the_crop_stage_of_today_and_turn_2_is_its_half_turn():
    from oracle import tools as otools
    from tests import synth

    page = synth.text_page(96, 128, 5, seed=21)
    gray = otools.rgb2gray_u8(page)
    boxes = np.stack([_rect(10, 20, 60, 20), _rect(30, 5, 12, 80)])
    got, turns, quads = st.crops(page, boxes, "any")
    assert got.shape == (4, 31, 200) and got.dtype == np.float32 and turns.tolist() == [0, 2, 1, 3] and quads.shape == (4, 4, 2)
    assert np.array_equal(got[0], otools.warp_box(gray, boxes[0], 31, 200).astype("float32") / 255)
    (w, h), scale, _, _, (cw, ch) = st.quad_params(quads[2])
    assert (w, h) == (80, 12) and (cw, ch) == (200, 30) and scale == 2.5  # the tall box fills the crop instead of a sliver
    with pytest.raises(ZeroDivisionError):
        st.crops(page, np.stack([_rect(5, 5, 0.5, 40)]), "any")


def test_select_rule():
    lab = np.full((8, 2, 5), -1, np.int64)
    v = np.zeros((8, 2), np.float32)
    lab[0, 1, :2] = [3, 4]; v[0] = (-0.1, -9.0)          # candidate 0 empty, 1 not: 1 wins whatever the values  # noqa: E702
    lab[1, 0, :2] = [3, 4]; v[1] = (-9.0, -0.1)          # candidate 1 empty: 0 wins whatever the values  # noqa: E702
    v[2] = (-3.0, -1.0)                                   # both empty: the larger value  # noqa: E702
    lab[3, :, 0] = 1; v[3] = (-2.0, -2.0)                 # a tie keeps candidate 0  # noqa: E702
    lab[4, :, 0] = 1; v[4] = (-2.0, np.nan)               # NaN keeps candidate 0  # noqa: E702
    lab[5, :, 0] = 1; v[5] = (np.nan, -2.0)               # ... on either side  # noqa: E702
    lab[6, :, 0] = 1; v[6] = (-np.inf, -50.0)             # -inf loses to a finite value  # noqa: E702
    lab[7, :, 0] = 1; v[7] = (-np.inf, -np.inf)           # and ties with itself  # noqa: E702
    assert st.select(lab, v).tolist() == [1, 0, 1, 0, 0, 0, 1, 0]
    assert st.select(lab[:0], v[:0]).shape == (0,)


def test_results_record_keeps_its_layouts_and_appends_orientation_last():
    from keras_ocr_amd.results import Results, empty_orientation

    plain = Results(["b"], "l", scores=("d", "w", "c"), lexicon=("i", "p"), characters=["ch"])
    assert plain.orientation is None
    assert plain.render_context() == (["b"], "l", ("d", "w", "c"), ("i", "p"), ["ch"])
    assert plain.render_raw() == (["b"], "l", ("d", "w", "c"), None, ("i", "p"), ["ch"])
    assert Results(None, "l").render_recognition() == "l"
    assert Results(None, "l", scores=(None, "w", "c")).render_recognition() == ("l", "w", "c")
    assert Results(["b"], "l").render_context() == (["b"], "l") and Results(["b"], "l").render_raw() == (["b"], "l")
    how = ("t", "q", "v")
    turned = Results(["b"], "l", scores=("d", "w", "c"), orientation=how)
    assert turned.render_context() == (["b"], "l", ("d", "w", "c"), how)
    assert turned.render_raw() == (["b"], "l", ("d", "w", "c"), how)
    assert Results(["b"], "l", orientation=how).render_raw() == (["b"], "l", how)
    assert Results(None, "l", orientation=how).render_recognition() == ("l", "t", "q", "v")
    assert Results(None, "l", scores=(None, "w", "c"), orientation=how).render_recognition() == ("l", "w", "c", "t", "q", "v")
    assert Results.parse_context(turned.render_context(), scores=True, orientation=True) == turned
    assert Results.parse_context((["b"], "l")) == Results(["b"], "l")
    with pytest.raises(ValueError):
        Results.parse_context(turned.render_context(), scores=True)
    turns, quads, pairs = empty_orientation()
    assert (turns.shape, turns.dtype, quads.shape, quads.dtype, pairs.shape, pairs.dtype) == \
        ((0,), np.int32, (0, 4, 2), np.float32, (0, 2), np.float32)
    assert Results.empty().orientation is None and len(Results.empty().render_raw()) == 2 and len(Results.empty(orientation=True).render_raw()) == 3
    assert [a.shape for a in Results.empty(orientation=True).orientation] == [(0,), (0, 4, 2), (0, 2)]
    parts = [Results(None, np.zeros((m, 48), np.int32), orientation=(np.full(m, m, np.int32), np.zeros((m, 4, 2), np.float32),
                                                                      np.zeros((m, 2), np.float32))) for m in (2, 3)]
    joined = Results.concatenate(parts)
    assert joined.orientation[0].tolist() == [2, 2, 3, 3, 3] and joined.orientation[1].shape == (5, 4, 2) and joined.scores is None
    assert Results.concatenate([Results(None, np.zeros((1, 48), np.int32))]).orientation is None


def test_arguments_are_validated_without_a_gpu():
    from keras_ocr_amd import _lib, pipeline

    assert _lib.orientation_args("flip") == (1, 1.5) and _lib.orientation_args("any", 2) == (2, 2.0)
    for bad in ("up", 1, None, True):
        with pytest.raises(ValueError, match="orientation"):
            _lib.orientation_args(bad)
    for bad in (0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="tall_ratio"):
            _lib.orientation_args("any", bad)
    assert pipeline.orientation_of(None) is None and pipeline.orientation_of({"batch_size": 4, "tall_ratio": 3}) is None
    assert pipeline.orientation_of({"orientation": "any"}) == ("any", 1.5)
    assert pipeline.orientation_of({"orientation": "flip", "tall_ratio": 2, "verbose": 0}) == ("flip", 2.0)
    with pytest.raises(ValueError, match="tall_ratio"):
        pipeline.orientation_of({"orientation": "any", "tall_ratio": 0})
    for other in ({"beam_width": 4}, {"lexicon_top": 2}):
        with pytest.raises(ValueError, match=f"orientation and {list(other)[0]}"):
            pipeline.orientation_of({"orientation": "any", **other})
    with pytest.raises(ValueError, match="orientation and char_boxes"):
        pipeline.orientation_of({"orientation": "any"}, char_boxes=True)


def test_python_layer_refuses_without_a_gpu(monkeypatch):
    import keras_ocr_amd as k
    from keras_ocr_amd import pipeline

    page = [np.zeros((8, 8, 3), np.uint8)]
    turned = {"orientation": "any"}
    sharded = k.dist.ShardedPipeline(pipeline=None)
    with pytest.raises(NotImplementedError, match="orientation"):
        sharded.recognize(page, recognition_kwargs=turned)

    class Rec:
        alphabet = "abc"
        lexicon = object()

        def recognize_from_boxes(self, images, box_groups, return_scores=False):
            raise AssertionError("refused before it is called")

    class Det:
        def detect(self, images, **kw):
            return [np.zeros((1, 4, 2), np.float32) for _ in images]

    pipe = pipeline.Pipeline(detector=Det(), recognizer=Rec())
    for method in (pipe.recognize, pipe.recognize_with_scores, pipe.recognize_lines, pipe.recognize_raw):
        for other in ({"beam_width": 4}, {"lexicon_top": 2}):
            with pytest.raises(ValueError, match="orientation|one text per word|joins one text"):
                method(page, recognition_kwargs={**turned, **other})
    with pytest.raises(ValueError, match="orientation and beam_width"):
        pipe.recognize(page, recognition_kwargs={**turned, "beam_width": 4})
    with pytest.raises(ValueError, match="orientation and lexicon_top"):
        pipe.recognize_padded(page, None, None, recognition_kwargs={**turned, "lexicon_top": 2})
    with pytest.raises(ValueError, match="orientation and char_boxes"):
        pipe.recognize_characters(page, recognition_kwargs=turned)
    with pytest.raises(ValueError, match="orientation and char_boxes"):
        pipe.recognize_raw(page, recognition_kwargs=turned, char_boxes=True)
    with pytest.raises(ValueError, match="orientation"):
        pipe.evaluate(page, [[]], recognition_kwargs={"orientation": "sideways"})
    with pytest.raises(NotImplementedError, match="orientation"):
        pipe.recognize([np.zeros((8, 8, 3), np.float32)], recognition_kwargs=turned)
    # zero images: the empty value, nothing called
    assert pipe.recognize([], recognition_kwargs=turned) == []
    raw = pipe.recognize_raw([], recognition_kwargs=turned)
    assert len(raw) == 3 and [a.shape for a in raw[2]] == [(0,), (0, 4, 2), (0, 2)]
    # the stage-wise route passes the arguments on only to a recogniser that takes them
    monkeypatch.setattr(k.tools, "resize_image", lambda image, max_scale, max_size: (np.zeros((16, 16, 3), np.uint8), 2))
    with pytest.raises(TypeError, match="orientation"):
        pipe.recognize(page, recognition_kwargs=turned)

    # Recognizer.recognize_from_boxes: refusals that come before its context is touched
    rec = object.__new__(k.recognition.Recognizer)
    rec.alphabet, rec.lexicon, rec._ctx = "abc", None, None  # pylint: disable=protected-access
    boxes = [np.zeros((1, 4, 2), np.float32)]
    with pytest.raises(ValueError, match="orientation and beam_width"):
        rec.recognize_from_boxes(page, boxes, orientation="flip", beam_width=4)
    with pytest.raises(ValueError, match="orientation"):
        rec.recognize_from_boxes(page, boxes, orientation="left")
    with pytest.raises(ValueError, match="tall_ratio"):
        rec.recognize_from_boxes(page, boxes, orientation="any", tall_ratio=-1)
    with pytest.raises(ValueError, match="return_orientation"):
        rec.recognize_from_boxes(page, boxes, return_orientation=True)
    with pytest.raises(NotImplementedError, match="orientation"):
        rec.recognize_from_boxes([np.zeros((8, 8, 3), np.float32)], boxes, orientation="any")
    assert rec.recognize_from_boxes(page, [[]], orientation="any", return_orientation=True) == [[]]


def test_stagewise_route_carries_the_oriented_boxes(monkeypatch):
    import keras_ocr_amd as k
    from keras_ocr_amd import layout, pipeline

    quad = np.array([[8, 2], [8, 12], [2, 12], [2, 2]], np.float32)

    class Det:
        def detect(self, images, **kw):
            return [np.array([[[2, 2], [8, 2], [8, 12], [2, 12]]], np.float32) for _ in images]

    class Rec:
        alphabet = "abc"

        def recognize_from_boxes(self, images, box_groups, return_scores=False, orientation=None, tall_ratio=1.5,
                                 return_orientation=False):
            assert (orientation, tall_ratio, return_orientation) == ("any", 1.25, True)
            return [[("cab", layout.Orientation(1, quad, (-1.0, -3.0)))] for _ in box_groups]

    monkeypatch.setattr(k.tools, "resize_image", lambda image, max_scale, max_size: (np.zeros((16, 16, 3), np.uint8), 2))
    pipe = pipeline.Pipeline(detector=Det(), recognizer=Rec())
    out = pipe.recognize([np.zeros((8, 8, 3), np.uint8)], recognition_kwargs={"orientation": "any", "tall_ratio": 1.25})
    assert [t for t, _ in out[0]] == ["cab"] and np.array_equal(out[0][0][1], quad / 2)
    boxes, labels, how = pipe.recognize_raw([np.zeros((8, 8, 3), np.uint8)], recognition_kwargs={"orientation": "any", "tall_ratio": 1.25})
    assert how[0].tolist() == [1] and np.array_equal(how[1][0], quad / 2) and how[2].tolist() == [[-1.0, -3.0]]
    assert np.array_equal(boxes[0][0], quad / 2) and labels[0, :3].tolist() == [2, 0, 1]
