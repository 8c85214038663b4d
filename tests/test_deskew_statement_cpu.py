"""No GPU: the statement of the deskewed XY-cut (tests/deskew_statement.py) against plain block mode on unrotated pages,
against the blocks known by hand on rotated ones, its axis under outliers, ties and permutations, and the Python surface
on stub contexts."""
import inspect
import types

import numpy as np
import pytest

from tests import blocks_cases as bc
from tests import blocks_statement as bs
from tests import deskew_cases as dc
from tests import deskew_statement as ds


def _turn(a, b):
    """a - b in degrees, in [-180, 180)"""
    return (a - b + 180.0) % 360.0 - 180.0


def test_unrotated_pages_equal_plain_block_mode():
    """every quad of blocks_cases is built by box(): all directions are exactly (1, 0), every product with 0 or 1 is exact"""
    cases = bc.every_case()
    assert len(cases) > 35
    for name, quads, _, rule in cases:
        want, got = bs.blocks_page(quads, **rule), ds.blocks_page(quads, **rule)
        assert got["axis"] == (1.0, 0.0), name
        assert np.array_equal(got["block_of"], want["block_of"]) and np.array_equal(got["order"], want["order"]), name
        assert got["blocks"] == want["blocks"], name
        assert got["boxes"].dtype == np.float32 and np.array_equal(got["boxes"], want["boxes"]), name  # as numbers: a zero may be -0
        assert np.array_equal(got["frame"], np.asarray(quads, np.float32)), name


def test_rotated_pages_give_the_blocks_known_by_hand():
    from keras_ocr_amd import layout

    cases = dc.rotated_hand_cases()
    assert len(cases) == 18
    for name, quads, blocks, angle in cases:
        assert np.abs(quads).max() < 2048
        got = ds.blocks_page(quads)
        assert got["blocks"] == blocks, name
        assert got["order"].tolist() == [j for b in blocks for j in b], name
        if abs(angle) >= 7:  # the case is about something: the axis-aligned cut gets it wrong
            assert bs.blocks_page(quads)["blocks"] != blocks, name
        # the angle read back off every block box.  A coordinate below 2048 carries at most 6e-5 of float32 rounding per
        # corner and the shortest quad is 200 wide: the direction is off by under 2e-4 degrees
        assert abs(_turn(np.degrees(np.arctan2(got["axis"][1], got["axis"][0])), angle)) < 1e-3, name
        for box in got["boxes"]:
            found = layout.box_angle(box)
            assert -180.0 < found <= 180.0 and abs(_turn(found, angle)) < 1e-3, (name, found)


def test_box_angle():
    from keras_ocr_amd import layout

    assert layout.box_angle(bc.box(3, 4, 10, 5)) == 0.0
    assert layout.box_angle(bc.box(3, 4, 0, 5)) == 0.0  # no width
    assert layout.box_angle(np.array(bc.box(0, 0, 10, 5), np.float32)[[1, 2, 3, 0]]) == 90.0
    assert layout.box_angle(np.array(bc.box(0, 0, 10, 5), np.float32)[[3, 0, 1, 2]]) == -90.0
    assert layout.box_angle(np.array(bc.box(0, 0, 10, 5), np.float32)[[2, 3, 0, 1]]) == 180.0
    assert layout.box_angle([[0, 0], [-10, -0.0], [-10, -5], [0, -5]]) == 180.0  # atan2(-0, -10) is -180
    assert abs(layout.box_angle([[0, 0], [1, 1], [0, 2], [-1, 1]]) - 45.0) < 1e-12


def test_a_minority_of_turned_squares_does_not_pull_the_axis():
    for angle in (0.0, 12.0, -20.0, 180.0):
        quads, n_main = dc.page_with_outliers(angle)
        found = ds.page_axis(quads)
        assert found["w"][n_main:].sum() <= 0.25 * found["w"].sum()
        out_dir = found["u"][n_main:]
        main_dir = np.array([np.cos(np.radians(angle)), np.sin(np.radians(angle))])
        assert np.abs(out_dir @ main_dir).max() < 1e-6  # the outliers really stand across the text
        assert found["medoid"] < n_main, angle
        alone = ds.page_axis(quads[:n_main])
        # with or without them the axis is the direction of an ordinary quad: within the rounding of the rotation itself
        for axis in (found["axis"], alone["axis"]):
            assert abs(_turn(np.degrees(np.arctan2(axis[1], axis[0])), angle)) < 1e-3, angle
        if angle == 0.0:  # equal directions: the same axis exactly, and plain block mode's blocks
            assert found["axis"] == alone["axis"] == (1.0, 0.0)
            want, got = bs.blocks_page(quads), ds.blocks_page(quads)
            assert got["blocks"] == want["blocks"] and np.array_equal(got["boxes"], want["boxes"])
    # a mean would be pulled: the summed direction of this page is measurably off the text's
    quads, n_main = dc.page_with_outliers(0.0)
    u, w = ds.directions(quads)
    mean = (u * w[:, None]).sum(axis=0)
    assert abs(np.degrees(np.arctan2(mean[1], mean[0]))) > 1.0


def test_equal_directions_take_the_first_quad_with_one():
    slanted = np.array([[0, 0], [40, 30], [34, 38], [-6, 8]], np.float32)  # direction (0.8, 0.6): exact in float32 and float64
    quads = np.stack([np.array(bc.box(5, 5, 0, 10), np.float32)] + [slanted + np.float32(64 * k) for k in range(5)])
    found = ds.page_axis(quads)
    assert found["w"][0] == 0 and (found["u"][1:] == found["u"][1]).all()
    assert found["medoid"] == 1 and found["best"] == found["second"] == 0.0
    assert found["axis"] == (float(found["u"][1, 0]), float(found["u"][1, 1]))
    # two directions of equal weight: both candidates' costs are equal, the smaller index wins
    pair = np.stack([slanted, np.array(bc.box(0, 100, 50, 10), np.float32)])
    found = ds.page_axis(pair)
    assert found["best"] == found["second"] > 0 and found["medoid"] == 0


def test_a_page_without_directions_has_the_axis_1_0():
    quads = dc.zero_width_page()
    found = ds.page_axis(quads)
    assert found["axis"] == (1.0, 0.0) and found["medoid"] is None and found["best"] is None and (found["w"] == 0).all()
    want, got = bs.blocks_page(quads), ds.blocks_page(quads)
    assert got["blocks"] == want["blocks"] and np.array_equal(got["boxes"], want["boxes"])
    empty = ds.blocks_page(bc.page([]))
    assert empty["axis"] == (1.0, 0.0) and empty["blocks"] == [] and empty["boxes"].shape == (0, 4, 2)
    one = ds.blocks_page(dc.rotated(bc.page([bc.box(10, 20, 100, 24)]), 30.0))
    assert one["medoid"] == 0 and one["second"] is None and one["blocks"] == [[0]]


def test_blocks_do_not_depend_on_the_input_order():
    """on pages whose best candidate is clearly the best.  Another input order adds a candidate's terms in another order:
    the sum of n <= 2048 non-negative terms moves by at most n 2^-53 of itself, 2.3e-13; a page is used when its two best
    costs are 1e-9 of the larger apart, far above that"""
    rng = np.random.default_rng(41)
    used = 0
    for n, angle in ((40, 5.0), (65, -12.0), (130, 31.0), (300, 170.0), (64, 88.0)):
        quads = dc.rotated(bc.layout_page(rng, n), angle)
        first = ds.blocks_page(quads)
        if not first["second"] - first["best"] > 1e-9 * first["second"]:
            continue
        used += 1
        perm = rng.permutation(n)  # new index k holds old quad perm[k]
        second = ds.blocks_page(quads[perm])
        assert perm[second["medoid"]] == first["medoid"] and second["axis"] == first["axis"]
        assert [[int(perm[j]) for j in b] for b in second["blocks"]] == first["blocks"], (n, angle)
        assert np.array_equal(second["boxes"], first["boxes"])
    assert used >= 3


def test_refusals_of_the_statement():
    with pytest.raises(ValueError, match="2049"):
        ds.blocks_page(np.zeros((2049, 4, 2), np.float32))
    bad = bc.page([bc.box(0, 0, 30, 10)])
    bad[0, 2, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ds.blocks_page(bad)
    with pytest.raises(ValueError, match="min_gap_x"):
        ds.blocks_page(bc.page([bc.box(0, 0, 30, 10)]), min_gap_x=-1.0)


# ---- the surface ------------------------------------------------------------------------------------------------------------

class _PlainContext:
    """a context as it was before the switch: group_blocks without any new keyword, answered by the statement"""

    def __init__(self):
        self.calls = []

    def group_blocks(self, quads, offsets, min_gap_x=1.0, min_gap_y=0.75, return_boxes=True):
        self.calls.append(("plain", len(quads), list(offsets), min_gap_x, min_gap_y))
        return bs.group_batch([quads[a:b] for a, b in zip(offsets[:-1], offsets[1:])], min_gap_x=min_gap_x, min_gap_y=min_gap_y)


class _DeskewContext(_PlainContext):
    def group_blocks_deskewed(self, quads, offsets, min_gap_x=1.0, min_gap_y=0.75, return_boxes=True):
        self.calls.append(("deskewed", len(quads), list(offsets), min_gap_x, min_gap_y))
        return ds.group_batch([quads[a:b] for a, b in zip(offsets[:-1], offsets[1:])], min_gap_x=min_gap_x, min_gap_y=min_gap_y)


def test_constants_and_signatures():
    import keras_ocr_amd as k

    assert k._lib.KOCR_LINES_DESKEW == 4 and k._lib.KOCR_LINES_BLOCKS == 1  # pylint: disable=protected-access
    plain = inspect.signature(k.Context.group_blocks)
    assert list(inspect.signature(k.Context.group_blocks_deskewed).parameters) == list(plain.parameters)
    assert [p.default for p in inspect.signature(k.Context.group_blocks_deskewed).parameters.values()] == [p.default for p in plain.parameters.values()]
    plain = inspect.signature(k.layout.group_blocks)
    assert list(inspect.signature(k.layout.group_blocks_deskewed).parameters) == list(plain.parameters)
    assert [p.default for p in inspect.signature(k.layout.group_blocks_deskewed).parameters.values()] == [p.default for p in plain.parameters.values()]
    # refused by name before the library is reached (a context without one)
    nobody = types.SimpleNamespace()
    quads = bc.page([bc.box(0, 0, 30, 10)])
    with pytest.raises(ValueError, match="min_gap_y"):
        k.Context.group_blocks_deskewed(nobody, quads, [0, 1], min_gap_y=float("nan"))
    with pytest.raises(ValueError, match="offsets"):
        k.Context.group_blocks_deskewed(nobody, quads, [0, 2])


def test_layout_on_stub_contexts():
    from keras_ocr_amd import layout

    flat, blocks = bc.heading_columns_footer()
    quads = dc.rotated(flat, 10.0)
    # a context that knows nothing of the switch still serves group_blocks
    old = _PlainContext()
    assert [b.lines for b in layout.group_blocks([flat], ctx=old)[0]] == blocks and old.calls[0][0] == "plain"
    stub = _DeskewContext()
    pages = layout.group_blocks_deskewed([quads, [], flat], ctx=stub, min_gap_y=0.5)
    assert stub.calls == [("deskewed", 24, [0, 12, 12, 24], 1.0, 0.5)]
    assert [[b.lines for b in p] for p in pages] == [blocks, [], blocks]
    want = ds.blocks_page(quads, min_gap_y=0.5)["boxes"]
    assert all(isinstance(b, layout.Block) and b.box.dtype == np.float32 and b.box.tobytes() == w.tobytes() for b, w in zip(pages[0], want))
    assert all(abs(layout.box_angle(b.box) - 10.0) < 1e-3 for b in pages[0]) and all(layout.box_angle(b.box) == 0.0 for b in pages[2])
    assert [b.lines for b in layout.group_blocks([quads], ctx=stub)[0]] != blocks  # the plain cut on the rotated page
    assert layout.group_blocks_deskewed([], ctx=stub) == []
    with pytest.raises(TypeError, match="min_gab_x"):
        layout.group_blocks_deskewed([], ctx=stub, min_gab_x=2)


def test_recognize_blocks_deskew_on_a_stub_context():
    import keras_ocr_amd as k

    flat, blocks = bc.heading_columns_footer()
    quads = dc.rotated(flat, 10.0)
    lines = [(f"line{j}", q, [(f"line{j}", q)]) for j, q in enumerate(quads)]
    seen = []

    class Stub(k.pipeline.Pipeline):
        def recognize_lines(self, images, detection_kwargs=None, recognition_kwargs=None, **rule):
            seen.append((detection_kwargs, recognition_kwargs, rule))
            return [lines, []]

    stub = _DeskewContext()
    pipe = Stub(detector=types.SimpleNamespace(_ctx=stub), recognizer=object())
    got = pipe.recognize_blocks(["a", "b"], {"d": 1}, {"r": 2}, min_gap_y=0.5, max_gap=3.0, deskew=True)
    assert seen == [({"d": 1}, {"r": 2}, {"max_gap": 3.0})]  # the switch does not reach the line rule
    assert stub.calls == [("deskewed", 12, [0, 12, 12], 1.0, 0.5)]
    assert len(got) == 2 and got[1] == []
    want = ds.blocks_page(quads, min_gap_y=0.5)
    assert want["blocks"] == blocks
    for (text, box, members), indices, want_box in zip(got[0], blocks, want["boxes"]):
        assert text == "\n".join(f"line{j}" for j in indices) and box.tobytes() == want_box.tobytes()
        assert all(m is lines[j] for m, j in zip(members, indices)) and len(members) == len(indices)
        assert abs(k.layout.box_angle(box) - 10.0) < 1e-3
    assert "\n".join(t for t, _, _ in got[0]).split("\n") == [f"line{j}" for j in range(12)]  # column 1 in full before column 2
    # without the switch, and with it off, the plain cut is called
    for kwargs in ({}, {"deskew": False}):
        stub.calls.clear()
        plain = pipe.recognize_blocks(["a", "b"], **kwargs)
        assert [c[0] for c in stub.calls] == ["plain"] and seen[-1][2] == {}
        assert [[m[0] for m in members] for _, _, members in plain[0]] != [[f"line{j}" for j in b] for b in blocks]
    with pytest.raises(TypeError, match="deskew"):
        pipe.recognize_blocks([], deskew="yes")
