"""CPU suite: the float64 statement of the XY-cut (tests/blocks_statement.py) on layouts with answers written out by hand,
against an independent brute-force reading of the rule on small pages, under permutation of the input; and the surface
the feature adds, on a stub context."""
import inspect
import itertools
import types

import numpy as np
import pytest

from tests import blocks_cases as bc
from tests import blocks_statement as bs


def _check_page(name, quads, blocks, rule):
    got = bs.blocks_page(quads, **rule)
    n = len(quads)
    if blocks is not None:
        assert got["blocks"] == blocks, (name, got["blocks"])
    blocks = got["blocks"]
    assert sorted(got["order"].tolist()) == list(range(n)), name
    assert got["order"].tolist() == [j for b in blocks for j in b], name
    assert got["block_of"].tolist() == [next(k for k, b in enumerate(blocks) if j in b) for j in range(n)], name
    assert got["boxes"].shape == (len(blocks), 4, 2) and got["boxes"].dtype == np.float32, name
    return got


@pytest.mark.parametrize("case", bc.hand_made() + bc.threshold_edges(), ids=lambda c: c[0])
def test_hand_made_pages(case):
    _check_page(*case)


def test_widest_first_not_all_at_once():
    """the issue's page: cutting the widest horizontal gap first takes off footer and heading, and then the columns come
    apart; and of two equal widest gaps the topmost goes first, which the other choice would show in the order"""
    quads, blocks = bc.heading_columns_footer()
    got = _check_page("unshuffled", quads, blocks, {})
    assert got["blocks"] != bc.all_at_once_order()
    assert (got["H"], got["tx"], got["ty"]) == (24.0, 24.0, 18.0)
    assert [(axis, gaps) for axis, _, _, gaps in got["cuts"][:3]] == [("y", [46.0]), ("y", [40.0]), ("x", [40.0])]
    quads, first, other = bc.equal_widest()
    got = _check_page("equal widest", quads, first, {})
    assert got["blocks"] != other and got["cuts"][0][3] == [40.0] and got["cuts"][0][2] == [[0], [1, 2, 3, 4]]


def test_boxes_and_heights():
    cases = {c[0]: c for c in bc.hand_made()}
    got = _check_page(*cases["two columns"])
    assert np.array_equal(got["boxes"], bc.page([bc.box(0, 0, 200, 84), bc.box(240, 0, 200, 84)]))
    got = _check_page(*cases["zero height and width"])
    assert got["H"] == 24.0 and got["boxes"][0].tolist() == [[0, 0], [100, 0], [100, 60], [0, 60]] and got["boxes"][2].tolist() == [[250, 80]] * 4
    got = _check_page(*cases["only zero heights"])
    assert got["H"] == 0.0 and got["tx"] == 0.0 and got["ty"] == 0.0
    for case in bc.threshold_edges():
        got = bs.blocks_page(case[1], **case[3])
        assert 32.0 <= got["H"] < 32.00001, case[0]  # exactly 32 but where the second box's end was rounded
    quads, blocks = bc.tall_column()
    got = _check_page("column of 2048 blocks", quads, blocks, {})
    assert len(got["cuts"]) == 2047 and all(axis == "y" and len(parts[0]) == 1 for axis, _, parts, _ in got["cuts"])
    got = _check_page(*cases["staircase"])
    assert [axis for axis, _, _, _ in got["cuts"]] == ["x", "y"] * 19 + ["x"]


# ---- an independent reading of the rule, by brute force ------------------------------------------------------------------

def _valid_cuts(members, s, e, t):
    """{the quad a cut falls before: its gap} along one axis, every quad against every other, in Python floats"""
    found = {}
    for c in members:
        before = [j for j in members if (float(s[j]), j) < (float(s[c]), c)]
        if before:
            g = float(s[c]) - max(float(e[j]) for j in before)
            if g > 0 and g >= t:
                found[c] = g
    return found


def _check_by_brute_force(quads, rule, name):
    got = bs.blocks_page(quads, **rule)
    x0, x1, y0, y1 = bs.boxes_of(quads)
    tx, ty = got["tx"], got["ty"]
    for block in got["blocks"]:  # a block has no valid cut
        assert not _valid_cuts(block, x0, x1, tx) and not _valid_cuts(block, y0, y1, ty), (name, block)
    segments = [sorted(range(len(quads)))]
    for axis, segment, parts, gaps in got["cuts"]:
        assert segment in segments and sorted(j for p in parts for j in p) == segment and all(parts), (name, segment)
        along_x = _valid_cuts(segment, x0, x1, tx)
        if axis == "x":  # every valid gap was cut, and only those
            assert sorted(p[0] for p in parts[1:]) == sorted(along_x) and sorted(gaps) == sorted(along_x.values()), (name, segment)
            assert all(max(float(x0[j]) for j in a) <= min(float(x0[j]) for j in b) for a, b in zip(parts, parts[1:])), name
        else:  # no valid gap along x; the one cut is valid, the widest, and the topmost of the widest
            along_y = _valid_cuts(segment, y0, y1, ty)
            assert not along_x and len(parts) == 2 and along_y, (name, segment)
            widest = max(along_y.values())
            first = min((c for c, g in along_y.items() if g == widest), key=lambda c: (float(y0[c]), c))
            assert gaps == [widest] and parts[1][0] == first, (name, segment)
            assert set(parts[0]) == {j for j in segment if (float(y0[j]), j) < (float(y0[first]), first)}, name
        segments.remove(segment)
        segments += [sorted(p) for p in parts]
    assert sorted(segments) == sorted(sorted(b) for b in got["blocks"]), name


def test_small_pages_by_brute_force():
    checked = 0
    for name, quads, _, rule in bc.hand_made() + bc.threshold_edges():
        if len(quads) <= 7:
            _check_by_brute_force(quads, rule, name)
            checked += 1
    assert checked >= 15
    rng = np.random.default_rng(11)
    counts = set()
    for k in range(300):  # boxes on a coarse grid: equal starts, equal gaps, gaps of exactly t and touching boxes are common
        n = int(rng.integers(2, 8))
        xy, wh = rng.integers(0, 12, (n, 2)) * 16.0, rng.integers(0, 4, (n, 2)) * 16.0
        quads = bc.page([bc.box(x, y, w, h) for (x, y), (w, h) in zip(xy.tolist(), wh.tolist())])
        rule = {"min_gap_x": float(rng.choice([0.0, 0.5, 1.0])), "min_gap_y": float(rng.choice([0.0, 0.5, 0.75]))}
        _check_by_brute_force(quads, rule, f"grid page {k}")
        counts.add(len(bs.blocks_page(quads, **rule)["blocks"]))
    assert counts >= {1, 2, 3, 4, 5}


def test_a_page_does_not_depend_on_input_order():
    """the blocks are a property of the set of boxes: permuting the input permutes the indices, nothing else"""
    rng = np.random.default_rng(5)
    pages = [bc.heading_columns_footer()[0], bc.layout_page(rng, 300), bc.scatter_page(rng, 120)]
    for quads in pages:
        a = bs.blocks_page(quads)
        assert len(a["blocks"]) > 3
        for _ in range(3):
            perm = rng.permutation(len(quads))
            b = bs.blocks_page(quads[perm])
            assert [sorted(int(perm[j]) for j in block) for block in b["blocks"]] == [sorted(block) for block in a["blocks"]]
            assert np.array_equal(a["boxes"], b["boxes"])


def test_the_random_pages_are_what_they_are_meant_to_be():
    cases = bc.every_case()
    assert len({c[0] for c in cases}) == len(cases)
    sizes = {len(c[1]) for c in cases}
    assert set(bc.SIZES) | {300, 2048} <= sizes
    for name, quads, _, rule in bc.random_cases():
        got = _check_page(name, quads, None, rule)
        if len(quads) >= 63:
            assert 3 < len(got["blocks"]) < len(quads) and {axis for axis, _, _, _ in got["cuts"]} == {"x", "y"}, name
            assert max(len(b) for b in got["blocks"]) > 1, name
    batch = bc.mixed_batch()
    assert sum(len(p) == 0 for p in batch) >= 4 and len(batch[0]) == 0 and len(batch[-1]) == 0 and sum(len(p) > 0 for p in batch) >= 20


def test_refusals_of_the_statement():
    with pytest.raises(ValueError, match="2049"):
        bs.blocks_page(np.zeros((2049, 4, 2), np.float32))
    bad = bc.page([bc.box(0, 0, 30, 10)])
    bad[0, 2, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        bs.blocks_page(bad)
    for rule in ({"min_gap_x": -1.0}, {"min_gap_y": float("nan")}, {"min_gap_x": float("inf")}):
        with pytest.raises(ValueError, match=next(iter(rule))):
            bs.blocks_page(bc.page([bc.box(0, 0, 30, 10)]), **rule)


# ---- the surface ------------------------------------------------------------------------------------------------------------

class _StubContext:
    """Context.group_blocks, answered by the statement"""

    def __init__(self):
        self.calls = []

    def group_blocks(self, quads, offsets, min_gap_x=1.0, min_gap_y=0.75, return_boxes=True):
        self.calls.append((len(quads), list(offsets), min_gap_x, min_gap_y))
        pages = [quads[a:b] for a, b in zip(offsets[:-1], offsets[1:])]
        return bs.group_batch(pages, min_gap_x=min_gap_x, min_gap_y=min_gap_y)


def test_layout_blocks_on_a_stub_context():
    from keras_ocr_amd import layout

    assert layout.Block._fields == ("box", "lines")
    quads, blocks = bc.heading_columns_footer()
    two = bc.hand_made()[1]
    stub = _StubContext()
    pages = layout.group_blocks([quads, [], two[1], np.array([])], ctx=stub)
    assert len(stub.calls) == 1 and stub.calls[0] == (18, [0, 12, 12, 18, 18], 1.0, 0.75)
    assert [[b.lines for b in p] for p in pages] == [blocks, [], two[2], []]
    want = bs.blocks_page(quads)["boxes"]
    assert all(b.box.dtype == np.float32 and b.box.tobytes() == w.tobytes() for b, w in zip(pages[0], want))
    # the rule reaches the context: with a gutter of 40 and min_gap_x = 2 (48) the columns stay together
    pages = layout.group_blocks([quads], ctx=stub, min_gap_x=2.0, min_gap_y=0.5)
    assert stub.calls[-1][2:] == (2.0, 0.5) and [b.lines for b in pages[0]] == [[0], [1, 6, 2, 7, 3, 8], [4, 9, 5, 10], [11]]
    assert layout.group_blocks([], ctx=stub) == []
    with pytest.raises(TypeError, match="min_gab_x"):
        layout.group_blocks([], ctx=stub, min_gab_x=2)


def test_recognize_blocks_on_a_stub_context():
    import keras_ocr_amd as k

    quads, blocks = bc.heading_columns_footer()
    lines = [(f"line{j}", q, [(f"line{j}", q)]) for j, q in enumerate(quads)]
    seen = []

    class Stub(k.pipeline.Pipeline):
        def recognize_lines(self, images, detection_kwargs=None, recognition_kwargs=None, **rule):
            seen.append((detection_kwargs, recognition_kwargs, rule))
            return [lines, []]

    stub = _StubContext()
    pipe = Stub(detector=types.SimpleNamespace(_ctx=stub), recognizer=object())
    got = pipe.recognize_blocks(["a", "b"], {"d": 1}, {"r": 2}, min_gap_y=0.5, max_gap=3.0)
    assert seen == [({"d": 1}, {"r": 2}, {"max_gap": 3.0})] and stub.calls[0][2:] == (1.0, 0.5)
    assert len(got) == 2 and got[1] == []
    want = bs.blocks_page(quads, min_gap_y=0.5)
    assert want["blocks"] == blocks
    for (text, box, members), indices, want_box in zip(got[0], blocks, want["boxes"]):
        assert text == "\n".join(f"line{j}" for j in indices) and box.tobytes() == want_box.tobytes()
        assert all(m is lines[j] for m, j in zip(members, indices)) and len(members) == len(indices)
    # the text of the page: column 1 in full before column 2
    assert "\n".join(t for t, _, _ in got[0]).split("\n") == [f"line{j}" for j in range(12)]


def test_surface_and_refusals():
    import keras_ocr_amd as k

    sig = inspect.signature(k.Context.group_blocks)
    assert list(sig.parameters)[1:] == ["quads", "offsets", "min_gap_x", "min_gap_y", "return_boxes"]
    assert {n: p.default for n, p in sig.parameters.items() if n in bs.DEFAULTS} == bs.DEFAULTS and sig.parameters["return_boxes"].default is True
    sig = inspect.signature(k.layout.group_blocks)
    assert list(sig.parameters) == ["box_groups", "ctx", "min_gap_x", "min_gap_y"]
    assert {n: p.default for n, p in sig.parameters.items() if n in bs.DEFAULTS} == bs.DEFAULTS
    sig = inspect.signature(k.pipeline.Pipeline.recognize_blocks)
    assert list(sig.parameters)[1:] == ["images", "detection_kwargs", "recognition_kwargs", "min_gap_x", "min_gap_y", "line_rule"]
    assert {n: p.default for n, p in sig.parameters.items() if n in bs.DEFAULTS} == bs.DEFAULTS
    # what is there already keeps its signature
    assert list(inspect.signature(k.Context.group_lines).parameters)[1:] == ["quads", "offsets", "max_angle", "min_height_ratio", "max_offset", "max_gap",
                                                                             "return_boxes"]
    assert list(inspect.signature(k.pipeline.Pipeline.recognize_lines).parameters)[1:] == ["images", "detection_kwargs", "recognition_kwargs", "rule"]
    assert k._lib.KOCR_LINES_BLOCKS == 1  # pylint: disable=protected-access
    # refused by name before the library is reached (a context without one)
    nobody = types.SimpleNamespace()
    quads = bc.page([bc.box(0, 0, 30, 10)])
    for rule, bad in itertools.product(("min_gap_x", "min_gap_y"), (-1.0, float("nan"), float("inf"), -float("inf"))):
        with pytest.raises(ValueError, match=rule):
            k.Context.group_blocks(nobody, quads, [0, 1], **{rule: bad})
    with pytest.raises(ValueError, match="offsets"):
        k.Context.group_blocks(nobody, quads, [0, 2])
    # recognize_blocks refuses what recognize_lines refuses
    pipe = k.pipeline.Pipeline(detector=object(), recognizer=object())
    for key in ("beam_width", "lexicon_top"):
        with pytest.raises(ValueError, match=key):
            pipe.recognize_blocks([], recognition_kwargs={key: 4})
    pipe = k.pipeline.Pipeline(detector=object(), recognizer=types.SimpleNamespace(alphabet="ab"))
    with pytest.raises(TypeError, match="max_gab"):  # the line rule's own refusal, before any context is needed
        pipe.recognize_blocks([], max_gab=2)
    with pytest.raises(TypeError, match="min_gab_y"):
        pipe.recognize_blocks([], min_gab_y=2)
