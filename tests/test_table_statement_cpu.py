"""CPU suite: the table rule as stated (tests/table_statement.py) against answers known by hand and against an independent
brute-force reading of the same sentences; and the Python surface the feature adds, on a stub context."""
import inspect
import itertools
import types

import numpy as np
import pytest

from tests import table_cases as tc
from tests import table_statement as ts


def _check_page(name, quads, answer, rule):
    got = ts.table_page(quads, **rule)
    n = len(quads)
    for key, want in (answer or {}).items():
        have = got[key].tolist() if isinstance(got[key], np.ndarray) else got[key]
        assert have == want, (name, key, have, want)
    assert got["row"].shape == got["col0"].shape == got["col1"].shape == (n,), name
    assert got["S"] == (len(got["separators"]) if n else -1) and got["row_boxes"].shape == (got["R"], 4, 2) and got["col_boxes"].shape == (got["S"] + 1, 4, 2), name
    if n:
        assert sorted(set(got["row"].tolist())) == list(range(got["R"])), name  # every row has a member
        assert (got["col0"] >= 0).all() and (got["col1"] >= got["col0"]).all() and (got["col1"] <= got["S"]).all(), name
        assert got["S"] <= n - 1, name
    return got


@pytest.mark.parametrize("case", tc.hand_made() + tc.threshold_edges() + tc.support_cases(), ids=lambda c: c[0])
def test_hand_made_pages(case):
    _check_page(*case)


def test_the_larger_pages_hold_together():
    for name, quads, answer, rule in tc.random_cases():
        got = _check_page(name, quads, answer, rule)
        if name == "2048 single rows":
            assert got["R"] == 2048 and sum(len(w) for w in got["white"]) > 3000
    assert [len(c[1]) for c in tc.random_cases()[:len(tc.SIZES)]] == list(tc.SIZES)


def test_bands():
    """the bands of the 4 x 3 grid by hand: rows over the page's width, columns between the separators over its height"""
    _, quads, _, _ = tc.hand_made()[0]
    got = ts.table_page(quads)
    assert (got["H"], got["tx"], got["ty"]) == (10.0, 10.0, 2.5)
    assert got["row_boxes"].tolist() == [[[0, 20 * r], [250, 20 * r], [250, 20 * r + 10], [0, 20 * r + 10]] for r in range(4)]
    assert got["col_boxes"].tolist() == [[[a, 0], [b, 0], [b, 70], [a, 70]] for a, b in ((0, 40), (100, 145), (200, 250))]
    assert got["row_boxes"].dtype == got["col_boxes"].dtype == np.float32
    line_of, order, counts, boxes = ts.group_batch([quads, tc.page([]), quads[:1]])
    assert counts.tolist() == [7, 0, 2] and len(boxes) == 9 and len(line_of) == len(order) == 13
    assert order[:12].tolist() == [c | (c << 16) for _ in range(4) for c in range(3)]
    assert boxes[:4].tobytes() == got["row_boxes"].tobytes() and boxes[4:7].tobytes() == got["col_boxes"].tobytes()
    # a spanning cell in the packed form
    title = ts.group_batch([tc.hand_made()[2][1]])
    assert title[1][0] == (0 | (2 << 16)) and title[0][0] == 0
    assert ts.reading_order(quads, got["row"], got["col0"]) == list(range(12))


def test_support_changes_the_columns():
    quads = tc.support_page()
    assert [ts.table_page(quads, min_support=s)["S"] + 1 for s in (0.0, 0.5, 1.0)] == [4, 3, 2]


# -- an independent reading: coverage counted row by row at the float64 midpoint of every interval between two box edges --------

def _brute(quads, min_gap_x, min_gap_y, min_support):
    q = np.asarray(quads, np.float64).reshape(-1, 4, 2)
    n = len(q)
    x0, x1, y0, y1 = q[:, :, 0].min(1), q[:, :, 0].max(1), q[:, :, 1].min(1), q[:, :, 1].max(1)
    heights = [y1[i] - y0[i] for i in range(n) if y1[i] > y0[i]]
    H = sum(heights, 0.0) / len(heights) if heights else 0.0
    tx, ty = min_gap_x * H, min_gap_y * H
    # rows: a cut in front of quad i when everything that starts before it ends at least ty (and more than 0) above it
    row_starts = []
    for i in range(n):
        before = [j for j in range(n) if (y0[j], j) < (y0[i], i)]
        if before:
            g = y0[i] - max(y1[j] for j in before)
            if g > 0 and g >= ty:
                row_starts.append((y0[i], i))
    row = [sum(1 for s in row_starts if s <= (y0[i], i)) for i in range(n)]
    R = max(row) + 1
    K = max(1, int(np.ceil(min_support * R)))
    X0, X1 = x0.min(), x1.max()

    def white(r, m):
        """is m (never an edge of a white interval) inside a white interval of row r"""
        members = [i for i in range(n) if row[i] == r]
        if any(x0[i] <= m <= x1[i] for i in members):
            return False
        left, right = [x1[i] for i in members if x1[i] < m], [x0[i] for i in members if x0[i] > m]
        if left and right:
            return min(right) - max(left) > 0 and min(right) - max(left) >= tx
        return X0 < m < X1  # a margin: no width asked

    edges = sorted(set(x0.tolist()) | set(x1.tolist()))
    pieces = [(lo, hi, sum(white(r, (lo + hi) / 2) for r in range(R))) for lo, hi in zip(edges[:-1], edges[1:])]
    return {"row": row, "R": R, "K": K, "tx": tx, "ty": ty, "X1": X1, "pieces": pieces, "y0": y0, "y1": y1}


def test_against_a_brute_force_reading():
    pages = tc.small_integer_pages()
    assert len(pages) == 300 and max(len(p) for p, _ in pages) == 8
    seen_separators = seen_rows = seen_dropped = 0
    for k, (quads, rule) in enumerate(pages):
        got = ts.table_page(quads, **rule)
        b = _brute(quads, **rule)
        assert got["row"].tolist() == b["row"] and got["R"] == b["R"] and got["K"] == b["K"], k
        # every row gap is valid, and no valid one is left inside a row
        for r in range(1, b["R"]):
            above, below = [i for i in range(len(quads)) if b["row"][i] < r], [i for i in range(len(quads)) if b["row"][i] >= r]
            g = min(b["y0"][i] for i in below) - max(b["y1"][i] for i in above)
            assert g > 0 and g >= b["ty"], (k, r)
        for r in range(b["R"]):
            members = sorted((b["y0"][i], i) for i in range(len(quads)) if b["row"][i] == r)
            for at in range(1, len(members)):
                g = members[at][0] - max(b["y1"][i] for _, i in members[:at])
                assert not (g > 0 and g >= b["ty"]), (k, r)
        # the runs of the brute-force coverage, and of them the separators
        runs = []
        for lo, hi, c in b["pieces"]:
            if c >= b["K"]:
                if runs and runs[-1][1] == lo:
                    runs[-1] = (runs[-1][0], hi)
                else:
                    runs.append((lo, hi))
        wanted = [(a, e) for a, e in runs if e - a >= b["tx"] and e < b["X1"]]
        assert got["separators"] == wanted, (k, got["separators"], wanted)  # none missing, none too many
        seen_dropped += len(runs) - len(wanted)
        for a, e in got["separators"]:
            inside = [c for lo, hi, c in b["pieces"] if a <= lo and hi <= e]
            assert inside and min(inside) >= b["K"], k  # c >= K throughout
            beside = [c for lo, hi, c in b["pieces"] if hi == a or lo == e]
            assert all(c < b["K"] for c in beside), k  # maximal
            assert e - a >= b["tx"] and e < b["X1"], k
        seen_separators += len(wanted)
        seen_rows += b["R"] > 1
    assert seen_separators > 100 and seen_rows > 100 and seen_dropped > 50  # the pages do exercise the rule


def test_permutation_invariance():
    pages = [c[1] for c in tc.hand_made()] + [tc.support_page(), tc.grid_page(65, 7), tc.grid_page(257, 8)] + [p for p, _ in tc.small_integer_pages(30, 9)]
    for k, quads in enumerate(pages):
        want = ts.table_page(quads)
        perm = np.random.default_rng(k).permutation(len(quads))
        got = ts.table_page(quads[perm])
        for key in ("row", "col0", "col1"):
            assert got[key].tolist() == want[key][perm].tolist(), (k, key)
        assert (got["R"], got["S"], got["separators"]) == (want["R"], want["S"], want["separators"]), k
        assert got["row_boxes"].tobytes() == want["row_boxes"].tobytes() and got["col_boxes"].tobytes() == want["col_boxes"].tobytes(), k


def test_refusals_of_the_statement():
    quads = tc.page([tc.box(0, 0, 30, 10)])
    for rule in ({"min_gap_x": -1.0}, {"min_gap_y": float("nan")}, {"min_support": 1.5}, {"min_support": -0.1}, {"min_support": float("nan")}):
        with pytest.raises(ValueError, match=next(iter(rule))):
            ts.table_page(quads, **rule)
    with pytest.raises(ValueError, match="2049"):
        ts.table_page(np.zeros((2049, 4, 2), np.float32))
    empty = ts.table_page(tc.page([]))
    assert empty["R"] == 0 and empty["S"] == -1 and ts.group_batch([tc.page([])])[2].tolist() == [0]


# -- the Python surface on a stub context -------------------------------------------------------------------------------------

class _StubContext:
    """Context.group_table, answered by the statement"""

    def __init__(self):
        self.calls = []

    def group_table(self, quads, offsets, min_gap_x=1.0, min_gap_y=0.25, min_support=0.5, return_boxes=True):
        self.calls.append((len(quads), list(offsets), min_gap_x, min_gap_y, min_support))
        results = [ts.table_page(quads[a:b], min_gap_x=min_gap_x, min_gap_y=min_gap_y, min_support=min_support) for a, b in zip(offsets[:-1], offsets[1:])]
        cat = lambda key, dtype, tail: (np.concatenate([r[key] for r in results]) if results else np.zeros((0,) + tail, dtype)).astype(dtype)  # noqa: E731
        return (cat("row", np.int32, ()), cat("col0", np.int32, ()), cat("col1", np.int32, ()), np.array([r["R"] for r in results], np.int32),
                np.array([r["S"] + 1 for r in results], np.int32), cat("row_boxes", np.float32, (4, 2)), cat("col_boxes", np.float32, (4, 2)))


class _BlocksOnly:
    """a context from before the mode: it knows blocks and nothing of tables"""

    def group_blocks(self, quads, offsets, min_gap_x=1.0, min_gap_y=0.75, return_boxes=True):
        raise AssertionError("not asked for")


def test_layout_table_on_a_stub_context():
    from keras_ocr_amd import layout

    assert layout.Cell._fields == ("row", "col", "colspan", "words", "text") and layout.Cell(0, 1, 1, [2]).text is None
    assert layout.Table._fields == ("rows", "cols", "row_boxes", "col_boxes", "cells")
    title = tc.hand_made()[2]
    grid, answer = tc.shuffled(tc.hand_made()[0][1], tc.hand_made()[0][2], 3)
    stub = _StubContext()
    tables = layout.group_table([title[1], [], grid, np.array([])], ctx=stub)
    assert len(stub.calls) == 1 and stub.calls[0] == (25, [0, 13, 13, 25, 25], 1.0, 0.25, 0.5)
    assert [(t.rows, t.cols, len(t.cells)) for t in tables] == [(5, 3, 13), (0, 0, 0), (4, 3, 12), (0, 0, 0)]
    # the title: one cell over three columns, first in reading order
    assert tables[0].cells[0] == layout.Cell(0, 0, 3, [0]) and all(c.colspan == 1 for c in tables[0].cells[1:])
    assert [(c.row, c.col) for c in tables[0].cells[1:]] == [(r, c) for r in range(1, 5) for c in range(3)]
    assert tables[0].grid()[0] == ["0", "", ""] and tables[0].grid()[1] == ["1", "2", "3"]
    # the shuffled grid: the cells in reading order whatever the input order
    assert [(c.row, c.col) for c in tables[2].cells] == [(r, c) for r in range(4) for c in range(3)]
    assert all((answer["row"][c.words[0]], answer["col0"][c.words[0]]) == (c.row, c.col) and len(c.words) == 1 for c in tables[2].cells)
    want = ts.table_page(grid)
    assert tables[2].row_boxes.tobytes() == want["row_boxes"].tobytes() and tables[2].col_boxes.tobytes() == want["col_boxes"].tobytes()
    assert tables[1].grid() == [] and tables[1].row_boxes.shape == (0, 4, 2)
    # two words of one cell go left to right; the cell spans as far as its widest word
    page = tc.page([tc.box(130, 0, 100, 10), tc.box(100, 0, 20, 10), tc.box(0, 0, 40, 10), tc.box(0, 20, 40, 10), tc.box(100, 20, 40, 10),
                    tc.box(200, 20, 40, 10), tc.box(0, 40, 40, 10), tc.box(100, 40, 40, 10), tc.box(200, 40, 40, 10)])
    table = layout.group_table([page], ctx=stub)[0]
    assert (table.rows, table.cols) == (3, 3) and table.cells[:2] == [layout.Cell(0, 0, 1, [2]), layout.Cell(0, 1, 2, [1, 0])]
    # the rule reaches the context; unknown names do not
    layout.group_table([grid], ctx=stub, min_gap_x=2.0, min_gap_y=0.5, min_support=1.0)
    assert stub.calls[-1][2:] == (2.0, 0.5, 1.0)
    assert layout.group_table([], ctx=stub) == []
    with pytest.raises(TypeError, match="min_gab_x"):
        layout.group_table([], ctx=stub, min_gab_x=2)
    with pytest.raises(AttributeError, match="group_table"):
        layout.group_table([grid], ctx=_BlocksOnly())


def test_recognize_table_on_a_stub_context():
    import keras_ocr_amd as k

    title = tc.hand_made()[2][1]
    words = [(f"w{j}", q) for j, q in enumerate(title)]
    seen = []

    class Stub(k.pipeline.Pipeline):
        def recognize(self, images, detection_kwargs=None, recognition_kwargs=None):
            seen.append((detection_kwargs, recognition_kwargs))
            return [words, []]

    stub = _StubContext()
    pipe = Stub(detector=types.SimpleNamespace(_ctx=stub), recognizer=object())
    got = pipe.recognize_table(["a", "b"], {"d": 1}, {"r": 2}, min_support=0.75)
    assert seen == [({"d": 1}, {"r": 2})] and stub.calls[0][2:] == (1.0, 0.25, 0.75)
    assert len(got) == 2 and isinstance(got[0], k.layout.Table) and (got[1].rows, got[1].cols, got[1].cells) == (0, 0, [])
    assert got[0].grid() == [["w0", "", ""]] + [[f"w{1 + 3 * r + c}" for c in range(3)] for r in range(4)]
    assert got[0].cells[0].colspan == 3 and got[0].cells[0].words[0] is words[0] and got[0].cells[0].text == "w0"
    assert [w for cell in got[0].cells for w in cell.words] == words  # this page was given in reading order
    with pytest.raises(TypeError, match="min_gab_y"):
        pipe.recognize_table([], min_gab_y=1)


def test_surface_and_refusals():
    import keras_ocr_amd as k

    sig = inspect.signature(k.Context.group_table)
    assert list(sig.parameters)[1:] == ["quads", "offsets", "min_gap_x", "min_gap_y", "min_support", "return_boxes"]
    assert {n: p.default for n, p in sig.parameters.items() if n in ts.DEFAULTS} == ts.DEFAULTS and sig.parameters["return_boxes"].default is True
    assert list(inspect.signature(k.layout.group_table).parameters) == ["box_groups", "ctx", "rule"]
    assert list(inspect.signature(k.pipeline.Pipeline.recognize_table).parameters)[1:] == ["images", "detection_kwargs", "recognition_kwargs", "rule"]
    assert k._lib.KOCR_LINES_TABLE == 16 and k._lib.KOCR_LINES_BLOCKS == 1 and k._lib.KOCR_LINES_DESKEW == 4  # pylint: disable=protected-access
    # refused by name before the library is reached (a context without one)
    nobody = types.SimpleNamespace()
    quads = tc.page([tc.box(0, 0, 30, 10)])
    for rule, bad in itertools.product(("min_gap_x", "min_gap_y"), (-1.0, float("nan"), float("inf"), -float("inf"))):
        with pytest.raises(ValueError, match=rule):
            k.Context.group_table(nobody, quads, [0, 1], **{rule: bad})
    for bad in (1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="min_support"):
            k.Context.group_table(nobody, quads, [0, 1], min_support=bad)
    with pytest.raises(ValueError, match="offsets"):
        k.Context.group_table(nobody, quads, [0, 2])
    # recognize_table refuses what recognize_blocks refuses
    pipe = k.pipeline.Pipeline(detector=object(), recognizer=object())
    for key in ("beam_width", "lexicon_top", "pattern"):
        with pytest.raises(ValueError, match=key):
            pipe.recognize_table([], recognition_kwargs={key: 4})
        with pytest.raises(ValueError, match=key):
            pipe.recognize_blocks([], recognition_kwargs={key: 4})
