"""GPU suite: the word boxes of a table put into rows, columns and spanning cells on the device (kocr_group_lines with
flags == KOCR_LINES_TABLE) against its float64 statement (tests/table_statement.py): the integers equal, the band boxes bit
for bit; and the same call with flags == 0 and flags == KOCR_LINES_BLOCKS untouched by it."""
import ctypes

import numpy as np
import pytest

from tests import blocks_cases as bc
from tests import blocks_statement as bs
from tests import lines_cases as lc
from tests import lines_statement as ls
from tests import table_cases as tc
from tests import table_statement as ts

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32
TABLE = 16


def _assert_same(got, want, what, names=("line_of", "order", "line_counts")):
    """(line_of, order, line_counts, line_boxes) of the device against the statement's"""
    for name, g, w in zip(names, got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        different = np.flatnonzero(g != w)
        assert different.size == 0, (what, name, different[:5], g[different[:5]], w[different[:5]])
    g, w = got[3], want[3]
    assert g.dtype == np.float32 and g.shape == w.shape, (what, g.shape, w.shape)
    different = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(-1, 8).any(axis=1))
    assert different.size == 0, (what, "boxes", different[:5], g[different[:5]], w[different[:5]])


def _raw(lib, ctx, quads, offsets, cap, flags=TABLE, boxes=True, rule=(1.0, 0.25, 0.5)):
    """kocr_group_lines itself: -> (rc, *true_lines, (line_of, order, line_counts, line_boxes) filled with -7 before, message)"""
    from keras_ocr_amd import _lib

    quads, offsets = np.ascontiguousarray(quads, F32), np.ascontiguousarray(offsets, I32)
    n, total = len(offsets) - 1, len(quads)
    out = (np.full(total, -7, I32), np.full(total, -7, I32), np.full(max(n, 1), -7, I32), np.full((max(cap, 1), 4, 2), -7, F32))
    count = ctypes.c_int64(-1)
    rc = lib.kocr_group_lines(ctx._h, n, _lib._ptr(quads), _lib._ptr(offsets), ls.cos_max_of(15.0), rule[2], rule[0], rule[1], _lib._ptr(out[0]),  # pylint: disable=protected-access
                              _lib._ptr(out[1]), _lib._ptr(out[2]), _lib._ptr(out[3]) if boxes else None, cap if boxes else 0, ctypes.byref(count), flags)
    return rc, count.value, out, lib.kocr_last_error(ctx._h)  # pylint: disable=protected-access


def _table(lib, ctx, pages, rule=None):
    """the raw call with room for every band, cut to the bands there are"""
    rule = {**ts.DEFAULTS, **(rule or {})}
    quads, offsets = tc.flatten(pages)
    rc, count, out, message = _raw(lib, ctx, quads, offsets, 2 * len(quads), rule=(rule["min_gap_x"], rule["min_gap_y"], rule["min_support"]))
    assert rc == 0, message
    assert count == int(out[2][:len(pages)].sum()) and (out[3][count:] == -7).all()
    return out[0], out[1], out[2][:len(pages)], out[3][:count]


@pytest.fixture(scope="module")
def lib():
    import keras_ocr_amd

    return keras_ocr_amd.load_library()


@pytest.fixture(scope="module")
def stated():
    """every case with the statement's answer, computed once: (name, quads, answer by hand or None, rule, statement)"""
    return [case + (ts.group_batch([case[1]], **case[3]),) for case in tc.every_case()]


def test_every_case_equals_the_statement(ctx, lib, stated):
    assert len(stated) > 35 and {len(s[1]) for s in stated} >= set(tc.SIZES)
    for name, quads, answer, rule, want in stated:
        got = _table(lib, ctx, [quads], rule)
        _assert_same(got, want, name)
        for key, shift in (("row", None), ("col0", 0), ("col1", 16)):  # and the answers known by hand
            if answer and key in answer:
                assert (got[0] if shift is None else (got[1] >> shift) & 0xFFFF).tolist() == answer[key], (name, key)
        if answer and "R" in answer and "S" in answer:
            assert got[2].tolist() == [answer["R"] + answer["S"] + 1], name


def test_context_group_table_unpacks_the_call(ctx, stated):
    for wanted in ("title row", "grid 257", "2048 in one row"):
        name, quads, _, rule, _ = next(s for s in stated if s[0] == wanted)
        want = ts.table_page(quads, **rule)
        row_of, first, last, rows, cols, row_boxes, col_boxes = ctx.group_table(quads, [0, len(quads)], **rule)
        assert all(a.dtype == np.int32 for a in (row_of, first, last, rows, cols)), name
        assert (row_of.tolist(), first.tolist(), last.tolist()) == (want["row"].tolist(), want["col0"].tolist(), want["col1"].tolist()), name
        assert (rows.tolist(), cols.tolist()) == ([want["R"]], [want["S"] + 1]), name
        assert row_boxes.dtype == col_boxes.dtype == np.float32
        assert row_boxes.tobytes() == want["row_boxes"].tobytes() and col_boxes.tobytes() == want["col_boxes"].tobytes(), name
        again = ctx.group_table(quads, [0, len(quads)], return_boxes=False, **rule)
        assert again[5] is None and again[6] is None and all(a.tobytes() == b.tobytes() for a, b in zip(again[:5], (row_of, first, last, rows, cols)))
    # a batch with empty pages: the bands go to the right page
    pages = tc.mixed_batch()
    got = ctx.group_table(*tc.flatten(pages))
    wants = [ts.table_page(p) for p in pages]
    assert got[3].tolist() == [w["R"] for w in wants] and got[4].tolist() == [w["S"] + 1 for w in wants]
    assert got[5].tobytes() == b"".join(w["row_boxes"].tobytes() for w in wants) and got[6].tobytes() == b"".join(w["col_boxes"].tobytes() for w in wants)
    empty = ctx.group_table(tc.page([]), [0, 0, 0])
    assert [a.shape for a in empty] == [(0,), (0,), (0,), (2,), (2,), (0, 4, 2), (0, 4, 2)] and empty[3].tolist() == empty[4].tolist() == [0, 0]
    for rule, name in (({"min_support": 1.5}, "min_support"), ({"min_gap_x": -1.0}, "min_gap_x"), ({"min_gap_y": float("inf")}, "min_gap_y")):
        with pytest.raises(ValueError, match=name):
            ctx.group_table(pages[1], [0, len(pages[1])], **rule)
    with pytest.raises(ValueError, match="2049"):
        ctx.group_table(np.zeros((2049, 4, 2), F32), [0, 2049])


def test_a_page_alone_and_inside_a_batch(ctx, lib, stated):
    pages = tc.mixed_batch()
    assert sum(len(p) == 0 for p in pages) >= 4
    want = ts.group_batch(pages)
    got = _table(lib, ctx, pages)
    _assert_same(got, want, "mixed batch")
    line_of, order, counts, boxes = got
    offsets = tc.flatten(pages)[1]
    first = np.concatenate([[0], np.cumsum(counts)])
    for k, page in enumerate(pages):
        alone = _table(lib, ctx, [page])
        inside = (line_of[offsets[k]:offsets[k + 1]], order[offsets[k]:offsets[k + 1]], counts[k:k + 1], boxes[first[k]:first[k + 1]])
        _assert_same(alone, inside, f"page {k} of {len(page)} quads alone")
    # a small page beside the largest one runs in a block sized for the largest
    small, large = tc.page([tc.box(0, 0, 40, 10), tc.box(60, 0, 40, 10), tc.box(0, 20, 40, 10)]), next(s for s in stated if s[0] == "grid 2048")
    assert len(small) == 3 and not large[3]
    both = _table(lib, ctx, [small, large[1], tc.page([]), small])
    want = ts.group_batch([small, large[1], tc.page([]), small])
    _assert_same(both, want, "3, 2048, 0, 3")
    # the small page by hand: two rows; the gap (40, 60) and the lower row's margin (40, 100) make one run up to the right
    # edge, which is no separator: one column
    assert both[2][0] == both[2][3] == 2 + 1 and both[2][2] == 0


def test_raw_abi(ctx, lib):
    from keras_ocr_amd import _lib

    assert _lib.KOCR_LINES_TABLE == TABLE
    pages = [tc.hand_made()[2][1], tc.page([]), tc.page([tc.box(0, 0, 30, 10)])]  # 5 + 3, 0 and 1 + 1 bands
    quads, offsets = tc.flatten(pages)
    want = ts.group_batch(pages)
    assert want[2].tolist() == [8, 0, 2]
    # capacity one too small: the code, the true number, and the integer outputs complete
    rc, count, out, message = _raw(lib, ctx, quads, offsets, 9)
    assert rc == _lib.KOCR_ECAPACITY and count == 10 and b"10 bands" in message
    _assert_same((out[0], out[1], out[2], want[3]), want, "capacity too small")
    assert (out[3] == -7).all()
    rc, count, out, _ = _raw(lib, ctx, quads, offsets, 10)
    assert rc == 0 and count == 10
    _assert_same((out[0], out[1], out[2], out[3][:10]), want, "raw call")
    rc, count, out, _ = _raw(lib, ctx, quads, offsets, 0, boxes=False)  # line_boxes == NULL
    assert rc == 0 and count == 10 and (out[3] == -7).all()
    _assert_same((out[0], out[1], out[2], want[3]), want, "raw call without boxes")
    # the mode stands alone: every other value that holds its bit is refused by name, with nothing written
    for flags in (17, 18, 20, 21, 48):
        rc, _, out, message = _raw(lib, ctx, quads, offsets, 32, flags=flags)
        assert rc == _lib.KOCR_EINVAL and b"flags" in message and all((o == -7).all() for o in out), (flags, message)
    # the rule's arguments under the existing checks and messages
    rc, _, out, message = _raw(lib, ctx, quads, offsets, 32, rule=(1.0, 0.25, 1.5))
    assert rc == _lib.KOCR_EINVAL and b"min_height_ratio" in message and b"outside [0, 1]" in message and all((o == -7).all() for o in out)
    rc, _, out, message = _raw(lib, ctx, quads, offsets, 32, rule=(-1.0, 0.25, 0.5))
    assert rc == _lib.KOCR_EINVAL and b"max_offset" in message and b"is not a finite number >= 0" in message and all((o == -7).all() for o in out)
    rc, _, _, message = _raw(lib, ctx, quads, offsets, 32, rule=(1.0, float("nan"), 0.5))
    assert rc == _lib.KOCR_EINVAL and b"max_gap" in message and b"is not a finite number >= 0" in message
    # the other refusals, with line mode's messages
    rc, _, _, message = _raw(lib, ctx, np.zeros((3 + 2049, 4, 2), F32), [0, 3, 3 + 2049], 8)
    assert rc == _lib.KOCR_EINVAL and b"page 1 holds 2049 words" in message
    rc, _, _, message = _raw(lib, ctx, quads, [0, 13, 12, 14], 32)
    assert rc == _lib.KOCR_EINVAL and b"offsets decreases at entry 2" in message
    bad = quads.copy()
    bad[13, 2, 1] = np.nan
    rc, _, _, message = _raw(lib, ctx, bad, offsets, 32)
    assert rc == _lib.KOCR_EINVAL and b"page 2, word 0: non-finite coordinate" in message
    # N = 0 and a batch of empty pages
    rc, count, _, _ = _raw(lib, ctx, tc.page([]), [0], 0)
    assert rc == 0 and count == 0
    rc, count, out, _ = _raw(lib, ctx, tc.page([]), [0, 0, 0, 0], 0)
    assert rc == 0 and count == 0 and out[2].tolist() == [0, 0, 0]
    # the call after all of that is unharmed
    _assert_same(_table(lib, ctx, pages), want, "after the refusals")


def _rows_of(ctx, call):
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = call()
        rows = ctx.profile_report()
    finally:
        ctx.profile_enable(False)
    return out, {name: row["launches"] for name, row in rows.items() if row["launches"]}


def test_first_call_on_a_fresh_context_with_guards_and_the_other_modes_untouched(ctx, lib, stated):
    """a context whose first call is a table call, its arenas guarded; then flags 0 and 1 on the same context: what they
    returned on a context that never saw the mode, with their own profiler rows only"""
    import keras_ocr_amd

    pages = [s[1] for s in stated if s[0] in ("grid 65", "grid 257", "grid 1025", "2048 single rows")] + [tc.page([])]
    assert len(pages) == 5
    want = ts.group_batch(pages)
    words = lc.small_pages()
    wq, wo = lc.flatten(words)
    blocks = [bc.heading_columns_footer()[0], bc.staircase()[0]]
    bq, bo = bc.flatten(blocks)
    lines_before, blocks_before = ctx.group_lines(wq, wo), ctx.group_blocks(bq, bo)  # the session's context, before any table call of this test
    _assert_same(lines_before, ls.group_batch(words)[:4], "line mode, the statement")
    _assert_same(blocks_before, bs.group_batch(blocks), "block mode, the statement")
    c = keras_ocr_amd.Context(0)
    try:
        c.set_arena_guards(True)
        got, rows = _rows_of(c, lambda: _table(lib, c, pages))
        assert rows == {"table_grid": 1, "lines_pack": 1}
        _assert_same(got, want, "first call")
        assert c.check_arena_guards()[0] == 0
        _, rows = _rows_of(c, lambda: c.group_table(*tc.flatten(pages), return_boxes=False))
        assert rows == {"table_grid": 1}
        lines_after, rows = _rows_of(c, lambda: c.group_lines(wq, wo))
        assert rows == {"lines_group": 1, "lines_pack": 1}
        blocks_after, rows = _rows_of(c, lambda: c.group_blocks(bq, bo))
        assert rows == {"blocks_cut": 1, "lines_pack": 1}
        assert all(a.tobytes() == b.tobytes() for a, b in zip(lines_before, lines_after))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(blocks_before, blocks_after))
        _assert_same(_table(lib, c, pages), want, "table mode again")
        assert c.check_arena_guards()[0] == 0
    finally:
        c.set_arena_guards(False)
        c.close()


class _Grid:
    """a detector that finds a title over three rows of three columns, the middle cell of the middle row in two words, in
    detector-input pixels (a duck-typed stage: the pipeline takes its stage-wise route).  Boxes 12 high: tx = 12, ty = 3 there"""

    def __init__(self):
        words, cells = [tc.box(4, 4, 236, 12)], [(0, 0)]
        for r in range(3):
            for c in range(3):
                x, y = 4 + 86 * c, 24 + 20 * r
                if (r, c) == (1, 1):
                    words += [tc.box(x + 34, y, 30, 12), tc.box(x, y, 30, 12)]  # the right word first
                    cells += [(r + 1, c), (r + 1, c)]
                else:
                    words.append(tc.box(x, y, 40 + 8 * ((r + c) % 3), 12))
                    cells.append((r + 1, c))
        self.boxes, self.cells = tc.page(words), cells

    def detect(self, images, **kwargs):
        return [self.boxes.copy() for _ in images]


def test_layout_and_pipeline_end_to_end(ctx, crnn_weights):
    import keras_ocr_amd
    from keras_ocr_amd import layout

    grid = _Grid()
    rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=ctx)
    pipe = keras_ocr_amd.pipeline.Pipeline(detector=grid, recognizer=rec)
    noise = np.random.default_rng(0).integers(0, 255, (64, 128, 3), dtype=np.uint8)
    words = pipe.recognize([noise, noise])
    assert len(words) == 2 and len(words[0]) == len(grid.cells) == 11
    assert all(np.array_equal(box, found / 2) for (_, box), found in zip(words[0], grid.boxes))  # input-image pixels, in the detector's order
    # layout.group_table on recognize()'s boxes: the statement's numbers
    tables = layout.group_table([[box for _, box in words[0]], []], ctx=ctx)
    want = ts.table_page(np.array([box for _, box in words[0]], F32))
    assert (want["R"], want["S"]) == (4, 2) and want["col1"].tolist()[0] == 2
    assert (tables[0].rows, tables[0].cols, tables[1].rows, tables[1].cols, tables[1].cells) == (4, 3, 0, 0, [])
    assert tables[0].row_boxes.tobytes() == want["row_boxes"].tobytes() and tables[0].col_boxes.tobytes() == want["col_boxes"].tobytes()
    assert [(c.row, c.col, c.colspan, c.words) for c in tables[0].cells] == \
        [(0, 0, 3, [0])] + [(r, c, 1, [j for j, at in enumerate(grid.cells) if at == (r, c)][::-1 if (r, c) == (2, 1) else 1])
                            for r in range(1, 4) for c in range(3)]
    # Pipeline.recognize_table: the matrix of texts, and recognize()'s own tuples
    got = pipe.recognize_table([noise, noise])
    assert len(got) == 2 and all(isinstance(t, layout.Table) for t in got)
    expected = [["", "", ""] for _ in range(4)]
    for (r, c), members in ((at, [j for j, a in enumerate(grid.cells) if a == at]) for at in sorted(set(grid.cells))):
        members.sort(key=lambda j: float(words[0][j][1][:, 0].min()))
        expected[r][c] = " ".join(words[0][j][0] for j in members)
    for table, page in zip(got, words):
        assert table.grid() == expected and (table.rows, table.cols) == (4, 3)
        flat = [w for cell in table.cells for w in cell.words]
        assert sorted((t, b.tobytes()) for t, b in flat) == sorted((t, b.tobytes()) for t, b in page) and len(flat) == 11
        assert all(b.dtype == np.float32 for _, b in flat)
        assert all(cell.text == " ".join(t for t, _ in cell.words) for cell in table.cells)
        assert table.cells[0].colspan == 3 and [len(cell.words) for cell in table.cells] == [1, 1, 1, 1, 1, 2, 1, 1, 1, 1]
        assert table.row_boxes.tobytes() == want["row_boxes"].tobytes()
    assert pipe.recognize_table([]) == []
    with pytest.raises(ValueError, match="beam_width"):
        pipe.recognize_table([noise], recognition_kwargs={"beam_width": 4})
    with pytest.raises(TypeError, match="min_gap_z"):
        pipe.recognize_table([noise], min_gap_z=1.0)
    # a rule reaches the device: with every row required the title's row hides both gutters
    assert [t.cols for t in pipe.recognize_table([noise], min_support=1.0)] == [1]
