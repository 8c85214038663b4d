"""GPU suite: the XY-cut in the page's own frame on the device (kocr_group_lines with flags == KOCR_LINES_BLOCKS |
KOCR_LINES_DESKEW) against its float64 statement (tests/deskew_statement.py): the integers equal, the block boxes bit for
bit; and the same call with flags == 0 and flags == KOCR_LINES_BLOCKS untouched by it."""
import ctypes

import numpy as np
import pytest

from tests import blocks_cases as bc
from tests import blocks_statement as bs
from tests import deskew_cases as dc
from tests import deskew_statement as ds
from tests import lines_cases as lc
from tests import lines_statement as ls

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32


def _assert_same(got, want, what):
    """(block_of, order, block_counts, block_boxes) of the device against the statement's"""
    for name, g, w in zip(("block_of", "order", "block_counts"), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        different = np.flatnonzero(g != w)
        assert different.size == 0, (what, name, different[:5], g[different[:5]], w[different[:5]])
    g, w = got[3], want[3]
    assert g.dtype == np.float32 and g.shape == w.shape, (what, g.shape, w.shape)
    different = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(-1, 8).any(axis=1))
    assert different.size == 0, (what, "block_boxes", different[:5], g[different[:5]], w[different[:5]])


@pytest.fixture(scope="module")
def stated():
    """every page with the statement's answer, computed once: (name, quads, rule, answer)"""
    return [case + (ds.group_batch([case[1]], **case[2]),) for case in dc.gpu_cases()]


def test_every_page_equals_the_statement(ctx, stated):
    assert sorted(len(s[1]) for s in stated)[:3] == [0, 1, 2] and {63, 64, 65, 257, 1025, 2048} <= {len(s[1]) for s in stated}
    for name, quads, rule, want in stated:
        got = ctx.group_blocks_deskewed(quads, [0, len(quads)], **rule)
        _assert_same(got, want, name)
    # the blocks known by hand, rotated
    by_name = {s[0]: s for s in stated}
    for name, quads, blocks, _ in dc.rotated_hand_cases():
        want = by_name[name][3]
        assert want[2].tolist() == [len(blocks)] and want[1].tolist() == [j for b in blocks for j in b], name
    # without the boxes: the same integers
    name, quads, rule, want = by_name["outliers at 12"]
    block_of, order, counts, boxes = ctx.group_blocks_deskewed(quads, [0, len(quads)], return_boxes=False, **rule)
    assert boxes is None
    _assert_same((block_of, order, counts, want[3]), want, "without boxes")
    # a page that is not rotated: plain block mode's results as numbers (a zero may be -0)
    for name, quads, _, rule in [c for c in bc.hand_made() + bc.random_cases() if len(c[1]) <= 300]:
        plain, got = ctx.group_blocks(quads, [0, len(quads)], **rule), ctx.group_blocks_deskewed(quads, [0, len(quads)], **rule)
        assert all(np.array_equal(g, p) for g, p in zip(got, plain)), name


def test_a_page_alone_and_inside_a_batch(ctx, stated):
    chosen = [s for s in stated if not s[2]]  # one rule per call
    pages, at = dc.with_empty_pages([s[1] for s in chosen])
    assert sum(len(p) == 0 for p in pages) >= 4 and max(len(p) for p in pages) == 2048
    quads, offsets = bc.flatten(pages)
    block_of, order, counts, boxes = ctx.group_blocks_deskewed(quads, offsets)
    assert counts.shape == (len(pages),) and counts.sum() == len(boxes)
    first = np.concatenate([[0], np.cumsum(counts)])
    for k, page in enumerate(pages):
        inside = (block_of[offsets[k]:offsets[k + 1]], order[offsets[k]:offsets[k + 1]], counts[k:k + 1], boxes[first[k]:first[k + 1]])
        if k in at:  # a small page beside the largest one runs in a block sized for the largest
            name, _, _, want = chosen[at.index(k)]
            _assert_same(inside, want, f"{name} inside the batch")
        else:
            assert len(page) == 0 and counts[k] == 0
        _assert_same(ctx.group_blocks_deskewed(page, [0, len(page)]), inside, f"page {k} of {len(page)} quads alone")


def _raw(lib, ctx, n, quads, offsets, cap, flags, boxes=True, gaps=(1.0, 0.75)):
    from keras_ocr_amd import _lib

    total = len(quads)
    out = (np.full(total, -7, I32), np.full(total, -7, I32), np.full(max(n, 1), -7, I32), np.full((max(cap, 1), 4, 2), -7, F32))
    count = ctypes.c_int64(-1)
    rc = lib.kocr_group_lines(ctx._h, n, _lib._ptr(quads), _lib._ptr(offsets), ls.cos_max_of(15.0), 0.5, gaps[0], gaps[1], _lib._ptr(out[0]),  # pylint: disable=protected-access
                              _lib._ptr(out[1]), _lib._ptr(out[2]), _lib._ptr(out[3]) if boxes else None, cap if boxes else 0, ctypes.byref(count), flags)
    return rc, count.value, out, lib.kocr_last_error(ctx._h)  # pylint: disable=protected-access


def test_raw_abi(ctx):
    import keras_ocr_amd
    from keras_ocr_amd import _lib

    lib = keras_ocr_amd.load_library()
    deskew = _lib.KOCR_LINES_BLOCKS | _lib.KOCR_LINES_DESKEW
    assert deskew == 5
    pages = [dc.rotated(bc.hand_made()[1][1], 25.0), bc.page([]), dc.rotated(bc.page([bc.box(0, 0, 30, 10)]), -50.0)]  # 2 + 0 + 1 blocks
    quads, offsets = bc.flatten(pages)
    want = ds.group_batch(pages)
    assert want[2].tolist() == [2, 0, 1]
    # flags that stay refused, by name, with nothing written
    for flags in (4, 6, 7, 8):
        rc, _, out, message = _raw(lib, ctx, 3, quads, offsets, 8, flags)
        assert rc == _lib.KOCR_EINVAL and b"flags" in message and all((o == -7).all() for o in out), (flags, message)
        if flags == 4:
            assert b"KOCR_LINES_DESKEW needs KOCR_LINES_BLOCKS" in message
    # capacity one too small: the code, the true number, and the integer outputs complete
    rc, count, out, message = _raw(lib, ctx, 3, quads, offsets, 2, deskew)
    assert rc == _lib.KOCR_ECAPACITY and count == 3 and b"3 blocks" in message
    _assert_same((out[0], out[1], out[2], want[3]), want, "capacity too small")
    assert (out[3] == -7).all()
    rc, count, out, _ = _raw(lib, ctx, 3, quads, offsets, 3, deskew)
    assert rc == 0 and count == 3
    _assert_same((out[0], out[1], out[2], out[3][:3]), want, "raw call")
    rc, count, out, _ = _raw(lib, ctx, 3, quads, offsets, 0, deskew, boxes=False)  # line_boxes == NULL
    assert rc == 0 and count == 3 and (out[3] == -7).all()
    _assert_same((out[0], out[1], out[2], want[3]), want, "raw call without boxes")
    # block mode's refusals, with its messages
    rc, _, _, message = _raw(lib, ctx, 3, quads, offsets, 8, deskew, gaps=(-1.0, 0.75))
    assert rc == _lib.KOCR_EINVAL and b"max_offset" in message
    bad = quads.copy()
    bad[6, 2, 1] = np.nan
    rc, _, _, message = _raw(lib, ctx, 3, bad, offsets, 8, deskew)
    assert rc == _lib.KOCR_EINVAL and b"page 2, word 0: non-finite coordinate" in message
    with pytest.raises(ValueError, match="page 2, word 0"):
        ctx.group_blocks_deskewed(bad, offsets)
    with pytest.raises(ValueError, match="2049"):
        ctx.group_blocks_deskewed(np.zeros((2049, 4, 2), F32), [0, 2049])
    # N = 0 and a batch of empty pages
    rc, count, _, _ = _raw(lib, ctx, 0, bc.page([]), np.array([0], I32), 0, deskew)
    assert rc == 0 and count == 0
    got = ctx.group_blocks_deskewed(bc.page([]), [0, 0, 0])
    assert [a.shape for a in got] == [(0,), (0,), (2,), (0, 4, 2)] and got[2].tolist() == [0, 0]
    # the call after all of that is unharmed
    _assert_same(ctx.group_blocks_deskewed(quads, offsets), want, "after the refusals")


def _rows_of(ctx, call):
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = call()
        rows = ctx.profile_report()
    finally:
        ctx.profile_enable(False)
    return out, {name: row["launches"] for name, row in rows.items() if row["launches"]}


def test_the_old_modes_are_untouched(ctx):
    """flags == 0 and flags == KOCR_LINES_BLOCKS before and after a deskew call: the same bits, and their own launches only"""
    words = lc.small_pages()
    wq, wo = lc.flatten(words)
    flat = [bc.heading_columns_footer()[0], bc.staircase()[0]]
    fq, fo = bc.flatten(flat)
    pages = [dc.rotated(p, 17.0) for p in flat]
    quads, offsets = bc.flatten(pages)
    lines_before, rows = _rows_of(ctx, lambda: ctx.group_lines(wq, wo))
    assert rows == {"lines_group": 1, "lines_pack": 1}
    _assert_same(lines_before, ls.group_batch(words)[:4], "line mode before")
    blocks_before, rows = _rows_of(ctx, lambda: ctx.group_blocks(fq, fo))
    assert rows == {"blocks_cut": 1, "lines_pack": 1}
    _assert_same(blocks_before, bs.group_batch(flat), "block mode before")
    got, rows = _rows_of(ctx, lambda: ctx.group_blocks_deskewed(quads, offsets))
    assert rows == {"blocks_axis": 1, "blocks_frame": 1, "blocks_cut": 1, "blocks_unframe": 1, "lines_pack": 1}
    _assert_same(got, ds.group_batch(pages), "deskew between")
    _, rows = _rows_of(ctx, lambda: ctx.group_blocks_deskewed(quads, offsets, return_boxes=False))
    assert rows == {"blocks_axis": 1, "blocks_frame": 1, "blocks_cut": 1}
    blocks_after, rows = _rows_of(ctx, lambda: ctx.group_blocks(fq, fo))
    assert rows == {"blocks_cut": 1, "lines_pack": 1}
    lines_after, rows = _rows_of(ctx, lambda: ctx.group_lines(wq, wo))
    assert rows == {"lines_group": 1, "lines_pack": 1}
    assert all(a.tobytes() == b.tobytes() for a, b in zip(lines_before, lines_after))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(blocks_before, blocks_after))


def test_first_call_on_a_fresh_context_with_guards(stated):
    """a context whose first call is a deskew call, its arenas guarded; then the other two modes on the same arenas"""
    import keras_ocr_amd

    chosen = [s for s in stated if len(s[1]) in (65, 257, 1025) and not s[2]]
    pages = [s[1] for s in chosen] + [bc.page([])]
    quads, offsets = bc.flatten(pages)
    want = tuple(np.concatenate([s[3][f] for s in chosen] + ([np.zeros(1, I32)] if f == 2 else [])) for f in range(4))
    words = lc.small_pages()
    wq, wo = lc.flatten(words)
    flat = bc.heading_columns_footer()[0]
    c = keras_ocr_amd.Context(0)
    try:
        c.set_arena_guards(True)
        _assert_same(c.group_blocks_deskewed(quads, offsets), want, "first call")
        assert c.check_arena_guards()[0] == 0
        _assert_same(c.group_lines(wq, wo), ls.group_batch(words)[:4], "line mode after deskew")
        _assert_same(c.group_blocks(flat, [0, len(flat)]), bs.group_batch([flat]), "block mode after deskew")
        _assert_same(c.group_blocks_deskewed(quads, offsets), want, "deskew again")
        assert c.check_arena_guards()[0] == 0
    finally:
        c.set_arena_guards(False)
        c.close()


def test_layout_group_blocks_deskewed(ctx):
    from keras_ocr_amd import layout

    flat, blocks = bc.heading_columns_footer()
    pages = [dc.rotated(flat, -33.0), bc.page([]), dc.rotated(bc.hand_made()[1][1], 90.0)]
    got = layout.group_blocks_deskewed(pages, ctx=ctx)
    want = [ds.blocks_page(p) for p in pages]
    assert [[b.lines for b in p] for p in got] == [w["blocks"] for w in want] == [blocks, [], [[0, 1, 2], [3, 4, 5]]]
    for found, w in zip(got, want):
        assert [b.box.tobytes() for b in found] == [box.tobytes() for box in w["boxes"]]
    assert all(abs(layout.box_angle(b.box) + 33.0) < 1e-3 for b in got[0]) and all(abs(layout.box_angle(b.box) - 90.0) < 1e-3 for b in got[2])
    assert [[b.lines for b in p] for p in layout.group_blocks(pages, ctx=ctx)] != [w["blocks"] for w in want]


class _RotatedColumns:
    """a detector that finds two columns of eight lines of two words on a page turned by 10 degrees, in detector-input pixels
    (a duck-typed stage: the pipeline takes its stage-wise route)"""

    ANGLE = 10.0

    def __init__(self):
        words = []
        for cx, dy in ((30, 0), (146, 4)):  # gutter 30; the right column stands 4 lower
            for row in range(8):
                for k in range(2):
                    words.append(bc.box(cx + 46 * k, 4 + 18 * row + dy, 40, 12))
        flat = bc.page(words)
        self.left = flat[:, :, 0].max(axis=1) < 140
        self.boxes = dc.rotated(flat, self.ANGLE)

    def detect(self, images, **kwargs):
        return [self.boxes.copy() for _ in images]


def test_pipeline_end_to_end(crnn_weights):
    import keras_ocr_amd
    from keras_ocr_amd import layout

    columns = _RotatedColumns()
    assert columns.boxes[:, :, 0].min() >= 0 and columns.boxes[:, :, 0].max() < 256 and columns.boxes[:, :, 1].min() >= 0 and columns.boxes[:, :, 1].max() < 224
    context = keras_ocr_amd.Context(0)
    try:
        rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=context)
        pipe = keras_ocr_amd.pipeline.Pipeline(detector=columns, recognizer=rec)
        noise = np.random.default_rng(0).integers(0, 255, (112, 128, 3), dtype=np.uint8)
        axis = np.array([np.cos(np.radians(columns.ANGLE)), np.sin(np.radians(columns.ANGLE))])
        # along the text a left word ends before 116 + 4 detector pixels, in input-image pixels half of that
        side = lambda box: bool((np.asarray(box, np.float64) @ axis).max() < 65)  # noqa: E731
        lines = pipe.recognize_lines([noise])[0]
        assert len(lines) == 16 and all(len(ws) == 2 for _, _, ws in lines)
        runs = lambda blocks: sum(a != b for a, b in zip(blocks, blocks[1:]))  # noqa: E731
        blocks = pipe.recognize_blocks([noise], deskew=True)[0]
        words = [wb for _, _, members in blocks for _, _, ws in members for _, wb in ws]
        assert len(blocks) == 2 and [len(members) for _, _, members in blocks] == [8, 8]
        assert len(words) == 32 and [side(wb) for wb in words] == [True] * 16 + [False] * 16  # column after column
        want = ds.blocks_page(np.array([box for _, box, _ in lines], F32))
        assert [b.tobytes() for _, b, _ in blocks] == [b.tobytes() for b in want["boxes"]]
        assert all(abs(layout.box_angle(b) - columns.ANGLE) < 0.01 for _, b, _ in blocks)
        for text, _, members in blocks:
            assert text == "\n".join(t for t, _, _ in members) and text.count("\n") == 7
        # the same page without the switch: the gutter does not project to a gap along x, the columns interleave
        plain = pipe.recognize_blocks([noise])[0]
        sides = [side(wb) for _, _, members in plain for _, _, ws in members for _, wb in ws]
        assert len(sides) == 32 and runs(sides) > 1
        with pytest.raises(TypeError, match="deskew"):
            pipe.recognize_blocks([noise], deskew=1)
    finally:
        context.close()
