"""GPU suite: the boxes of a page cut into blocks in reading order on the device (kocr_group_lines with flags ==
KOCR_LINES_BLOCKS) against its float64 statement (tests/blocks_statement.py): the integers equal, the block boxes bit for
bit; and the same call with flags == 0 untouched by it."""
import ctypes

import numpy as np
import pytest

from tests import blocks_cases as bc
from tests import blocks_statement as bs
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
    """every case with the statement's answer, computed once: (name, quads, blocks by hand or None, rule, answer)"""
    return [case + (bs.group_batch([case[1]], **case[3]),) for case in bc.every_case()]


def test_every_case_equals_the_statement(ctx, stated):
    assert len(stated) > 35
    for name, quads, blocks, rule, want in stated:
        got = ctx.group_blocks(quads, [0, len(quads)], **rule)
        _assert_same(got, want, name)
        if blocks is not None:  # and the answers known by hand
            assert got[2].tolist() == [len(blocks)] and got[1].tolist() == [j for b in blocks for j in b], name
    # without the boxes: the same integers
    name, quads, _, rule, want = next(s for s in stated if s[0] == "layout 300")
    block_of, order, counts, boxes = ctx.group_blocks(quads, [0, len(quads)], return_boxes=False, **rule)
    assert boxes is None
    _assert_same((block_of, order, counts, want[3]), want, "layout 300 without boxes")


def test_a_page_alone_and_inside_a_batch(ctx):
    pages = bc.mixed_batch()
    assert sum(len(p) == 0 for p in pages) >= 4
    quads, offsets = bc.flatten(pages)
    want = bs.group_batch(pages)
    got = ctx.group_blocks(quads, offsets)
    _assert_same(got, want, "mixed batch")
    block_of, order, counts, boxes = got
    first = np.concatenate([[0], np.cumsum(counts)])
    for k, page in enumerate(pages):
        alone = ctx.group_blocks(page, [0, len(page)])
        inside = (block_of[offsets[k]:offsets[k + 1]], order[offsets[k]:offsets[k + 1]], counts[k:k + 1], boxes[first[k]:first[k + 1]])
        _assert_same(alone, inside, f"page {k} of {len(page)} quads alone")
    # a small page beside the largest one runs in a block sized for the largest
    small, large = bc.heading_columns_footer()[0], next(c[1] for c in bc.random_cases() if len(c[1]) == 2048 and not c[3])
    both = ctx.group_blocks(*bc.flatten([small, large, small]))
    _assert_same(both, bs.group_batch([small, large, small]), "small, 2048, small")


def _raw(lib, ctx, n, quads, offsets, cap, flags, boxes=True, gaps=(1.0, 0.75), total=None):
    from keras_ocr_amd import _lib

    total = len(quads) if total is None else total
    out = (np.full(total, -7, I32), np.full(total, -7, I32), np.full(max(n, 1), -7, I32), np.full((max(cap, 1), 4, 2), -7, F32))
    count = ctypes.c_int64(-1)
    rc = lib.kocr_group_lines(ctx._h, n, _lib._ptr(quads), _lib._ptr(offsets), ls.cos_max_of(15.0), 0.5, gaps[0], gaps[1], _lib._ptr(out[0]),  # pylint: disable=protected-access
                              _lib._ptr(out[1]), _lib._ptr(out[2]), _lib._ptr(out[3]) if boxes else None, cap if boxes else 0, ctypes.byref(count), flags)
    return rc, count.value, out, lib.kocr_last_error(ctx._h)  # pylint: disable=protected-access


def test_raw_abi(ctx):
    import keras_ocr_amd
    from keras_ocr_amd import _lib

    lib = keras_ocr_amd.load_library()
    blocks = _lib.KOCR_LINES_BLOCKS
    pages = [bc.hand_made()[1][1], bc.page([]), bc.page([bc.box(0, 0, 30, 10)])]  # 2 + 0 + 1 blocks
    quads, offsets = bc.flatten(pages)
    want = bs.group_batch(pages)
    # capacity one too small: the code, the true number, and the integer outputs complete
    rc, count, out, message = _raw(lib, ctx, 3, quads, offsets, 2, blocks)
    assert rc == _lib.KOCR_ECAPACITY and count == 3 and b"3 blocks" in message
    _assert_same((out[0], out[1], out[2], want[3]), want, "capacity too small")
    assert (out[3] == -7).all()
    rc, count, out, _ = _raw(lib, ctx, 3, quads, offsets, 3, blocks)
    assert rc == 0 and count == 3
    _assert_same((out[0], out[1], out[2], out[3][:3]), want, "raw call")
    rc, count, out, _ = _raw(lib, ctx, 3, quads, offsets, 0, blocks, boxes=False)  # line_boxes == NULL
    assert rc == 0 and count == 3 and (out[3] == -7).all()
    _assert_same((out[0], out[1], out[2], want[3]), want, "raw call without boxes")
    # any other flag
    for flags in (2, 3, -1):
        rc, _, out, message = _raw(lib, ctx, 3, quads, offsets, 8, flags)
        assert rc == _lib.KOCR_EINVAL and b"flags" in message and (out[0] == -7).all(), flags
    # the gaps: line mode's checks of max_offset and max_gap, with their messages
    for gaps, name in (((-1.0, 0.75), b"max_offset"), ((float("nan"), 0.75), b"max_offset"), ((float("inf"), 0.75), b"max_offset"),
                       ((1.0, -0.5), b"max_gap"), ((1.0, float("nan")), b"max_gap"), ((1.0, float("inf")), b"max_gap")):
        rc, _, _, message = _raw(lib, ctx, 3, quads, offsets, 8, blocks, gaps=gaps)
        assert rc == _lib.KOCR_EINVAL and name in message and b"is not a finite number >= 0" in message, gaps
    for rule in ({"min_gap_x": -1.0}, {"min_gap_y": float("nan")}, {"min_gap_y": float("inf")}):
        with pytest.raises(ValueError, match=next(iter(rule))):
            ctx.group_blocks(quads, offsets, **rule)
    # the other refusals, with line mode's messages
    many = np.zeros((3 + 2049, 4, 2), F32)
    rc, _, _, message = _raw(lib, ctx, 2, many, np.array([0, 3, 3 + 2049], I32), 8, blocks)
    assert rc == _lib.KOCR_EINVAL and b"page 1 holds 2049 words" in message
    with pytest.raises(ValueError, match="2049"):
        ctx.group_blocks(many, [0, 3, 3 + 2049])
    rc, _, _, message = _raw(lib, ctx, 3, quads, np.array([0, 4, 3, 7], I32), 8, blocks)
    assert rc == _lib.KOCR_EINVAL and b"offsets decreases at entry 2" in message
    for value in (np.nan, np.inf):
        bad = quads.copy()
        bad[6, 2, 1] = value
        rc, _, _, message = _raw(lib, ctx, 3, bad, offsets, 8, blocks)
        assert rc == _lib.KOCR_EINVAL and b"page 2, word 0: non-finite coordinate" in message
        with pytest.raises(ValueError, match="page 2, word 0"):
            ctx.group_blocks(bad, offsets)
    # N = 0 and a batch of empty pages
    rc, count, _, _ = _raw(lib, ctx, 0, bc.page([]), np.array([0], I32), 0, blocks)
    assert rc == 0 and count == 0
    rc, count, out, _ = _raw(lib, ctx, 3, bc.page([]), np.array([0, 0, 0, 0], I32), 0, blocks)
    assert rc == 0 and count == 0 and out[2].tolist() == [0, 0, 0]
    got = ctx.group_blocks(bc.page([]), [0, 0, 0])
    assert [a.shape for a in got] == [(0,), (0,), (2,), (0, 4, 2)] and got[2].tolist() == [0, 0]
    assert [a.shape for a in ctx.group_blocks(bc.page([]), [0])] == [(0,), (0,), (0,), (0, 4, 2)]
    # the call after all of that is unharmed
    _assert_same(ctx.group_blocks(quads, offsets), want, "after the refusals")


def test_first_call_on_a_fresh_context_with_guards():
    """a context whose first call is a block-mode call, its arenas guarded; then a line-mode call on the same arenas"""
    import keras_ocr_amd

    pages = [c[1] for c in bc.random_cases() if len(c[1]) in (65, 300, 1025) and not c[3]] + [bc.page([])]
    quads, offsets = bc.flatten(pages)
    words = lc.small_pages()
    wq, wo = lc.flatten(words)
    c = keras_ocr_amd.Context(0)
    try:
        c.set_arena_guards(True)
        _assert_same(c.group_blocks(quads, offsets), bs.group_batch(pages), "first call")
        assert c.check_arena_guards()[0] == 0
        _assert_same(c.group_lines(wq, wo), ls.group_batch(words)[:4], "line mode after block mode")
        _assert_same(c.group_blocks(quads, offsets), bs.group_batch(pages), "block mode again")
        assert c.check_arena_guards()[0] == 0
    finally:
        c.set_arena_guards(False)
        c.close()


def _rows_of(ctx, call):
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        out = call()
        rows = ctx.profile_report()
    finally:
        ctx.profile_enable(False)
    return out, {name: row["launches"] for name, row in rows.items() if row["launches"]}


def test_line_mode_is_untouched(ctx):
    """flags == 0 before and after block-mode calls: the same bits, and its own two launches only"""
    words = lc.small_pages()
    wq, wo = lc.flatten(words)
    pages = [bc.heading_columns_footer()[0], bc.staircase()[0]]
    quads, offsets = bc.flatten(pages)
    before, rows = _rows_of(ctx, lambda: ctx.group_lines(wq, wo))
    assert rows == {"lines_group": 1, "lines_pack": 1}
    _assert_same(before, ls.group_batch(words)[:4], "line mode before")
    got, rows = _rows_of(ctx, lambda: ctx.group_blocks(quads, offsets))
    assert rows == {"blocks_cut": 1, "lines_pack": 1}
    _assert_same(got, bs.group_batch(pages), "block mode between")
    _, rows = _rows_of(ctx, lambda: ctx.group_blocks(quads, offsets, return_boxes=False))
    assert rows == {"blocks_cut": 1}
    after, rows = _rows_of(ctx, lambda: ctx.group_lines(wq, wo))
    assert rows == {"lines_group": 1, "lines_pack": 1}
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


class _Columns:
    """a detector that finds two columns of three lines of two words, in detector-input pixels (a duck-typed stage: the
    pipeline takes its stage-wise route)"""

    def __init__(self):
        words = []
        for cx, dy in ((4, 0), (130, 4)):  # the right column stands 4 lower: by centre y the lines alternate left, right
            for row in range(3):
                for k in range(2):
                    words.append(bc.box(cx + 46 * k, 6 + 18 * row + dy, 40, 12))
        self.boxes = bc.page(words)
        self.left = self.boxes[:, :, 0].max(axis=1) < 128

    def detect(self, images, **kwargs):
        return [self.boxes.copy() for _ in images]


def _column_runs(sides):
    """how often the side changes along a reading order"""
    return sum(a != b for a, b in zip(sides, sides[1:]))


def test_pipeline_end_to_end(craft_weights, crnn_weights):
    import keras_ocr_amd
    from keras_ocr_amd import layout
    from oracle import craft as ocraft, tools as otools

    rng = np.random.default_rng(0)
    page = np.full((64, 96, 3), 255, np.uint8)
    for _ in range(4):
        x, y = int(rng.integers(0, 60)), int(rng.integers(0, 50))
        page[y:y + 10, x:x + 30] = rng.integers(0, 120, (10, 30, 3), dtype=np.uint8)
    big = otools.resize_image(page, 2, 2048)[0][None]
    cw = keras_ocr_amd.weights.calibrate_craft_head(craft_weights, ocraft.detector_predict(craft_weights, big), text_frac=0.12, link_frac=0.05)
    context = keras_ocr_amd.Context(0)
    try:
        det = keras_ocr_amd.detection.Detector(weights=cw, ctx=context)
        rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=context)
        # 1. the detector's own boxes, whatever they are: recognize_blocks is recognize_lines + group_blocks + the statement
        pipe = keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)
        images = [page, page]
        lines_before = pipe.recognize_lines(images)
        assert all(len(lines) > 0 for lines in lines_before)
        for rule in ({}, {"min_gap_x": 0.25, "min_gap_y": 0.1}):
            got = pipe.recognize_blocks(images, **rule)
            cut = layout.group_blocks([[box for _, box, _ in lines] for lines in lines_before], ctx=context, **rule)
            assert len(got) == len(cut) == 2
            for lines, blocks, found in zip(lines_before, got, cut):
                want = bs.blocks_page(np.array([box for _, box, _ in lines], F32), **rule)
                assert [b.lines for b in found] == want["blocks"] and len(blocks) == len(want["blocks"])
                for (text, box, members), indices, want_box in zip(blocks, want["blocks"], want["boxes"]):
                    assert text == "\n".join(lines[j][0] for j in indices)
                    assert box.dtype == np.float32 and box.tobytes() == want_box.tobytes()
                    assert [(t, b.tobytes(), [(wt, wb.tobytes()) for wt, wb in ws]) for t, b, ws in members] == \
                        [(lines[j][0], lines[j][1].tobytes(), [(wt, wb.tobytes()) for wt, wb in lines[j][2]]) for j in indices]
        lines_after = pipe.recognize_lines(images)
        assert [[(t, b.tobytes()) for t, b, _ in lines] for lines in lines_after] == [[(t, b.tobytes()) for t, b, _ in lines] for lines in lines_before]
        assert pipe.recognize_blocks([]) == []
        with pytest.raises(ValueError, match="beam_width"):
            pipe.recognize_blocks([page], recognition_kwargs={"beam_width": 4})
        # 2. a two-column page (the boxes from a stand-in detector, read by the recogniser): the columns do not interleave
        columns = _Columns()
        pipe = keras_ocr_amd.pipeline.Pipeline(detector=columns, recognizer=rec)
        noise = rng.integers(0, 255, (64, 128, 3), dtype=np.uint8)
        lines = pipe.recognize_lines([noise])[0]
        side = lambda box: bool(box[:, 0].max() < 64)  # noqa: E731  input-image pixels: half the detector's
        assert len(lines) == 6 and all(len(ws) == 2 for _, _, ws in lines)
        assert _column_runs([side(box) for _, box, _ in lines]) == 5  # left, right, left, right, ...: what the issue is about
        blocks = pipe.recognize_blocks([noise])[0]
        assert len(blocks) == 2 and [len(members) for _, _, members in blocks] == [3, 3]
        words = [wb for _, _, members in blocks for _, _, ws in members for _, wb in ws]
        assert len(words) == 12 and [side(wb) for wb in words] == [True] * 6 + [False] * 6
        assert [[(t, b.tobytes()) for t, b, _ in members] for _, _, members in blocks] == \
            [[(t, b.tobytes()) for t, b, _ in lines[0::2]], [(t, b.tobytes()) for t, b, _ in lines[1::2]]]
        for text, _, members in blocks:
            assert text == "\n".join(t for t, _, _ in members) and text.count("\n") == 2
        want = bs.blocks_page(np.array([box for _, box, _ in lines], F32))
        assert want["blocks"] == [[0, 2, 4], [1, 3, 5]] and [b.tobytes() for _, b, _ in blocks] == [b.tobytes() for b in want["boxes"]]
    finally:
        context.close()
