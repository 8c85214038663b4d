"""GPU suite: recognised words grouped into text lines on the device (kocr_group_lines) against its float64 statement
(tests/lines_statement.py): the integers equal, the line boxes bit for bit."""
import ctypes

import numpy as np
import pytest

from tests import lines_cases as lc
from tests import lines_statement as ls
from tests import stream_gate as sg

pytestmark = pytest.mark.gpu

I32, F32 = np.int32, np.float32


def _assert_same(got, want, what):
    """(line_of, order, line_counts, line_boxes) of the device against the statement's"""
    for name, g, w in zip(("line_of", "order", "line_counts"), got, want):
        assert g.dtype == np.int32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        different = np.flatnonzero(g != w)
        assert different.size == 0, (what, name, different[:5], g[different[:5]], w[different[:5]])
    g, w = got[3], want[3]
    assert g.dtype == np.float32 and g.shape == w.shape, (what, g.shape, w.shape)
    different = np.flatnonzero((g.view(np.uint32) != w.view(np.uint32)).reshape(-1, 8).any(axis=1))  # a line is 4 x 2 floats; no lines: nothing differs
    assert different.size == 0, (what, "line_boxes", different[:5], g[different[:5]], w[different[:5]])


@pytest.fixture(scope="module")
def batch():
    """the ragged batch of 64 random pages and the statement's answer, computed once"""
    pages = lc.random_batch()
    quads, offsets = lc.flatten(pages)
    *want, margin = ls.group_batch(pages)
    assert margin > 1e-9
    return pages, quads, offsets, want


def test_batch_equals_the_statement(ctx, batch):
    pages, quads, offsets, want = batch
    assert set(lc.BATCH_SIZES) <= {len(p) for p in pages} and len(pages) == 64
    got = ctx.group_lines(quads, offsets)
    _assert_same(got, want, "batch")
    assert want[2].sum() > 400 and len(want[3]) == want[2].sum()
    # without the boxes: the same integers
    line_of, order, counts, boxes = ctx.group_lines(quads, offsets, return_boxes=False)
    assert boxes is None
    _assert_same((line_of, order, counts, want[3]), want, "batch without boxes")


def test_hand_made_and_exact_cases(ctx):
    cases = lc.hand_made() + lc.exact_thresholds()
    rules = []
    for case in cases:
        if case[3] not in rules:
            rules.append(case[3])
    assert len(rules) == 2
    for rule in rules:
        chosen = [c for c in cases if c[3] == rule]
        quads, offsets = lc.flatten([c[1] for c in chosen])
        got = ctx.group_lines(quads, offsets, **rule)
        _assert_same(got, ls.group_batch([c[1] for c in chosen], **rule)[:4], f"cases with {rule}")
        # and the answers known by hand
        for k, (name, page, lines, _) in enumerate(chosen):
            assert got[2][k] == len(lines), name
            assert got[1][offsets[k]:offsets[k + 1]].tolist() == [j for line in lines for j in line], name


def test_other_rules(ctx):
    """every parameter away from its default, on random pages"""
    pages = lc.small_pages()
    quads, offsets = lc.flatten(pages)
    for rule in lc.OTHER_RULES:
        *want, margin = ls.group_batch(pages, **rule)
        assert margin > 1e-9, rule
        _assert_same(ctx.group_lines(quads, offsets, **rule), want, str(rule))


def test_long_chains(ctx):
    """512 words, each linked to its two neighbours only, in scrambled index order: one line; with the link in the middle
    broken: two"""
    for broken in (False, True):
        quads, lines = lc.chain(512, broken)
        got = ctx.group_lines(quads, [0, 512])
        assert got[2].tolist() == [len(lines)] and got[1].tolist() == [j for line in lines for j in line]
        _assert_same(got, ls.group_batch([quads])[:4], f"chain, broken={broken}")


def test_batch_independence(ctx, batch):
    """every page alone: the same integers and the same box bits as inside the batch"""
    pages, quads, offsets, _ = batch
    line_of, order, counts, boxes = ctx.group_lines(quads, offsets)
    first = np.concatenate([[0], np.cumsum(counts)])
    for k, page in enumerate(pages):
        alone = ctx.group_lines(page, [0, len(page)])
        inside = (line_of[offsets[k]:offsets[k + 1]], order[offsets[k]:offsets[k + 1]], counts[k:k + 1], boxes[first[k]:first[k + 1]])
        _assert_same(alone, inside, f"page {k} of {len(page)} words alone")


def _raw(lib, ctx, n, quads, offsets, cap, boxes=True, cos_max=None, total=None):
    from keras_ocr_amd import _lib

    total = len(quads) if total is None else total
    out = (np.full(total, -7, I32), np.full(total, -7, I32), np.full(max(n, 1), -7, I32), np.full((max(cap, 1), 4, 2), -7, F32))
    lines = ctypes.c_int64(-1)
    rc = lib.kocr_group_lines(ctx._h, n, _lib._ptr(quads), _lib._ptr(offsets), ls.cos_max_of(15.0) if cos_max is None else cos_max, 0.5, 0.5,  # pylint: disable=protected-access
                              1.5, _lib._ptr(out[0]), _lib._ptr(out[1]), _lib._ptr(out[2]), _lib._ptr(out[3]) if boxes else None, cap if boxes else 0,
                              ctypes.byref(lines), 0)
    return rc, lines.value, out, lib.kocr_last_error(ctx._h)  # pylint: disable=protected-access


def test_raw_abi(ctx):
    import keras_ocr_amd
    from keras_ocr_amd import _lib

    lib = keras_ocr_amd.load_library()
    pages = [lc.page(lc.row(0, 0, [30, 30]) + lc.row(0, 40, [30])), lc.page([]), lc.page(lc.row(0, 0, [30, 30, 30]))]  # 2 + 0 + 1 lines
    quads, offsets = lc.flatten(pages)
    want = ls.group_batch(pages)[:4]
    rc, lines, _, message = _raw(lib, ctx, 3, quads, offsets, 2)
    assert rc == _lib.KOCR_ECAPACITY and lines == 3 and b"3 lines" in message
    rc, lines, out, _ = _raw(lib, ctx, 3, quads, offsets, 3)
    assert rc == 0 and lines == 3
    _assert_same((out[0], out[1], out[2], out[3][:3]), want, "raw call")
    rc, lines, out, _ = _raw(lib, ctx, 3, quads, offsets, 0, boxes=False)  # line_boxes == NULL
    assert rc == 0 and lines == 3 and (out[3] == -7).all()
    _assert_same((out[0], out[1], out[2], want[3]), want, "raw call without boxes")
    # refusals, each with its message
    many = np.zeros((3 + 2049, 4, 2), F32)
    rc, _, _, message = _raw(lib, ctx, 2, many, np.array([0, 3, 3 + 2049], I32), 8)
    assert rc == _lib.KOCR_EINVAL and b"page 1 holds 2049 words" in message
    rc, _, _, message = _raw(lib, ctx, 3, quads, np.array([0, 4, 3, 6], I32), 8)
    assert rc == _lib.KOCR_EINVAL and b"offsets decreases at entry 2" in message
    bad = quads.copy()
    bad[5, 2, 1] = np.nan
    rc, _, _, message = _raw(lib, ctx, 3, bad, offsets, 8)
    assert rc == _lib.KOCR_EINVAL and b"page 2, word 2: non-finite coordinate" in message
    with pytest.raises(ValueError, match="page 2, word 2"):
        ctx.group_lines(bad, offsets)
    bad[5, 2, 1] = np.inf
    assert _raw(lib, ctx, 3, bad, offsets, 8)[0] == _lib.KOCR_EINVAL
    # max_angle = 90: refused by name where the angle is an argument, as its cosine 0 at the C boundary
    with pytest.raises(ValueError, match="max_angle"):
        ctx.group_lines(quads, offsets, max_angle=90)
    rc, _, _, message = _raw(lib, ctx, 3, quads, offsets, 8, cos_max=0.0)
    assert rc == _lib.KOCR_EINVAL and b"cos_max" in message and b"max_angle" in message
    for rule in ({"min_height_ratio": 1.5}, {"max_offset": -1.0}, {"max_gap": float("nan")}):
        with pytest.raises(ValueError, match=next(iter(rule))):
            ctx.group_lines(quads, offsets, **rule)
    with pytest.raises(ValueError, match="2049"):
        ctx.group_lines(many, [0, 3, 3 + 2049])
    # N = 0 and a batch of empty pages
    rc, lines, _, _ = _raw(lib, ctx, 0, lc.page([]), np.array([0], I32), 0)
    assert rc == 0 and lines == 0
    rc, lines, out, _ = _raw(lib, ctx, 3, lc.page([]), np.array([0, 0, 0, 0], I32), 0)
    assert rc == 0 and lines == 0 and out[2].tolist() == [0, 0, 0]
    got = ctx.group_lines(lc.page([]), [0, 0, 0])
    assert [a.shape for a in got] == [(0,), (0,), (2,), (0, 4, 2)] and got[2].tolist() == [0, 0]
    assert [a.shape for a in ctx.group_lines(lc.page([]), [0])] == [(0,), (0,), (0,), (0, 4, 2)]
    # the call after all of that is unharmed
    _assert_same(ctx.group_lines(quads, offsets), want, "after the refusals")


def test_on_a_caller_stream(ctx):
    """on a stream handed over with kocr_set_stream, behind long-running work queued there, the call gives the arrays it
    gives on the context's own stream, complete on return"""
    import torch
    import keras_ocr_amd

    lib = keras_ocr_amd.load_library()
    pages = lc.small_pages()
    quads, offsets = lc.flatten(pages)
    poison, _ = lc.flatten(lc.small_pages(shift=10))
    total, lines = len(quads), int(ls.group_batch(pages)[2].sum())
    case = sg.Case("kocr_group_lines", [3, sg.In(quads, poison), offsets, ls.cos_max_of(15.0), 0.5, 0.5, 1.5, sg.Out(total, I32), sg.Out(total, I32),
                                        sg.Out(3, I32), sg.Out((total, 4, 2), F32), total, np.zeros(1, np.int64)], False,
                   view=lambda outs: outs[:3] + [outs[3][:lines]])
    stream = torch.cuda.Stream()
    try:
        ctx.set_stream(None)
        rc, outs, _ = sg.host_call(lib, ctx, case)
        assert rc == 0
        want = case.view(outs)
        _assert_same(want, ls.group_batch(pages)[:4], "own stream")
        rc, outs, _ = sg.host_call(lib, ctx, case, "poison")
        assert rc == 0 and not sg.same_bits(case.view(outs)[:2], want[:2])
        ctx.set_stream(stream.cuda_stream)
        rc, outs, _ = sg.host_call(lib, ctx, case)
        assert rc == 0 and sg.same_bits(case.view(outs), want)
        sg.host_call(lib, ctx, case, "poison")  # what the arenas hold before the gated call is not its answer
        g = sg.gated_call(lib, ctx, case, stream, sg.Gate(), on_device=0)
        assert g.rc == 0 and sg.same_bits(case.view(g.outs), want), "the host outputs were not complete and correct on return"
        assert g.gate_ms > 10 * g.call_ms or g.gate_ms > 50, (g.gate_ms, g.call_ms)
    finally:
        ctx.set_stream(None)


def test_layout_and_pipeline(craft_weights, crnn_weights):
    """the small synthetic page of test_evaluation_gpu.py::test_pipeline_evaluate, the detector's head calibrated as in
    __graft_entry__.smoke"""
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
        pipe = keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)
        images = [page, page]
        plain = pipe.recognize(images)
        assert len(plain[0]) > 0 and len(plain[1]) > 0
        for rule in ({}, {"max_gap": 40.0, "max_offset": 0.8}):
            got = pipe.recognize_lines(images, **rule)
            assert len(got) == len(plain)
            for words, lines in zip(plain, got):
                want = ls.group_page(np.array([box for _, box in words], np.float32), **rule)
                assert len(lines) == len(want["lines"])
                members = [w for _, _, ws in lines for w in ws]
                # a permutation of recognize()'s tuples, the boxes the same bits
                assert sorted(t for t, _ in members) == sorted(t for t, _ in words)
                assert [(t, b.tobytes()) for t, b in members] == [(words[j][0], words[j][1].tobytes()) for j in want["order"]]
                for (text, box, ws), indices, want_box in zip(lines, want["lines"], want["boxes"]):
                    assert text == " ".join(words[j][0] for j in indices) == " ".join(t for t, _ in ws)
                    assert box.dtype == np.float32 and box.tobytes() == want_box.tobytes()
            # layout.group_lines on the boxes alone, on the default context and on this one
            stated = [ls.group_page(np.array([box for _, box in words], np.float32), **rule) for words in plain]
            for ctx_arg in (None, context):
                pages = layout.group_lines([[box for _, box in words] for words in plain], ctx=ctx_arg, **rule)
                assert [[(line.words, line.box.tobytes()) for line in p] for p in pages] == \
                    [[(indices, box.tobytes()) for indices, box in zip(want["lines"], want["boxes"])] for want in stated]
        assert layout.group_lines([[], np.array([])], ctx=context) == [[], []]
        assert pipe.recognize_lines([]) == []
        with pytest.raises(ValueError, match="beam_width"):
            pipe.recognize_lines([page], recognition_kwargs={"beam_width": 4})
        with pytest.raises(ValueError, match="lexicon_top"):
            pipe.recognize_lines([page], recognition_kwargs={"lexicon_top": 2})
    finally:
        context.close()
