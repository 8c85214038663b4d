"""Long words without a GPU ("Long words"): tools.window_plan, the host mirror of the rule's integer
part, against tests/windows_statement.py on a grid; the properties the rule promises; and the stitched decode statement
against a sum over all paths on a toy crop."""
import itertools
import math

import numpy as np
import pytest

from keras_ocr_amd import tools
from tests import ctc_statement as cs
from tests import windows_cases as wc
from tests import windows_statement as ws


def test_window_plan_equals_the_statement_on_the_grid():
    grid = wc.wh_grid()
    seen_k, long_edges = set(), 0
    for w, h, aspect, overlap in grid:
        for discard in wc.DISCARDS:
            try:
                want = ws.plan(w, h, aspect, overlap, discard)
            except ValueError:
                with pytest.raises(ValueError):
                    tools.window_plan(w, h, aspect, overlap, discard)
                continue
            if want[3] > 4 * ws.FRAMES_MAX:
                continue
            got = tools.window_plan(w, h, aspect, overlap, discard)
            assert (got.windows, got.fractions, got.ranges, got.frames) == want, (w, h, aspect, overlap, discard)
            seen_k.add(want[0])
        # the two sides of "long" are both there for this (h, aspect)
        long_edges += float(w) > aspect * float(h)
    assert {1, 2, 3} <= seen_k and any(38 <= k <= 42 for k in seen_k)
    assert 0 < long_edges < len(grid)
    assert any(h == 1 for _, h, _, _ in grid)


def test_the_grid_has_the_k_boundaries():
    """31 w - 200 h an exact multiple of S h, and one above it: K steps by one between the two"""
    steps = 0
    for overlap in wc.OVERLAPS:
        stride = 200 - overlap
        for h in (31, 62):
            for k in (1, 2, 39):
                w = (k * stride + 200) * h // 31
                assert 31 * w - 200 * h == k * stride * h  # exact: h is a multiple of 31
                if float(w) > 10.0 * float(h):
                    assert ws.plan(w, h, 10.0, overlap, 2)[0] == k + 1 and ws.plan(w + 1, h, 10.0, overlap, 2)[0] == k + 2
                    assert (w, h, 10.0, overlap) in wc.wh_grid() and (w + 1, h, 10.0, overlap) in wc.wh_grid()
                    steps += 1
    assert steps >= 6


def test_just_below_at_and_above_the_aspect():
    for h in (8, 31):
        assert tools.window_plan(10 * h - 1, h).windows == 1
        assert tools.window_plan(10 * h, h).windows == 1  # long iff w > A h, strictly
        assert tools.window_plan(10 * h + 1, h).windows >= 2
    assert tools.window_plan(1661, 8).windows == 40 and tools.window_plan(1661, 8).frames == 39 * 40 + 48


@pytest.mark.parametrize("overlap", wc.OVERLAPS)
@pytest.mark.parametrize("discard", wc.DISCARDS)
def test_properties(overlap, discard):
    f, stride = overlap // 8, 200 - overlap
    for w, h, aspect, o in wc.wh_grid():
        if o != overlap:
            continue
        K, fractions, ranges, frames = ws.plan(w, h, aspect, overlap, discard)
        if K > 200:
            continue
        assert all(lo < hi for lo, hi in ranges)  # every window keeps frames
        assert sum(hi - lo for lo, hi in ranges) == frames == (K - 1) * stride // 4 + 50 - discard  # they tile [0, T')
        assert fractions[0][0] == 0.0 and fractions[-1][1] == 1.0
        assert ranges[0][0] == discard and ranges[-1][1] == 50
        if K == 1:
            continue
        scale = 31 / h  # crop pixels per box pixel
        for k in range(K - 1):
            # consecutive windows meet at the same nominal crop x: frame hi_k of window k and frame lo_{k+1} of window k + 1
            x_end = fractions[k][0] * w * scale + 4 * ranges[k][1]
            x_begin = fractions[k + 1][0] * w * scale + 4 * ranges[k + 1][0]
            assert abs(x_end - x_begin) < 1e-6 * max(1.0, x_end)
            assert ranges[k][1] == 50 - f and ranges[k + 1][0] == f
            assert fractions[k][1] < 1.0 or k == K - 2  # only the last two windows may reach the end
        # the last window is longer than the overlap: more than O h / 31 box pixels
        assert (1.0 - fractions[-1][0]) * w > overlap * h / 31 * (1 - 1e-12)
        # and the one before it does not hold the whole box
        assert fractions[-2][0] * w * scale + 200 < w * scale + 1e-6


def test_refusals():
    for bad in (dict(aspect=6.4), dict(aspect=float("nan")), dict(aspect=float("inf")), dict(overlap=12), dict(overlap=104), dict(overlap=44),
                dict(overlap=8), dict(discard=-1), dict(overlap=96, discard=38), dict(overlap=40, discard=45)):
        with pytest.raises(ValueError):
            tools.window_plan(400, 20, **bad)
        with pytest.raises(ValueError):
            ws.plan(400, 20, **{"aspect": 10.0, "overlap": 40, "discard": 2, **bad})
    assert tools.window_plan(400, 20, overlap=96, discard=37).windows > 1  # d < 50 - f = 38
    assert tools.window_plan(400, 20, aspect=200 / 31).windows > 1
    for w, h in ((0, 5), (5, 0)):
        with pytest.raises(ZeroDivisionError):
            tools.window_plan(w, h)
        with pytest.raises(ZeroDivisionError):
            ws.plan(w, h)


def test_geometry_of_the_statement():
    """K = 1 is the ordered box itself; the end points of a long box are its own corners, bit for bit; neighbours overlap"""
    from oracle import tools as otools

    for box in wc.PLAN_BOXES:
        ob, _ = otools.get_rotated_box(box)
        K, quads, ranges, frames = ws.windows(box)
        assert quads.shape == (K, 4, 2) and quads.dtype == np.float32 and len(ranges) == K
        if K == 1:
            assert np.array_equal(quads[0], np.asarray(ob, np.float32))
            continue
        assert np.array_equal(quads[0][[0, 3]], np.asarray(ob, np.float32)[[0, 3]])    # tl, bl
        assert np.array_equal(quads[-1][[1, 2]], np.asarray(ob, np.float32)[[1, 2]])   # tr, br
        along = np.asarray(ob, np.float64)[1] - np.asarray(ob, np.float64)[0]
        pos = lambda p: float((np.asarray(p, np.float64) - np.asarray(ob, np.float64)[0]) @ along) / float(along @ along)  # noqa: E731
        for k in range(K - 1):
            assert pos(quads[k][0]) < pos(quads[k + 1][0]) < pos(quads[k][1]) <= pos(quads[k + 1][1]) + 1e-9
    assert sorted({ws.windows(b)[0] for b in wc.PLAN_BOXES})[:4] == [1, 2, 3, 4]
    with pytest.raises(ValueError):
        ws.windows(wc.rect(0, 0, 3000, 8))  # 31 * 3000 / 8 crop pixels: more than 2048 frames


def _brute_force(probs, label):
    lq = cs.log_q(probs[np.newaxis])[0]
    T, C = lq.shape
    total = 0.0
    for path in itertools.product(range(C), repeat=T):
        if cs.collapse(path, C - 1) == label:
            total += math.exp(sum(lq[t, c] for t, c in enumerate(path)))
    return math.log(total)


@pytest.mark.parametrize("seed", range(4))
def test_stitched_decode_against_all_paths(seed):
    """a toy stitch: 2 windows of 4 frames of 4 pixels (a 16-pixel crop), overlap 8 -> f = 1, 6 frames, 3 classes; also a
    single window and 3 windows (8 frames)"""
    rng = np.random.default_rng(seed)
    frames, px, overlap, discard = 4, 4, 8, 0
    counts = [2, 1, 3]
    logits = rng.normal(0, 2, (sum(counts), frames, 3))
    if seed == 0:  # a run across the seam: class 0 wins the last kept frame of window 0 and the first kept one of window 1
        logits[0, 2, 0] = logits[1, 1, 0] = 6.0
    seqs = ws.stitch(logits, counts, overlap, discard, frames, px)
    assert [len(s) for s in seqs] == [6, 4, 8]
    assert np.array_equal(seqs[0], np.concatenate([logits[0, 0:3], logits[1, 1:4]]))
    assert np.array_equal(seqs[2], np.concatenate([logits[3, 0:3], logits[4, 1:3], logits[5, 1:4]]))
    for (labels, chars, logw, n, _), seq in zip(ws.stitch_decode(logits, counts, overlap, discard, frames, px), seqs):
        probs = ws.softmax(seq)
        assert n == len(seq) and len(chars) == len(labels)
        assert labels == cs.collapse(list(probs.argmax(-1)), 2)
        assert abs(logw - _brute_force(probs, labels)) < 1e-9
    if seed == 0:
        first = ws.stitch_decode(logits, counts, overlap, discard, frames, px)[0][0]
        path = list(ws.softmax(seqs[0]).argmax(-1))
        assert path[2] == path[3] == 0 and first.count(0) == len([i for i in range(6) if path[i] == 0 and (i == 0 or path[i - 1] != 0)])


def test_chosen_logits_decode_as_stated():
    for overlap, discard in itertools.product((16, 96), wc.DISCARDS):
        for classes in (37, 96):
            logits, counts, expect = wc.chosen_logits(classes, overlap, discard)
            got = ws.stitch_decode(logits, counts, overlap, discard)
            assert [g[0] for g in got] == expect, (overlap, discard, classes)
            assert [g[3] for g in got] == [(k - 1) * (200 - overlap) // 4 + 50 - discard for k in counts]
