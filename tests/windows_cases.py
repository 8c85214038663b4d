"""Cases of the long-word tests (tests/test_windows_statement_cpu.py, tests/test_windows_gpu.py): pure numpy, seeded, built
once.  Nothing here touches a GPU."""
import functools

import numpy as np

F32 = np.float32
OVERLAPS = (16, 40, 96)
DISCARDS = (0, 2, 5)
ASPECTS = (200 / 31, 10.0, 12.5)


def wh_grid():
    """(w, h, aspect, overlap) of the plan grid: per (aspect, overlap, h) the widths just below, at and just above aspect * h,
    the K boundaries -- 31 w - 200 h an exact multiple of S h where an integer w gives one, and one above it -- for K = 2, 3
    and about 40, and h = 1"""
    out = []
    for aspect in ASPECTS:
        for overlap in OVERLAPS:
            stride = 200 - overlap
            for h in (1, 8, 31, 62):
                edge = int(aspect * h)
                ws = {max(edge - 1, 1), edge, edge + 1, edge + 2, 7 * h, 21 * h}
                for k in (1, 2, 39):
                    # 31 w - 200 h = k S h  <=>  w = (k S + 200) h / 31
                    num = (k * stride + 200) * h
                    ws |= {num // 31, num // 31 + 1}
                    if num % 31 == 0:
                        ws.add(num // 31 - 1)
                out += [(w, h, aspect, overlap) for w in sorted(ws) if w >= 1]
    return out


def rect(x0, y0, w, h):
    return np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]], F32)


def rotated(cx, cy, w, h, degrees):
    a = np.radians(degrees)
    r = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return (np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]]) @ r.T + [cx, cy]).astype(F32)


def trapezoid(x0, y0, w, h, pinch):
    """a mild trapezoid: the right side shorter by 2 * pinch"""
    return np.array([[x0, y0], [x0 + w, y0 + pinch], [x0 + w, y0 + h - pinch], [x0, y0 + h]], F32)


# On a 120 x 400 page.  At aspect 10, overlap 40: a short word, a box at 6.5 : 1 (wider than the crop, not long), K = 2, 3 and 4,
# the same rotated by 30 and 80 degrees, a mild trapezoid, a long box partly outside the page, and a thin one
PLAN_BOXES = np.stack([
    rect(10, 10, 60, 20), rect(10, 40, 130, 20), rect(5, 70, 180, 16), rect(5, 90, 300, 16), rect(5, 5, 390, 14),
    rotated(200, 60, 180, 16, 30), rotated(200, 60, 110, 10, 80), rotated(200, 60, 300, 16, 30), trapezoid(20, 30, 320, 20, 2),
    rect(250, 100, 200, 12), rect(3, 60, 390, 8)])


def long_box(y, h=8, w=1661, x=10):
    return rect(x, y, w, h)


@functools.lru_cache(maxsize=None)
def page(h=120, w=400, seed=7):
    """a noisy page with dark strokes: every crop of it has structure everywhere"""
    rng = np.random.default_rng(seed)
    img = rng.integers(150, 256, (h, w, 3), dtype=np.uint8)
    for _ in range(h * w // 60):
        y, x = int(rng.integers(0, h - 3)), int(rng.integers(0, w - 3))
        img[y:y + int(rng.integers(1, 4)), x:x + int(rng.integers(1, 4))] = rng.integers(0, 100, 3, dtype=np.uint8)
    img.flags.writeable = False
    return img


def random_logits(rng, n, classes, scale=3.0):
    return rng.normal(0, scale, (n, 50, classes)).astype(F32)


def chosen_logits(classes, overlap, discard):
    """Logits (sum K, 50, classes) and K per word for the seam cases, at f = overlap / 8 and d = discard; every frame is the
    blank unless said otherwise (class a = 3, b = 5, blank = classes - 1).  Words, in order:
      0  K = 2: label a in the last kept frames of window 0 and the first kept frames of window 1 -- one run across the seam
      1  K = 2: a at the end of window 0's kept frames, a blank frame first in window 1, then a again -- two characters
      2  K = 2: b is arg-max only in frames the seam drops (both sides) and in window 0's discarded frames -- it must not appear
      3  K = 3: all blank
      4  K = 2: exact ties: a and b equal and largest in the frames around the seam -- the first maximum (a) wins, one run
      5  K = 1: a, blank, b inside one ordinary crop
      6  K = 3: a run of a across both seams, b dropped in every overlap
    Returns logits, counts and the expected label lists."""
    f, blank, a, b = overlap // 8, classes - 1, 3, 5
    counts = [2, 2, 2, 3, 2, 1, 3]
    lg = np.full((sum(counts), 50, classes), -4.0, F32)
    lg[:, :, blank] = 4.0
    rng = np.random.default_rng(overlap * 10 + discard)
    lg += rng.normal(0, 0.05, lg.shape).astype(F32)  # no accidental ties

    def put(win, frames, cls, value=8.0):
        lg[win, frames, cls] = value

    hi, lo = 50 - f, f
    put(0, slice(hi - 2, hi), a), put(1, slice(lo, lo + 2), a)                              # word 0
    put(2, slice(hi - 2, hi), a), put(3, slice(lo + 1, lo + 3), a)                          # word 1 (frame lo of window 3 stays blank)
    put(4, slice(hi, 50), b), put(5, slice(0, lo), b), put(4, slice(0, discard), b)        # word 2
    for win in (9, 10):                                                                     # word 4
        fr = slice(hi - 1, hi) if win == 9 else slice(lo, lo + 1)
        lg[win, fr, a] = 8.0
        lg[win, fr, b] = 8.0
    put(11, slice(10, 12), a), put(11, slice(20, 23), b)                                    # word 5
    put(12, slice(hi - 3, 50), a), put(13, slice(0, 50), a), put(14, slice(0, lo + 3), a)  # word 6 ...
    put(12, slice(hi, 50), b, 9.0), put(13, slice(0, lo), b, 9.0), put(13, slice(hi, 50), b, 9.0), put(14, slice(0, lo), b, 9.0)
    expect = [[a], [a, a], [], [], [a], [a, b], [a]]
    return lg, np.array(counts, np.int32), expect


# ---- the workspace table of the windowed entry points ------------------------------------------------------------------
# What tests/workspace_cases.py is for the functions of include/kocr.h, for those of include/kocr_windows.h: one row per call of
# an entry point that takes memory from the context's bump arenas, at the smallest shapes that take each allocation path;
# tests/test_windows_abi_cpu.py holds the table against the header and the sources, tests/test_windows_gpu.py runs every row
# on a cold context with arena guards.  A row: name, entry (the extern "C" function), method (the Context method), args (a
# zero-argument callable), touches (arenas the call must have reserved).
NO_ARENA = ("kocr_windowed_results_shape", "kocr_windowed_results")  # copies out of what a row's call left


def _edge_boxes():
    return np.stack([long_box(4 + 10 * i) for i in range(26)])


def workspace_rows():
    one = np.zeros((0, 4, 2), F32)
    return [
        {"name": "window_plan", "entry": "kocr_window_plan", "method": "window_plan", "args": lambda: (PLAN_BOXES,), "touches": ("io",)},
        {"name": "window_plan-330_boxes", "entry": "kocr_window_plan", "method": "window_plan",
         "args": lambda: (np.concatenate([PLAN_BOXES] * 30),), "touches": ("io",)},
        {"name": "warp_crops_windowed", "entry": "kocr_warp_crops_windowed", "method": "warp_crops_windowed",
         "args": lambda: (np.stack([page(), page()]), [PLAN_BOXES[:6], PLAN_BOXES[6:]]), "touches": ("io",)},
        {"name": "warp_crops_windowed-page_without_boxes", "entry": "kocr_warp_crops_windowed", "method": "warp_crops_windowed",
         "args": lambda: (np.stack([page(), page()]), [one, PLAN_BOXES[:4]]), "touches": ("io",)},
        {"name": "ctc_stitch_decode", "entry": "kocr_ctc_stitch_decode", "method": "ctc_stitch_decode",
         "args": lambda: (random_logits(np.random.default_rng(1), 50, 37), [1, 41, 5, 3]), "touches": ("io",)},
        {"name": "recognize_boxes_windowed", "entry": "kocr_recognize_boxes_windowed", "method": "recognize_boxes_windowed",
         "args": lambda: (np.stack([page(), page()]), [PLAN_BOXES[:6], PLAN_BOXES[6:]]), "touches": ("io", "ws")},
        {"name": "recognize_boxes_windowed-one_short_box", "entry": "kocr_recognize_boxes_windowed", "method": "recognize_boxes_windowed",
         "args": lambda: (page()[None], [PLAN_BOXES[:1]]), "touches": ("io", "ws")},
        {"name": "recognize_boxes_windowed-two_batches", "entry": "kocr_recognize_boxes_windowed", "method": "recognize_boxes_windowed",
         "args": lambda: (page(270, 1700, seed=11)[None], [_edge_boxes()]), "touches": ("io", "ws")},
    ]
