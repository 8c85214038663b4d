"""The statement of kocr_char_boxes ("Characters"): the characters of a word box, read off the
detector's region map.  The reference has no counterpart, so this file IS the definition; csrc/chars.hip follows it
operation by operation in float64 (compiled without fused multiply-adds), so its integers equal these and its float32
outputs carry these bits.

Every float64 operation stands alone on its line or is parenthesised the way the kernel evaluates it: a sum of two products
is ``x * x + y * y`` (two roundings of the products, one of the sum), a length is ``sqrt`` of that and never ``hypot``.

A text map ``T`` is (h, w) float32, channel 0 of one page's heat-map; pixel centres sit at integer coordinates.  A word is a
quad [tl, tr, br, bl] in float32 detector-input pixels (heat-map pixels x 2), as ``getBoxes`` returns it."""
import math

import numpy as np

MAX_COLS = 512
MAX_ROWS = 32
DEFAULTS = {"peak_threshold": 0.4, "valley_ratio": 0.7, "extent_threshold": 0.2}


def check_rule(peak_threshold=0.4, valley_ratio=0.7, extent_threshold=0.2):
    """The three parameters as floats, or ValueError naming the one out of range: all finite, 0 < peak_threshold,
    0 <= valley_ratio <= 1, 0 <= extent_threshold <= peak_threshold."""
    p, r, e = float(peak_threshold), float(valley_ratio), float(extent_threshold)
    if not (math.isfinite(p) and p > 0):
        raise ValueError(f"peak_threshold {p} is not a finite number > 0")
    if not 0 <= r <= 1:
        raise ValueError(f"valley_ratio {r} outside [0, 1]")
    if not 0 <= e <= p:
        raise ValueError(f"extent_threshold {e} outside [0, peak_threshold = {p}]")
    return p, r, e


def _length(dx, dy):
    return math.sqrt(dx * dx + dy * dy)


def _lerp(p, q, t):
    """p + (q - p) t, per coordinate"""
    return (p[0] + (q[0] - p[0]) * t, p[1] + (q[1] - p[1]) * t)


def half_quad(quad):
    """the quad in heat-map coordinates, float64: four (x, y) tuples tl, tr, br, bl"""
    q = np.asarray(quad, dtype=np.float32).reshape(4, 2).astype(np.float64)
    return [(float(q[c, 0]) / 2.0, float(q[c, 1]) / 2.0) for c in range(4)]


def grid(quad):
    """(n_cols, n_rows) of the word's sampling grid, or None for a word without width or height"""
    tl, tr, br, bl = half_quad(quad)
    wq = (_length(tr[0] - tl[0], tr[1] - tl[1]) + _length(br[0] - bl[0], br[1] - bl[1])) * 0.5
    hq = (_length(bl[0] - tl[0], bl[1] - tl[1]) + _length(br[0] - tr[0], br[1] - tr[1])) * 0.5
    if not wq > 0 or not hq > 0:
        return None
    n_cols = int(min(float(MAX_COLS), max(1.0, math.ceil(wq))))
    n_rows = int(min(float(MAX_ROWS), max(1.0, math.ceil(hq))))
    return n_cols, n_rows


def sample(text_map, px, py):
    """bilinear interpolation of the map at (px, py): the four pixels around (floor x, floor y), horizontally first; a pixel
    outside the map counts as 0"""
    h, w = text_map.shape
    x0, y0 = math.floor(px), math.floor(py)
    if not (-1 <= x0 <= w - 1 and -1 <= y0 <= h - 1):
        return 0.0
    x0, y0 = int(x0), int(y0)
    fx, fy = px - x0, py - y0

    def pixel(y, x):
        return float(text_map[y, x]) if 0 <= x < w and 0 <= y < h else 0.0

    t00, t01, t10, t11 = pixel(y0, x0), pixel(y0, x0 + 1), pixel(y0 + 1, x0), pixel(y0 + 1, x0 + 1)
    top = t00 + (t01 - t00) * fx
    bottom = t10 + (t11 - t10) * fx
    return top + (bottom - top) * fy


def profile(text_map, quad):
    """the word's profile: per column the maximum over the rows of the sampled map; None without a grid"""
    cells = grid(quad)
    if cells is None:
        return None
    n_cols, n_rows = cells
    tl, tr, br, bl = half_quad(quad)
    out = []
    for i in range(n_cols):
        u = (i + 0.5) / n_cols
        a, b = _lerp(tl, tr, u), _lerp(bl, br, u)
        best = None
        for j in range(n_rows):
            v = (j + 0.5) / n_rows
            p = _lerp(a, b, v)
            s = sample(text_map, p[0], p[1])
            if best is None or s > best:
                best = s
        out.append(best)
    return out


def split(prof, peak_threshold, valley_ratio, extent_threshold):
    """(bounds, peaks) of a profile: K peak columns and the K + 1 column bounds of their characters; ([], []) without any"""
    n = len(prof)
    reach = [i for i in range(n) if prof[i] >= extent_threshold]
    if not reach:
        return [], []
    first, last = reach[0], reach[-1]
    peaks, cuts = [], []
    c, low, low_at = -1, 0.0, -1
    for i in range(first, last + 1):
        here = prof[i]
        if c >= 0 and here < low:  # the running minimum since c; a tie keeps the first position
            low, low_at = here, i
        left = prof[i - 1] if i - 1 >= 0 else -1.0
        right = prof[i + 1] if i + 1 < n else -1.0
        if not (here >= peak_threshold and here > left and here >= right):
            continue
        if c < 0:
            c, low, low_at = i, here, i
        elif low <= valley_ratio * min(prof[c], here):
            peaks.append(c)
            cuts.append(low_at)
            c, low, low_at = i, here, i
        elif here > prof[c]:
            c, low, low_at = i, here, i
    if c < 0:
        return [], []
    peaks.append(c)
    return [first] + cuts + [last + 1], peaks


def word_chars(text_map, quad, peak_threshold=0.4, valley_ratio=0.7, extent_threshold=0.2):
    """One word: ``{"boxes": (K, 4, 2) float32, "scores": (K,) float32, "bounds": [...], "peaks": [...], "n_cols", "n_rows",
    "profile"}``; K = 0 for a word without characters."""
    peak_threshold, valley_ratio, extent_threshold = check_rule(peak_threshold, valley_ratio, extent_threshold)
    text_map = np.asarray(text_map, dtype=np.float32)
    cells = grid(quad)
    none = {"boxes": np.zeros((0, 4, 2), np.float32), "scores": np.zeros(0, np.float32), "bounds": [], "peaks": [], "n_cols": 0,
            "n_rows": 0, "profile": []}
    if cells is None:
        return none
    prof = profile(text_map, quad)
    bounds, peaks = split(prof, peak_threshold, valley_ratio, extent_threshold)
    none.update(n_cols=cells[0], n_rows=cells[1], profile=prof)
    if not peaks:
        return none
    n_cols = cells[0]
    tl, tr, br, bl = half_quad(quad)
    boxes = np.zeros((len(peaks), 4, 2), np.float32)
    for k in range(len(peaks)):
        u0, u1 = bounds[k] / n_cols, bounds[k + 1] / n_cols
        corners = (_lerp(tl, tr, u0), _lerp(tl, tr, u1), _lerp(bl, br, u1), _lerp(bl, br, u0))
        with np.errstate(over="ignore"):
            boxes[k] = [[np.float32(x * 2.0), np.float32(y * 2.0)] for x, y in corners]
    with np.errstate(over="ignore"):
        scores = np.array([np.float32(prof[p]) for p in peaks], np.float32)
    return {"boxes": boxes, "scores": scores, "bounds": bounds, "peaks": peaks, "n_cols": cells[0], "n_rows": cells[1], "profile": prof}


def char_batch(heat, pages, **rule):
    """A batch: ``heat`` (N, h, w, 2) float32, ``pages`` a list of (n_i, 4, 2) quads.  Returns ``(char_counts int32 (total,),
    char_quads float32 (chars, 4, 2), char_scores float32 (chars,))`` -- all characters of all words in word order."""
    heat = np.asarray(heat, dtype=np.float32)
    counts, boxes, scores = [], [np.zeros((0, 4, 2), np.float32)], [np.zeros(0, np.float32)]
    for i, page in enumerate(pages):
        for quad in np.asarray(page, dtype=np.float32).reshape(-1, 4, 2):
            got = word_chars(heat[i, :, :, 0], quad, **rule)
            counts.append(len(got["peaks"]))
            boxes.append(got["boxes"])
            scores.append(got["scores"])
    return np.array(counts, np.int32), np.concatenate(boxes), np.concatenate(scores)
