"""Generate tests/golden/maps_golden.npz by EXECUTING THE REFERENCE's detector-target code.

Run in the build container (where /root/reference exists):  python tests/golden/make_golden_maps.py

Calls the reference's ``detection.compute_maps`` (detection.py:106-198), ``get_gaussian_heatmap`` (:55-62),
``compute_input`` (:34-42), ``invert_input`` (:45-52), ``map_to_rgb`` (:201-204) and ``tools.fix_line``
(tools.py:584-600) through make_golden.install_stubs(), with three stand-ins replaced afterwards:

  * ``cv2.getPerspectiveTransform`` / ``cv2.warpPerspective``: the statement's functions (tests/maps_statement.py, on
    oracle/tools.py's restatement of cv2, cross-checked there);
  * shapely ``MultiPoint.minimum_rotated_rectangle``: oracle.tools.min_rotated_rect_f64 (AttributeError on degenerate
    input, as shapely's LineString / Point have no ``exterior``).

Everything else -- the ordering and orientation of fix_line, the clamp, the half-scale quads, the link endpoints, the
link chain and its reset at spaces, the accumulation and the final clip / 255 -- is the reference's code.

A case is only ever appended: the arrays the file already holds are checked to stay byte for byte before it is rewritten.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden  # noqa: E402
from oracle import tools as otools  # noqa: E402
from tests import maps_statement as ms  # noqa: E402


def install():
    make_golden.install_stubs()
    cv2 = sys.modules["cv2"]
    cv2.getPerspectiveTransform = lambda src, dst: ms.get_perspective_transform(src, dst)
    cv2.warpPerspective = lambda image, M, dsize, **kw: ms.warp_perspective(image, M, dsize)

    class _Ring:
        def __init__(self, pts):
            closed = np.concatenate([pts, pts[:1]])
            self.xy = (list(closed[:, 0]), list(closed[:, 1]))

    class _Rect:
        def __init__(self, pts):
            self.exterior = _Ring(pts)

    class MultiPoint:  # noqa
        def __init__(self, points=None):
            self._points = np.asarray(points)

        @property
        def minimum_rotated_rectangle(self):
            return _Rect(otools.min_rotated_rect_f64(self._points))  # AttributeError when degenerate

    sys.modules["shapely.geometry"].MultiPoint = MultiPoint


def rect(x, y, w, h, angle=0.0):
    c, s = np.cos(angle), np.sin(angle)
    pts = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
    return (pts @ np.array([[c, s], [-s, c]]) + [x, y]).astype(np.float32)


def word(x, y, text, cw=9.0, ch=12.0, gap=1.5, angle=0.0, vertical=False):
    """Characters of a word along a direction; returns [(box, character)]."""
    c, s = np.cos(angle), np.sin(angle)
    out = []
    for i, t in enumerate(text):
        d = i * ((ch if vertical else cw) + gap)
        ox, oy = (x - s * d, y + c * d) if vertical else (x + c * d, y + s * d)
        out.append((rect(ox, oy, cw, ch, angle), t))
    return out


def cases():
    rng = np.random.default_rng(11)
    pages = []
    # 1: horizontal words, a space, a line reaching past the top-left corner
    pages.append((64, 96, [word(4, 6, "ab c"), word(-5, -3, "xyz", cw=8, ch=10)]))
    # 2: a vertical line, a rotated line; W / 2 odd
    pages.append((80, 90, [word(70, 4, "tall", cw=10, ch=9, vertical=True), word(8, 30, "rot", angle=0.35)]))
    # 3: perspective (jittered) characters, a vertical rotated line, a degenerate (collinear) character, a duplicate box
    jit = [(b + rng.uniform(-1.5, 1.5, (4, 2)).astype(np.float32), c) for b, c in word(10, 50, "persp", cw=11, ch=14)]
    degenerate = [(np.array([[20, 20], [30, 20], [40, 20], [25, 20]], np.float32), "d")]
    dup = word(60, 10, "qq", cw=7, ch=7)
    dup = [dup[0], (dup[0][0].copy(), "r"), dup[1]]
    pages.append((96, 128, [jit, word(100, 30, "vrt", angle=-0.3, vertical=True) + degenerate, dup]))
    # 4: one character per line, a line of one space, a single-point character, a quad larger than the page
    pages.append((48, 64, [[(rect(10, 10, 6, 8), "a")], [(rect(20, 20, 6, 6), " ")],
                           [(np.full((4, 2), 17.0, np.float32), "p")], [(rect(-40, -30, 150, 120, 0.2), "B")]]))
    # 5: no lines
    pages.append((32, 48, []))
    # 6: a 258-character diagonal line whose orientation comes down to the order of numpy's float32 sum (257 differences:
    # split twice), and a short line
    seed, n = ms.LONG_TIE_SEEDS[3]
    assert n == 258
    pages.append((300, 300, [ms.long_tie_line(seed, n), word(200, 40, "short", cw=8, ch=11)]))
    return pages


def main():
    install()
    from keras_ocr import detection, tools  # the reference's modules  # noqa: E402

    out = {}
    heatmaps = [detection.get_gaussian_heatmap(size=512, distanceRatio=1.5),
                detection.get_gaussian_heatmap(size=33, distanceRatio=2.5)]
    out["heatmap_args"] = np.array([[512, 1.5], [33, 2.5]])
    for k, hm in enumerate(heatmaps):
        out[f"heatmap{k}"] = hm
    for i, (H, W, lines) in enumerate(cases()):
        quads = [b for line in lines for b, _ in line]
        out[f"case{i}_hw"] = np.array([H, W], np.int32)
        out[f"case{i}_quads"] = np.array(quads, np.float32).reshape(-1, 4, 2)
        out[f"case{i}_chars"] = np.array([c for line in lines for _, c in line], dtype="<U1")
        out[f"case{i}_offsets"] = np.cumsum([0] + [len(line) for line in lines]).astype(np.int32)
        fixed, orient = [], []
        for line in lines:
            fl, o = tools.fix_line(line)
            fixed += [b for b, _ in fl]
            orient.append(o == "vertical")
            assert [c for _, c in fl] == [c for _, c in ms.fix_line(line)[0]]
        out[f"case{i}_fixed"] = np.array(fixed, np.float32).reshape(-1, 4, 2)
        out[f"case{i}_vertical"] = np.array(orient, bool)
        for k, hm in enumerate(heatmaps):
            out[f"case{i}_maps{k}"] = detection.compute_maps(heatmap=hm, image_height=H, image_width=W, lines=lines)
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (2, 6, 5, 3), dtype=np.uint8)
    out["input_img"] = img
    out["input_x"] = detection.compute_input(img)
    out["input_inv"] = detection.invert_input(out["input_x"])
    out["rgb_in"] = out["case1_maps0"]
    out["rgb_out"] = detection.map_to_rgb(out["case1_maps0"])
    path = os.path.join(HERE, "maps_golden.npz")
    if os.path.exists(path):  # a case is only ever appended: what the file holds already stays byte for byte
        old = dict(np.load(path))
        for key, value in old.items():
            assert key in out and out[key].dtype == value.dtype and out[key].shape == value.shape, key
            assert out[key].tobytes() == value.tobytes(), key
        print("kept", len(old), "arrays; new:", sorted(set(out) - set(old)))
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
