"""The detector-target statement of DESIGN.md section 4: ``tools.fix_line`` and ``detection.compute_maps``
(reference detection.py:106-198, tools.py:584-600) in numpy, built on oracle/tools.py's restatement of cv2.

Every warp covers the FULL map, as the reference's ``cv2.warpPerspective`` calls do; the GPU (warp.hip,
``kocr_compute_maps``) only visits a bounding box per quad and is held to this statement bit for bit.

Rules (each pinned by tests/golden/maps_golden.npz, generated from the reference's own code, except where marked):

* ``fix_line``: the centre of a rotated box is ``box.mean(axis=0)`` in float32, i.e. ``((p0 + p1) + p2) + p3`` then
  ``/ 4``.  The line is vertical iff ``np.diff(cy_sorted).sum() > np.diff(cx_sorted).sum()``, both sums float32 in
  numpy's pairwise order (``pairwise_sum_f32``).  Ties in the ordering break by the character's index (a stable sort);
  numpy's default sort is not stable, so equal centres may be ordered differently there (a stated deviation).
* per character (after ordering): the clamp ``max(v, 0)``; the character quad is the clamped rotated box ``/ 2`` in
  float32; ``xc = (((x1 + x2) + x3) + x4) / 4`` and ``yc = (((y4 + y1) + y3) + y2) / 4``; the link endpoints are float32
  (numpy >= 2 keeps ``np.float32 op python int`` in float32; a numpy-1 run rounds once in float64: unpinned).  A ``" "``
  resets the link chain and draws nothing.  An empty line raises IndexError.
* a singular perspective system: cv2.getPerspectiveTransform returns zeros with ``M[2, 2] = 1`` and cv2.invert of it
  the zero matrix, so every map pixel samples the heat-map's (0, 0) (as we read OpenCV; unpinned).
* the maps accumulate the uint8 warps in float32 (integer sums, exact in any order) and return
  ``clip(0, 255) / 255`` float32 of shape (H / 2, W / 2, 2), text first.
"""
import numpy as np

from oracle import tools as otools

F32 = np.float32


def pairwise_sum_f32(a):
    """np.sum of a 1-D float32 array (numpy's pairwise summation): below 8 elements a sequential sum from -0.0; up to 128,
    eight strided partial sums seeded with a[0..7] combined as ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder
    in order; above 128, split at n // 2 rounded down to a multiple of 8."""
    a = np.asarray(a, F32)
    n = len(a)
    if n == 0:
        return F32(0)  # np.sum's identity
    if n < 8:
        r = F32(-0.0)
        for v in a:
            r = F32(r + v)
        return r
    if n <= 128:
        r = [F32(v) for v in a[:8]]
        i = 8
        while i < n - n % 8:
            for j in range(8):
                r[j] = F32(r[j] + a[i + j])
            i += 8
        res = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
        while i < n:
            res = F32(res + a[i])
            i += 1
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return F32(pairwise_sum_f32(a[:n2]) + pairwise_sum_f32(a[n2:]))


def box_center(box):
    """box.mean(axis=0) of a (4, 2) float32 box."""
    b = np.asarray(box, F32)
    return F32(F32(F32(b[0] + b[1]) + b[2]) + b[3]) / F32(4)


def fix_line(line):
    """tools.fix_line: [(points, character)] -> ([(rotated box float32 (4, 2), character)] in reading order,
    "horizontal" | "vertical")."""
    line = [(otools.get_rotated_box(box)[0], character) for box, character in line]
    if not line:
        raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
    centers = np.array([box_center(box) for box, _ in line], F32)
    sortedx = np.argsort(centers[:, 0], kind="stable")
    sortedy = np.argsort(centers[:, 1], kind="stable")
    dy = pairwise_sum_f32(np.diff(centers[sortedy][:, 1]))
    dx = pairwise_sum_f32(np.diff(centers[sortedx][:, 0]))
    if dy > dx:
        return [line[idx] for idx in sortedy], "vertical"
    return [line[idx] for idx in sortedx], "horizontal"


def line_quads(line):
    """The quads compute_maps draws for one line: [(character quad float32 (4, 2) or None, link quad or None)] in the
    order of fix_line (a space draws neither; the first character of a chain has no link)."""
    line, orientation = fix_line(line)
    out = []
    prev = None
    two = F32(2)
    for box, c in line:
        x1, y1, x2, y2, x3, y3, x4, y4 = [F32(0) if v < 0 else F32(v) for v in np.asarray(box, F32).reshape(8)]
        if c == " ":
            prev = None
            out.append((None, None))
            continue
        yc = F32(F32(F32(y4 + y1) + y3) + y2) / F32(4)
        xc = F32(F32(F32(x1 + x2) + x3) + x4) / F32(4)
        if orientation == "horizontal":
            cur = np.array([[(xc + (x1 + x2) / two) / two, (yc + (y1 + y2) / two) / two],
                            [(xc + (x3 + x4) / two) / two, (yc + (y3 + y4) / two) / two]], F32) / two
        else:
            cur = np.array([[(xc + (x1 + x4) / two) / two, (yc + (y1 + y4) / two) / two],
                            [(xc + (x2 + x3) / two) / two, (yc + (y2 + y3) / two) / two]], F32) / two
        char = np.array([[x1, y1], [x2, y2], [x3, y3], [x4, y4]], F32) / two
        link = None
        if prev is not None:
            if orientation == "horizontal":
                link = np.array([prev[0], cur[0], cur[1], prev[1]], F32)
            else:
                link = np.array([prev[0], prev[1], cur[1], cur[0]], F32)
        out.append((char, link))
        prev = cur
    return out


def heatmap_src(heatmap):
    return np.array([[0, 0], [heatmap.shape[1], 0], [heatmap.shape[1], heatmap.shape[0]], [0, heatmap.shape[0]]], F32)


def get_perspective_transform(src, dst):
    """cv2.getPerspectiveTransform, with OpenCV's answer to a singular system: zeros with M[2, 2] = 1."""
    try:
        return otools.get_perspective_transform(src, dst)
    except ZeroDivisionError:
        M = np.zeros((3, 3), np.float64)
        M[2, 2] = 1.0
        return M


def warp_perspective(heatmap, M, dsize):
    """cv2.warpPerspective(heatmap, M, dsize) over the whole destination (uint8, bilinear, constant 0)."""
    return otools.warp_perspective_u8(heatmap, M, dsize)


def compute_maps(heatmap, image_height, image_width, lines):
    """detection.compute_maps: (H / 2, W / 2, 2) float32, text then link."""
    assert image_height % 2 == 0, "Height must be an even number"
    assert image_width % 2 == 0, "Width must be an even number"
    h, w = image_height // 2, image_width // 2
    textmap = np.zeros((h, w), F32)
    linkmap = np.zeros((h, w), F32)
    src = heatmap_src(heatmap)
    for line in lines:
        for char, link in line_quads(line):
            if link is not None:
                linkmap += warp_perspective(heatmap, get_perspective_transform(src, link), (w, h)).astype(F32)
            if char is not None:
                textmap += warp_perspective(heatmap, get_perspective_transform(src, char), (w, h)).astype(F32)
    return np.concatenate([textmap[..., None], linkmap[..., None]], axis=2).clip(0, 255) / F32(255)


def get_gaussian_heatmap(size=512, distanceRatio=3.34):  # pylint: disable=invalid-name
    """detection.get_gaussian_heatmap (detection.py:45-53)."""
    v = np.abs(np.linspace(-size / 2, size / 2, num=size))
    x, y = np.meshgrid(v, v)
    g = np.sqrt(x**2 + y**2)
    g *= distanceRatio / (size / 2)
    g = np.exp(-(1 / 2) * (g**2))
    g *= 255
    return g.clip(0, 255).astype("uint8")


def mse_loss_f64(y_true, y_pred, sample_weight=None):
    """Keras' compiled mse as evaluate reports it, in float64: per pixel the mean over the two
    channels of (y - y_hat)^2, per image the sum over pixels, weighted by sample_weight, divided by N * h * w."""
    y = np.asarray(y_true, np.float64)
    p = np.asarray(y_pred, np.float64)
    per_image = (((y - p) ** 2).mean(-1)).reshape(len(y), -1).sum(1)
    sw = np.ones(len(y)) if sample_weight is None else np.asarray(sample_weight, np.float64).reshape(len(y))
    return float((sw * per_image).sum() / (y.shape[0] * y.shape[1] * y.shape[2]))


def one_leaf_sum_f32(a):
    """The 8 <= n <= 128 rule of pairwise_sum_f32 applied to the whole array without the split: what a summation that never
    splits gives.  Equal to pairwise_sum_f32 up to 128 elements."""
    a = np.asarray(a, F32)
    n = len(a)
    if n <= 128:
        return pairwise_sum_f32(a)
    r = [F32(v) for v in a[:8]]
    i = 8
    while i < n - n % 8:
        for j in range(8):
            r[j] = F32(r[j] + a[i + j])
        i += 8
    res = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
    while i < n:
        res = F32(res + a[i])
        i += 1
    return res


def tie_line(seed, n, pitch=(3, 9), jitter=0.3):
    """A diagonal line of n axis-aligned characters whose x and y spans are equal in real arithmetic: the orientation
    comes down to float32 rounding, and for some seeds numpy's pairwise order and a plain left-to-right sum disagree.
    ``pitch`` is the range of the step between characters, ``jitter`` the half-range of y - x; a small pitch lets a long
    line fit a small map (the jitter has to stay below half the smallest pitch for the line to arrive sorted)."""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.uniform(pitch[0], pitch[1], n))
    y = x + rng.uniform(-jitter, jitter, n)
    y[-1] = y[0] + (x[-1] - x[0])
    line = []
    for i in range(n):
        cx, cy = x[i] + 40.123, y[i] + 17.77
        line.append((np.array([[cx - 1.5, cy - 2], [cx + 1.5, cy - 2], [cx + 1.5, cy + 2], [cx - 1.5, cy + 2]], F32), "ab"[i % 2]))
    return line


TIE_SEEDS = ((11, 20), (13, 22), (16, 25), (20, 29))  # (seed, n): lines on which the two summation orders disagree

# Long tie lines: tie_line(seed, n, LONG_TIE_PITCH, LONG_TIE_JITTER) on a LONG_TIE_HW input (a 166 x 166 map).  n - 1
# differences are summed: 64 (one stride past a wave of characters), 128 (the last leaf), 129 (the first split), 257 (the
# first second-level split: 257 -> 128 + 129 -> 128 + (64 + 65)) and 299.
LONG_TIE_PITCH = (0.5, 1.5)
LONG_TIE_JITTER = 0.1
LONG_TIE_HW = (332, 332)
# (seed, n): for every n the first seed of range(400) on which numpy's pairwise order and a left-to-right sum decide the
# orientation differently and, from n = 130 on, the pairwise order and one_leaf_sum_f32 do too
LONG_TIE_SEEDS = ((13, 65), (0, 129), (1, 130), (23, 258), (2, 300))


def long_tie_line(seed, n):
    return tie_line(seed, n, LONG_TIE_PITCH, LONG_TIE_JITTER)


LONG_PAGE_HW = (148, 148)


def long_lines_page():
    """A page of four lines of 64, 65, 129 and 130 characters whose characters arrive in a scrambled order.  Returns
    ``(lines, expected)``: ``lines`` as compute_maps takes them, ``expected`` per line ``([(box, character)] in reading order,
    orientation)``.  All coordinates are multiples of 1 / 8, so every centre is exact in float32.

    * lines 1 and 3 are vertical (the 130-character one leans 1 : 2.5), lines 0 and 2 horizontal;
    * spaces sit inside every line, one at ordered position 63 of line 1 and one at position 64 of lines 2 and 3;
    * line 2 holds a character and a space on one centre, the character first (input indices 10 and 100); line 3 a space and
      a character on one centre, the space first (input indices 20 and 70): the index decides which of the two the link
      chain reaches, and the two indices lie on different sides of 64;
    * the input order of every line is a permutation with a fixed seed."""
    rng = np.random.default_rng(2025)
    letters = "abcdefghijklmnopqrstuvwxyz"

    def box(cx, cy, w, h):
        return np.array([[cx - w / 2, cy - h / 2], [cx + w / 2, cy - h / 2], [cx + w / 2, cy + h / 2], [cx - w / 2, cy + h / 2]], F32)

    # (n, vertical, start along, start across, lean across per step, spaces at ordered positions, twin (first, second, slots))
    specs = [(64, False, 6.0, 8.0, 0.0, (20, 41), None),
             (65, True, 30.0, 14.0, 0.0, (7, 63), None),
             (129, False, 5.0, 24.0, 0.125, (30, 64, 90), (50, "char", (10, 100))),
             (130, True, 4.0, 62.0, 0.375, (12, 64, 101), (77, "space", (20, 70)))]
    lines, expected = [], []
    for n, vertical, along0, across0, lean, spaces, twin in specs:
        ordered = []
        along = along0
        for k in range(n):
            if twin is not None and k == twin[0] + 1:
                # the twin of the character before: the same box, so the same centre
                ordered.append((ordered[-1][0].copy(), " " if twin[1] == "char" else letters[k % 26]))
                continue
            along += float(rng.integers(7, 10)) / 8.0  # a step of 0.875, 1 or 1.125
            across = across0 + lean * k + float(rng.integers(0, 5)) / 8.0
            cx, cy = (across, along) if vertical else (along, across)
            ordered.append((box(cx, cy, 3.0, 4.5) if not vertical else box(cx, cy, 4.5, 3.0), " " if k in spaces else letters[k % 26]))
        if twin is not None and twin[1] == "space":
            ordered[twin[0]] = (ordered[twin[0]][0], " ")
        order = [int(v) for v in rng.permutation(n)]  # order[slot] = ordered position of the character given at input slot
        if twin is not None:
            for member, slot in zip((twin[0], twin[0] + 1), twin[2]):
                at = order.index(member)
                order[at], order[slot] = order[slot], order[at]
        lines.append([ordered[k] for k in order])
        expected.append((ordered, "vertical" if vertical else "horizontal"))
    return lines, expected
