"""The rule keras_ocr_amd/csrc/lines.hip implements (kocr_group_lines), stated in numpy float64 with every operation in a
fixed order: IEEE `+ - * / sqrt` one at a time (numpy's elementwise operations and Python floats never fuse a product
into a sum).  The kernel carries out the same operations in the same order, so its integers equal these and its line
boxes carry the same float32 bits (tests/test_lines_gpu.py).  DESIGN.md section 4, "Lines".

A word is a quad [p0 top-left, p1 top-right, p2 bottom-right, p3 bottom-left] of float32 (what getBoxes / adjust_boxes
produce), promoted to float64.  One function per step:

  word_records   l, r, c, a, w, h, u of every word, and which words are degenerate
  link_matrix    the four conditions for every pair, and how far the pairs that were tested stay from the thresholds
  components     the lines: connected components of the link graph, named by their smallest word index
  line_axis      the sum of the members' directions in ascending word index, normalised
  word_order     the members sorted along the axis
  line_box       the bounding rectangle along the axis, as float64 corners
  group_page     all of it for one page, the lines sorted top to bottom
"""
import math

import numpy as np

DEFAULTS = {"max_angle": 15.0, "min_height_ratio": 0.5, "max_offset": 0.5, "max_gap": 1.5}
MAX_WORDS = 2048  # per page


def cos_max_of(max_angle):
    """the direction threshold, computed once on the host and handed to the kernel as a double"""
    if not 0 <= max_angle < 90:
        raise ValueError(f"max_angle {max_angle} outside [0, 90)")
    return math.cos(math.radians(max_angle))


def _norm(x, y):
    return np.sqrt(x * x + y * y)


def word_records(quads):
    """quads float32 (n, 4, 2) -> dict of float64 arrays: c (n, 2), u (n, 2), w (n,), h (n,), and degenerate (n,) bool.
    l = (p0 + p3) * 0.5, r = (p1 + p2) * 0.5, c = (l + r) * 0.5, a = r - l, w = sqrt(a.x a.x + a.y a.y),
    h = 0.5 (|p3 - p0| + |p2 - p1|), u = a / w.  A word with w == 0 or h == 0 is degenerate: u = (1, 0)."""
    q = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2).astype(np.float64)
    p0, p1, p2, p3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    l = (p0 + p3) * 0.5
    r = (p1 + p2) * 0.5
    c = (l + r) * 0.5
    a = r - l
    w = _norm(a[:, 0], a[:, 1])
    e0, e1 = p3 - p0, p2 - p1
    h = 0.5 * (_norm(e0[:, 0], e0[:, 1]) + _norm(e1[:, 0], e1[:, 1]))
    degenerate = (w == 0) | (h == 0)
    u = np.zeros_like(a)
    u[:, 0] = 1.0
    ok = ~degenerate
    u[ok] = a[ok] / w[ok][:, None]
    return {"q": q, "c": c, "u": u, "w": w, "h": h, "degenerate": degenerate}


def _relative(lhs, rhs):
    """|lhs - rhs| relative to the larger magnitude of the two (1 where both are zero)"""
    scale = np.maximum(np.abs(lhs), np.abs(rhs))
    return np.where(scale > 0, np.abs(lhs - rhs) / np.where(scale > 0, scale, 1.0), 1.0)


def link_matrix(rec, cos_max, min_height_ratio, max_offset, max_gap, rows=256):
    """-> (link (n, n) bool, symmetric, False on the diagonal; margin): Link(a, b) for two non-degenerate words holds when
      1. u_a . u_b >= cos_max
      2. min(h_a, h_b) >= min_height_ratio * max(h_a, h_b)
      3. across <= max_offset * min(h_a, h_b)
      4. along - 0.5 * (w_a + w_b) <= max_gap * max(h_a, h_b)
    with s = u_a + u_b, m = s / |s|, d = c_b - c_a, along = |d.x m.x + d.y m.y|, across = |d.x m.y - d.y m.x|, a < b.
    3 and 4 are evaluated only where 1 holds (s cannot vanish there: cos_max > 0).  margin: the smallest relative distance
    of a tested condition's two sides over all pairs of non-degenerate words (inf without any)."""
    c, u, w, h, deg = rec["c"], rec["u"], rec["w"], rec["h"], rec["degenerate"]
    n = len(w)
    link = np.zeros((n, n), bool)
    margin = math.inf
    for a0 in range(0, n, rows):
        a = slice(a0, min(n, a0 + rows))
        ua, ca, wa, ha = u[a, None, :], c[a, None, :], w[a, None], h[a, None]
        ub, cb, wb, hb = u[None, :, :], c[None, :, :], w[None, :], h[None, :]
        tested = ~deg[a, None] & ~deg[None, :] & (np.arange(n)[None, :] > np.arange(a.start, a.stop)[:, None])
        dot = ua[..., 0] * ub[..., 0] + ua[..., 1] * ub[..., 1]
        hmin, hmax = np.minimum(ha, hb), np.maximum(ha, hb)
        c1 = dot >= cos_max
        low = min_height_ratio * hmax
        c2 = hmin >= low
        geo = tested & c1
        with np.errstate(invalid="ignore", divide="ignore"):
            sx, sy = ua[..., 0] + ub[..., 0], ua[..., 1] + ub[..., 1]
            sn = _norm(sx, sy)
            mx, my = sx / sn, sy / sn
            dx, dy = cb[..., 0] - ca[..., 0], cb[..., 1] - ca[..., 1]
            along = np.abs(dx * mx + dy * my)
            across = np.abs(dx * my - dy * mx)
            off = max_offset * hmin
            c3 = across <= off
            gap = along - 0.5 * (wa + wb)
            far = max_gap * hmax
            c4 = gap <= far
        both = tested & c1 & c2 & c3 & c4
        link[a] = both
        for lhs, rhs, where in ((dot, np.broadcast_to(cos_max, dot.shape), tested), (hmin, low, tested), (across, off, geo), (gap, far, geo)):
            if where.any():
                margin = min(margin, float(_relative(lhs[where], rhs[where]).min()))
    link |= link.T
    return link, margin


def components(link):
    """-> label (n,) int: the smallest word index of each word's connected component (linking is transitive)"""
    n = len(link)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in np.argwhere(np.triu(link, 1)).tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], dtype=np.int64)


def line_axis(rec, members):
    """A = sum of the members' u, added from (0, 0) in ascending word index; -> A / |A| as two Python floats.  A line of
    one degenerate word has u = (1, 0) and so the axis (1, 0); a sum of zero length (directions that turn by half a circle
    along a chain) also gives (1, 0)."""
    ax, ay = 0.0, 0.0
    for j in sorted(members):
        ax = ax + float(rec["u"][j, 0])
        ay = ay + float(rec["u"][j, 1])
    norm = math.sqrt(ax * ax + ay * ay)
    if norm == 0:
        return 1.0, 0.0
    return ax / norm, ay / norm


def word_order(rec, members, axis):
    """the members by t = c.x A.x + c.y A.y ascending, ties by word index"""
    c = rec["c"]
    return sorted(members, key=lambda j: (float(c[j, 0]) * axis[0] + float(c[j, 1]) * axis[1], j))


def line_box(rec, members, axis):
    """V = (-A.y, A.x); t0, t1 = min, max of p . A and s0, s1 of p . V over the four corners of all members; -> float64
    (4, 2): tl = t0 A + s0 V, tr = t1 A + s0 V, br = t1 A + s1 V, bl = t0 A + s1 V"""
    ax, ay = axis
    vx, vy = -ay, ax
    p = rec["q"][sorted(members)].reshape(-1, 2)
    t = p[:, 0] * ax + p[:, 1] * ay
    s = p[:, 0] * vx + p[:, 1] * vy
    t0, t1, s0, s1 = float(t.min()), float(t.max()), float(s.min()), float(s.max())
    return np.array([[t0 * ax + s0 * vx, t0 * ay + s0 * vy], [t1 * ax + s0 * vx, t1 * ay + s0 * vy],
                     [t1 * ax + s1 * vx, t1 * ay + s1 * vy], [t0 * ax + s1 * vx, t0 * ay + s1 * vy]], dtype=np.float64)


def group_page(quads, max_angle=15.0, min_height_ratio=0.5, max_offset=0.5, max_gap=1.5, cos_max=None):
    """One page: quads float32 (n, 4, 2) -> dict with
      line_of  (n,) int32   the page-order index of each word's line
      order    (n,) int32   the word indices in reading order: line 0's words, then line 1's, ...
      lines    list of lists: the word indices of each line, in order
      boxes    (L, 4, 2) float32  the line boxes, rounded from float64
      margin   see link_matrix
    Lines are ordered by the y of the float64 box centre (tl + br) * 0.5, then its x, then the smallest member index."""
    quads = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)
    n = len(quads)
    if n > MAX_WORDS:
        raise ValueError(f"{n} words on a page, more than {MAX_WORDS}")
    if not np.isfinite(quads).all():
        raise ValueError("non-finite coordinate")
    cos_max = cos_max_of(max_angle) if cos_max is None else cos_max
    rec = word_records(quads)
    link, margin = link_matrix(rec, cos_max, min_height_ratio, max_offset, max_gap)
    label = components(link)
    found = []
    for root in np.flatnonzero(label == np.arange(n)).tolist():
        members = np.flatnonzero(label == root).tolist()
        axis = line_axis(rec, members)
        box = line_box(rec, members, axis)
        cx, cy = (box[0, 0] + box[2, 0]) * 0.5, (box[0, 1] + box[2, 1]) * 0.5
        found.append(((float(cy), float(cx), root), word_order(rec, members, axis), box))
    found.sort(key=lambda item: item[0])
    line_of = np.zeros(n, np.int32)
    for k, (_, words, _) in enumerate(found):
        line_of[words] = k
    return {"line_of": line_of, "order": np.array([j for _, words, _ in found for j in words], dtype=np.int32).reshape(-1),
            "lines": [words for _, words, _ in found], "margin": margin,
            "boxes": np.array([box for _, _, box in found], dtype=np.float64).reshape(-1, 4, 2).astype(np.float32)}


def group_batch(pages, **rule):
    """pages: list of (n_i, 4, 2) -> (line_of (total,), order (total,), line_counts (N,), boxes (lines, 4, 2), margin): the
    arrays kocr_group_lines returns for the batch"""
    results = [group_page(p, **rule) for p in pages]
    cat = lambda key, dtype, tail: (np.concatenate([r[key] for r in results]) if results else np.zeros((0,) + tail, dtype)).astype(dtype)  # noqa: E731
    return (cat("line_of", np.int32, ()), cat("order", np.int32, ()), np.array([len(r["lines"]) for r in results], np.int32),
            cat("boxes", np.float32, (4, 2)), min([r["margin"] for r in results], default=math.inf))
