"""The rule of kocr_group_lines with flags == KOCR_LINES_BLOCKS | KOCR_LINES_DESKEW (blocks_axis_kernel, blocks_frame_kernel
and blocks_unframe_kernel in keras_ocr_amd/csrc/blocks.hip), stated in numpy / Python float64 with every operation in a fixed
order, one IEEE operation at a time: the text direction of a page from its own quads, the XY-cut of tests/blocks_statement.py
in that frame, and the block boxes back on the page as rotated rectangles.  The kernels carry out the same operations, so
their integers equal these and their boxes carry the same float32 bits (tests/test_deskew_gpu.py).  DESIGN.md section 4,
"Rotated pages".

Every operation is + - * / or a square root, all correctly rounded on both sides; no angle is ever formed.  One function
per step:

  directions    u = a / w and w of every quad ("Lines" per-word arithmetic); a quad with w == 0 has no direction
  medoid_costs  c_k = the sum over j, in ascending j, of w_j * |u_k - u_j| for every quad with a direction
  page_axis     A = u_k of the smallest (c_k, k); (1, 0) on a page without any direction
  to_frame      every corner in the frame (A, V), V = (-A.y, A.x), rounded to float32
  from_frame    a frame box (X0, Y0, X1, Y1) as the rectangle tl, tr, br, bl on the page, rounded to float32
  blocks_page   all of it for one page
  group_batch   the arrays kocr_group_lines returns for a batch

The chord |u_k - u_j| grows with the angle between the two directions all the way from 0 to 180 degrees, so an upside-down
page gets its own axis; it is a metric, so the medoid is a median and not a mean, and a minority of short, near-square quads
whose rectangle came out turned by 90 degrees does not pull it; the weights are the quads' lengths, the long ones being the
reliable ones.
"""
import numpy as np

from tests import blocks_statement as bs

F32, F64 = np.float32, np.float64


def directions(quads):
    """quads float32 (n, 4, 2) [tl, tr, br, bl] -> (u float64 (n, 2), w float64 (n,)): l = (p0 + p3) * 0.5, r = (p1 + p2) * 0.5,
    a = r - l, w = sqrt(a.x * a.x + a.y * a.y), u = a / w; u = (1, 0) where w == 0 (never read: such a quad has no direction)"""
    q = np.asarray(quads, dtype=F32).reshape(-1, 4, 2).astype(F64)
    l = (q[:, 0] + q[:, 3]) * 0.5
    r = (q[:, 1] + q[:, 2]) * 0.5
    a = r - l
    w = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1])
    u = np.zeros_like(a)
    u[:, 0] = 1.0
    have = w > 0
    u[have] = a[have] / w[have][:, None]
    return u, w


def medoid_costs(u, w):
    """-> c float64 (n,): for every k with w_k > 0, c_k = 0.0 and then, for j ascending over the quads with w_j > 0 (j == k
    included), dx = u_k.x - u_j.x, dy = u_k.y - u_j.y, c_k = c_k + w_j * sqrt(dx * dx + dy * dy); +inf where w_k == 0.  (All
    k at once for one j: the elementwise numpy operations are the scalar ones.)"""
    c = np.zeros(len(w), F64)
    for j in np.flatnonzero(w > 0).tolist():
        dx = u[:, 0] - u[j, 0]
        dy = u[:, 1] - u[j, 1]
        c = c + w[j] * np.sqrt(dx * dx + dy * dy)
    c[~(w > 0)] = np.inf
    return c


def page_axis(quads):
    """-> dict: axis (A.x, A.y) as Python floats, medoid (the k it is the direction of, or None), best and second (the
    smallest and the second smallest cost among the candidates; None where there is no such candidate), u, w"""
    u, w = directions(quads)
    c = medoid_costs(u, w)
    candidates = np.flatnonzero(w > 0)
    if candidates.size == 0:
        return {"axis": (1.0, 0.0), "medoid": None, "best": None, "second": None, "u": u, "w": w}
    k = int(candidates[np.argmin(c[candidates])])  # argmin: the first of equal ones
    ranked = np.sort(c[candidates])
    return {"axis": (float(u[k, 0]), float(u[k, 1])), "medoid": k, "best": float(ranked[0]),
            "second": float(ranked[1]) if ranked.size > 1 else None, "u": u, "w": w}


def to_frame(quads, axis):
    """x' = p.x * A.x + p.y * A.y, y' = p.x * V.x + p.y * V.y with V = (-A.y, A.x), float64 of float32, each rounded to float32"""
    q = np.asarray(quads, dtype=F32).reshape(-1, 4, 2).astype(F64)
    ax, ay = F64(axis[0]), F64(axis[1])
    vx, vy = -ay, ax
    out = np.zeros(q.shape, F32)
    out[:, :, 0] = (q[:, :, 0] * ax + q[:, :, 1] * ay).astype(F32)
    out[:, :, 1] = (q[:, :, 0] * vx + q[:, :, 1] * vy).astype(F32)
    return out


def from_frame(frame_boxes, axis):
    """frame_boxes float32 (B, 4, 2) as blocks_statement writes them, [(X0, Y0), (X1, Y0), (X1, Y1), (X0, Y1)] -> float32
    (B, 4, 2): tl = X0 A + Y0 V, tr = X1 A + Y0 V, br = X1 A + Y1 V, bl = X0 A + Y1 V, every coordinate a * b + c * d in
    that order in float64, rounded to float32"""
    b = np.asarray(frame_boxes, dtype=F32).reshape(-1, 4, 2).astype(F64)
    ax, ay = F64(axis[0]), F64(axis[1])
    vx, vy = -ay, ax
    X0, Y0, X1, Y1 = b[:, 0, 0], b[:, 0, 1], b[:, 1, 0], b[:, 2, 1]
    out = np.zeros(b.shape, F32)
    for corner, (X, Y) in enumerate(((X0, Y0), (X1, Y0), (X1, Y1), (X0, Y1))):
        out[:, corner, 0] = (X * ax + Y * vx).astype(F32)
        out[:, corner, 1] = (X * ay + Y * vy).astype(F32)
    return out


def blocks_page(quads, min_gap_x=1.0, min_gap_y=0.75):
    """One page: blocks_statement.blocks_page of the quads in the page's own frame.  -> its dict, ``boxes`` replaced by the
    rotated rectangles on the page, plus ``frame_boxes`` (what the cut returned), ``frame`` (the quads it saw), ``axis``,
    ``medoid``, ``best`` and ``second`` (page_axis)"""
    quads = np.asarray(quads, dtype=F32).reshape(-1, 4, 2)
    if len(quads) > bs.MAX_QUADS:
        raise ValueError(f"{len(quads)} quads on a page, more than {bs.MAX_QUADS}")
    if not np.isfinite(quads).all():
        raise ValueError("non-finite coordinate")
    found = page_axis(quads)
    frame = to_frame(quads, found["axis"])
    out = bs.blocks_page(frame, min_gap_x, min_gap_y)
    out["frame"], out["frame_boxes"] = frame, out["boxes"]
    out["boxes"] = from_frame(out["frame_boxes"], found["axis"])
    for key in ("axis", "medoid", "best", "second"):
        out[key] = found[key]
    return out


def group_batch(pages, **rule):
    """pages: list of (n_i, 4, 2) -> (block_of (total,), order (total,), block_counts (N,), boxes (blocks, 4, 2)): the arrays
    kocr_group_lines returns for the batch with flags == KOCR_LINES_BLOCKS | KOCR_LINES_DESKEW"""
    results = [blocks_page(p, **rule) for p in pages]
    cat = lambda key, dtype, tail: (np.concatenate([r[key] for r in results]) if results else np.zeros((0,) + tail, dtype)).astype(dtype)  # noqa: E731
    return (cat("block_of", np.int32, ()), cat("order", np.int32, ()), np.array([len(r["blocks"]) for r in results], np.int32),
            cat("boxes", np.float32, (4, 2)))
