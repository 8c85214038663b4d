"""The rule keras_ocr_amd/csrc/blocks.hip implements (kocr_group_lines with flags == KOCR_LINES_BLOCKS), stated in numpy /
Python float64 with every operation in a fixed order, one IEEE operation at a time: the boxes of a page cut into blocks
(columns, paragraphs) by a recursive XY-cut and put into reading order.  The kernel carries out the same operations, so
its integers equal these and its block boxes carry the same float32 bits (tests/test_blocks_gpu.py).  DESIGN.md section
4, "Blocks".

A quad is four float32 points; only its axis-aligned box counts.  One function per step:

  boxes_of      x0, x1, y0, y1 of every quad (float32: min and max are exact)
  mean_height   H: the heights y1 - y0 > 0 summed in ascending index, divided by their number
  gaps          the gaps of a segment along one axis, in the order (start, index)
  cut_segment   rule 2 / rule 3 for one segment: its parts, or None for a block
  blocks_page   the recursion (iterative: it can be as deep as the page has boxes), the blocks in the order it emits them
  group_batch   the arrays kocr_group_lines returns for a batch

The defaults are judgement, not fitted to real pages.
"""
import numpy as np

DEFAULTS = {"min_gap_x": 1.0, "min_gap_y": 0.75}
MAX_QUADS = 2048  # per page


def boxes_of(quads):
    """quads float32 (n, 4, 2) -> x0, x1, y0, y1, each float32 (n,)"""
    q = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)
    return q[:, :, 0].min(axis=1), q[:, :, 0].max(axis=1), q[:, :, 1].min(axis=1), q[:, :, 1].max(axis=1)


def mean_height(y0, y1):
    """H = hsum / count over the quads with y1 > y0, hsum added from 0.0 in ascending index; 0.0 without any"""
    hsum, count = 0.0, 0
    for a, b in zip(y0.tolist(), y1.tolist()):  # float32 -> Python float: exact
        if b > a:
            hsum = hsum + (b - a)
            count += 1
    return hsum / count if count else 0.0


def gaps(members, s, e):
    """members: indices of a segment; s, e: float32 starts and ends of all quads along one axis.  -> (order, g): the members
    by (s, index), and for every one but the first g = float64(s) - max(float64(e) of the members before it) (len - 1,)"""
    m = np.asarray(sorted(members), dtype=np.int64)
    order = m[np.lexsort((m, s[m]))]
    s64, e64 = s[order].astype(np.float64), e[order].astype(np.float64)
    return order, s64[1:] - np.maximum.accumulate(e64)[:-1]


def cut_segment(members, box, tx, ty):
    """-> (axis, parts, gaps cut) or None.  Rule 2: with valid gaps along x (g > 0 and g >= tx) the segment is cut at ALL
    of them, the parts from left to right.  Rule 3: otherwise, with valid gaps along y, at the widest, the first of equal
    ones in (y0, index) order, the part above it first.  Rule 4: otherwise it is a block."""
    x0, x1, y0, y1 = box
    order, g = gaps(members, x0, x1)
    valid = np.flatnonzero((g > 0) & (g >= tx)) + 1  # positions in `order` that a cut falls before
    if valid.size:
        return "x", [part.tolist() for part in np.split(order, valid)], g[valid - 1].tolist()
    order, g = gaps(members, y0, y1)
    valid = (g > 0) & (g >= ty)
    if valid.any():
        k = int(np.argmax(np.where(valid, g, -1.0))) + 1  # argmax: the first of equal ones
        return "y", [order[:k].tolist(), order[k:].tolist()], [float(g[k - 1])]
    return None


def blocks_page(quads, min_gap_x=1.0, min_gap_y=0.75):
    """One page: quads float32 (n, 4, 2) -> dict with
      block_of  (n,) int32   the index of each quad's block in the order the recursion emits the blocks
      order     (n,) int32   the quad indices in reading order: block 0's quads, then block 1's, ...
      blocks    list of lists: the quads of each block by (y0, x0, index)
      boxes     (B, 4, 2) float32  [tl, tr, br, bl] = (X0, Y0), (X1, Y0), (X1, Y1), (X0, Y1) over the block's members
      cuts      list of (axis, segment, parts, gaps cut): every cut made, in the order made (for the tests)
      H, tx, ty the mean height and the two thresholds"""
    quads = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)
    n = len(quads)
    if n > MAX_QUADS:
        raise ValueError(f"{n} quads on a page, more than {MAX_QUADS}")
    if not np.isfinite(quads).all():
        raise ValueError("non-finite coordinate")
    for name, value in (("min_gap_x", min_gap_x), ("min_gap_y", min_gap_y)):
        if not (value >= 0 and np.isfinite(value)):
            raise ValueError(f"{name} {value} is not a finite number >= 0")
    box = boxes_of(quads)
    x0, x1, y0, y1 = box
    H = mean_height(y0, y1)
    tx, ty = float(np.float64(min_gap_x) * np.float64(H)), float(np.float64(min_gap_y) * np.float64(H))
    blocks, cuts = [], []
    stack = [list(range(n))] if n else []
    while stack:  # depth first, the first part of a cut next: the order a recursion emits
        members = stack.pop()
        found = cut_segment(members, box, tx, ty) if len(members) > 1 else None
        if found is None:
            blocks.append(sorted(members, key=lambda j: (float(y0[j]), float(x0[j]), j)))
            continue
        axis, parts, cut_gaps = found
        cuts.append((axis, sorted(members), parts, cut_gaps))
        stack.extend(reversed(parts))
    block_of = np.zeros(n, np.int32)
    boxes = np.zeros((len(blocks), 4, 2), np.float32)
    for k, members in enumerate(blocks):
        block_of[members] = k
        X0, X1, Y0, Y1 = x0[members].min(), x1[members].max(), y0[members].min(), y1[members].max()
        boxes[k] = [[X0, Y0], [X1, Y0], [X1, Y1], [X0, Y1]]
    return {"block_of": block_of, "order": np.array([j for b in blocks for j in b], dtype=np.int32).reshape(-1), "blocks": blocks,
            "boxes": boxes, "cuts": cuts, "H": H, "tx": tx, "ty": ty}


def group_batch(pages, **rule):
    """pages: list of (n_i, 4, 2) -> (block_of (total,), order (total,), block_counts (N,), boxes (blocks, 4, 2)): the arrays
    kocr_group_lines returns for the batch with flags == KOCR_LINES_BLOCKS"""
    results = [blocks_page(p, **rule) for p in pages]
    cat = lambda key, dtype, tail: (np.concatenate([r[key] for r in results]) if results else np.zeros((0,) + tail, dtype)).astype(dtype)  # noqa: E731
    return (cat("block_of", np.int32, ()), cat("order", np.int32, ()), np.array([len(r["blocks"]) for r in results], np.int32),
            cat("boxes", np.float32, (4, 2)))
