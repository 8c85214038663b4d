"""The rule keras_ocr_amd/csrc/table.hip implements (kocr_group_lines with flags == KOCR_LINES_TABLE), stated in numpy /
Python float64 with one IEEE operation at a time: the word boxes of ONE table put into rows, columns and spanning cells by
the white space between them.  The kernel carries out the same comparisons, subtractions and products, so its integers
equal these and its band boxes carry the same float32 bits (tests/test_table_gpu.py).  DESIGN.md section 4, "Tables".

A quad is four float32 points; only its axis-aligned box counts.  One function per step:

  rows_of          the page cut at ALL valid gaps along y (no recursion): the row of every quad
  white_intervals  per row the open intervals of x that no box of the row covers: the interior gaps of at least tx, and
                   the margins between the row's extent and the page's, whatever their width
  coverage_runs    the maximal runs of elementary intervals that at least K rows leave white
  table_page       separators (the runs that are wide enough and do not reach the right edge), the cell of every quad,
                   the row and column bands
  group_batch      the arrays kocr_group_lines returns for a batch
  reading_order    (row, col0, x0, index)

The defaults are judgement, not fitted to real pages.
"""
import math

import numpy as np

from tests.blocks_statement import boxes_of, mean_height

DEFAULTS = {"min_gap_x": 1.0, "min_gap_y": 0.25, "min_support": 0.5}
MAX_QUADS = 2048  # per page


def rows_of(y0, y1, ty):
    """-> (row of every quad (n,) int, R).  The quads by (y0, index); g = float64(y0) - max(float64(y1) of the quads
    before); a new row starts where g > 0 and g >= ty."""
    n = len(y0)
    row = np.zeros(n, np.int64)
    if n == 0:
        return row, 0
    order = np.lexsort((np.arange(n), y0))
    top, r = float(y1[order[0]]), 0
    for i in order[1:].tolist():
        g = float(y0[i]) - top  # one float64 subtraction of two float32 values
        if g > 0 and g >= ty:
            r += 1
        row[i] = r
        top = max(top, float(y1[i]))
    return row, r + 1


def white_intervals(members, x0, x1, X0, X1, tx):
    """the white intervals (a, b) of one row, as Python floats that are float32 values"""
    order = sorted(members, key=lambda j: (float(x0[j]), j))
    out = []
    reach = float(x1[order[0]])
    for i in order[1:]:
        a, b = reach, float(x0[i])
        if b - a > 0 and b - a >= tx:
            out.append((a, b))
        reach = max(reach, float(x1[i]))
    left, right = float(x0[order[0]]), reach  # the row's extent: min x0, max x1
    if left > X0:
        out.append((X0, left))
    if right < X1:
        out.append((right, X1))
    return out


def coverage_runs(intervals_by_row, K):
    """-> the maximal runs [(a, b)] of elementary intervals (between two consecutive distinct endpoint values) on which at
    least K rows have a white interval, from the left.  c is counted per elementary interval: the white intervals are open
    and an elementary interval lies inside one or outside it.  The white intervals of ONE row do not overlap (an interior
    gap lies between boxes of the row, a margin outside all of them), so the rows that cover (lo, hi) are as many as the
    intervals of all rows that do: those with a <= lo less those with b <= lo, two integer counts."""
    starts = np.sort(np.array([a for row in intervals_by_row for a, _ in row], np.float64))
    ends = np.sort(np.array([b for row in intervals_by_row for _, b in row], np.float64))
    points = sorted(set(starts.tolist()) | set(ends.tolist()))
    covered = (np.searchsorted(starts, points, side="right") - np.searchsorted(ends, points, side="right")).tolist()
    runs = []
    for lo, hi, c in zip(points[:-1], points[1:], covered):
        if c >= K:
            if runs and runs[-1][1] == lo:
                runs[-1] = (runs[-1][0], hi)
            else:
                runs.append((lo, hi))
    return runs


def table_page(quads, min_gap_x=1.0, min_gap_y=0.25, min_support=0.5):
    """One page: quads float32 (n, 4, 2) -> dict with
      row, col0, col1  (n,) int32  the row of every quad and the first and last column it touches
      R, S             rows and separators (S + 1 columns); 0 and -1 on a page without quads
      separators       [(a, b)] Python floats holding float32 values
      row_boxes        (R, 4, 2) float32   [(X0, Y0_r), (X1, Y0_r), (X1, Y1_r), (X0, Y1_r)]
      col_boxes        (S + 1, 4, 2) float32, column k from X0 (k = 0) or b_{k-1} to X1 (k = S) or a_k over Y0 .. Y1
      white, runs, K, H, tx, ty    for the tests"""
    quads = np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)
    n = len(quads)
    if n > MAX_QUADS:
        raise ValueError(f"{n} quads on a page, more than {MAX_QUADS}")
    if not np.isfinite(quads).all():
        raise ValueError("non-finite coordinate")
    for name, value in (("min_gap_x", min_gap_x), ("min_gap_y", min_gap_y)):
        if not (value >= 0 and np.isfinite(value)):
            raise ValueError(f"{name} {value} is not a finite number >= 0")
    if not 0 <= min_support <= 1:
        raise ValueError(f"min_support {min_support} outside [0, 1]")
    x0, x1, y0, y1 = boxes_of(quads)
    H = mean_height(y0, y1)
    tx, ty = float(np.float64(min_gap_x) * np.float64(H)), float(np.float64(min_gap_y) * np.float64(H))
    empty = np.zeros(0, np.int32)
    if n == 0:
        return {"row": empty, "col0": empty, "col1": empty, "R": 0, "S": -1, "separators": [], "row_boxes": np.zeros((0, 4, 2), np.float32),
                "col_boxes": np.zeros((0, 4, 2), np.float32), "white": [], "runs": [], "K": 0, "H": H, "tx": tx, "ty": ty}
    X0, X1, Y0, Y1 = float(x0.min()), float(x1.max()), float(y0.min()), float(y1.max())
    row, R = rows_of(y0, y1, ty)
    members = [np.flatnonzero(row == r).tolist() for r in range(R)]
    white = [white_intervals(m, x0, x1, X0, X1, tx) for m in members]
    K = max(1, int(math.ceil(float(np.float64(min_support) * np.float64(R)))))
    runs = coverage_runs(white, K)
    separators = [(a, b) for a, b in runs if b - a >= tx and b < X1]
    ends = np.array([b for _, b in separators], np.float64)  # ascending
    col0 = np.searchsorted(ends, x0.astype(np.float64), side="right").astype(np.int32)  # #{s : b_s <= x0}
    col1 = np.maximum(col0, np.searchsorted(ends, x1.astype(np.float64), side="left").astype(np.int32))  # #{s : b_s < x1}
    f = np.float32
    row_boxes = np.zeros((R, 4, 2), np.float32)
    for r, m in enumerate(members):
        top, bottom = y0[m].min(), y1[m].max()
        row_boxes[r] = [[f(X0), top], [f(X1), top], [f(X1), bottom], [f(X0), bottom]]
    S = len(separators)
    col_boxes = np.zeros((S + 1, 4, 2), np.float32)
    for k in range(S + 1):
        left = f(X0) if k == 0 else f(separators[k - 1][1])
        right = f(X1) if k == S else f(separators[k][0])
        col_boxes[k] = [[left, f(Y0)], [right, f(Y0)], [right, f(Y1)], [left, f(Y1)]]
    return {"row": row.astype(np.int32), "col0": col0, "col1": col1, "R": R, "S": S, "separators": separators, "row_boxes": row_boxes,
            "col_boxes": col_boxes, "white": white, "runs": runs, "K": K, "H": H, "tx": tx, "ty": ty}


def reading_order(quads, row, col0):
    """the quad indices by (row, col0, x0, index)"""
    x0 = boxes_of(quads)[0]
    return sorted(range(len(row)), key=lambda j: (int(row[j]), int(col0[j]), float(x0[j]), j))


def group_batch(pages, **rule):
    """pages: list of (n_i, 4, 2) -> (line_of (total,), order (total,), line_counts (N,), line_boxes (bands, 4, 2)): the
    arrays kocr_group_lines returns for the batch with flags == KOCR_LINES_TABLE: the row of every quad; col0 | col1 << 16;
    R_i + S_i + 1 bands per page (0 for a page without quads); per page its row bands, then its column bands"""
    results = [table_page(p, **rule) for p in pages]
    cat = lambda parts, dtype, tail: (np.concatenate(parts) if parts else np.zeros((0,) + tail, dtype)).astype(dtype)  # noqa: E731
    return (cat([r["row"] for r in results], np.int32, ()),
            cat([r["col0"].astype(np.int32) | (r["col1"].astype(np.int32) << 16) for r in results], np.int32, ()),
            np.array([r["R"] + r["S"] + 1 for r in results], np.int32),
            cat([b for r in results for b in (r["row_boxes"], r["col_boxes"])], np.float32, (4, 2)))
