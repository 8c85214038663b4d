"""The pages of the table tests (tests/test_table_statement_cpu.py, tests/test_table_gpu.py): built here from seeded numpy,
nothing is read from a file.  A case is (name, quads float32 (n, 4, 2), answer or None, rule): the answer known by hand as a
dict with some of row / col0 / col1 (per quad), R, S, separators [(a, b)] and K (None: whatever the statement says), and the
rule's keyword arguments.  Unless said otherwise a box is 10 high, so H = 10, tx = 10 and ty = 2.5 under the defaults."""
import numpy as np

from tests.blocks_cases import box, flatten, page  # noqa: F401  (flatten: for the tests)

F32 = np.float32
SIZES = (0, 1, 2, 63, 64, 65, 257, 1025, 2048)


def shuffled(quads, answer, seed):
    """the same page with its quads in another input order, and the per-quad answers in the new indices"""
    perm = np.random.default_rng(seed).permutation(len(quads))  # new index k holds old quad perm[k]
    return quads[perm], {k: ([v[j] for j in perm] if k in ("row", "col0", "col1") else v) for k, v in answer.items()}


def grid_4x3(first_row=0, rows=4):
    """cell (r, c) at x = 100 c, y = 20 r, 40 + 5 ((r + c) % 3) wide: column 0 ends at 40, 45, 50, 40, column 1 at 145, 150,
    140, 145, column 2 at 250, 240, 245, 250.  With K = 2 the runs are (40, 100) and (145, 200); (245, 250) reaches the right
    edge and is dropped"""
    boxes, cells = [], []
    for r in range(rows):
        for c in range(3):
            boxes.append(box(100 * c, 20 * (r + first_row), 40 + 5 * ((r + c) % 3), 10))
            cells.append((r + first_row, c))
    return boxes, cells


def hand_made():
    cases = []
    boxes, cells = grid_4x3()
    answer = {"row": [r for r, _ in cells], "col0": [c for _, c in cells], "col1": [c for _, c in cells], "R": 4, "S": 2, "K": 2,
              "separators": [(40.0, 100.0), (145.0, 200.0)]}
    cases.append(("grid 4x3", page(boxes), answer, {}))
    cases.append(("grid 4x3 shuffled", *shuffled(page(boxes), answer, 1), {}))

    # a title over the full width: no white in its row, K = ceil(2.5) = 3 of 5 rows, the four others still show the gutters
    # (the first from 45: only two rows are white on (40, 45))
    boxes, cells = grid_4x3(first_row=1)
    cases.append(("title row", page([box(0, 0, 250, 10)] + boxes),
                  {"row": [0] + [r for r, _ in cells], "col0": [0] + [c for _, c in cells], "col1": [2] + [c for _, c in cells], "R": 5, "S": 2,
                   "K": 3, "separators": [(45.0, 100.0), (145.0, 200.0)]}, {}))

    # a "total" row under the last two columns: its left margin (0, 100) votes for the first gutter
    boxes, cells = grid_4x3()
    cases.append(("total row", page(boxes + [box(100, 80, 40, 10), box(200, 80, 50, 10)]),
                  {"row": [r for r, _ in cells] + [4, 4], "col0": [c for _, c in cells] + [1, 2], "col1": [c for _, c in cells] + [1, 2], "R": 5,
                   "S": 2, "K": 3, "separators": [(40.0, 100.0), (145.0, 200.0)]}, {}))

    # the first column filled in row 2 only (50 wide): three left margins (0, 100) and one gap (50, 100): c = 3 on (0, 50),
    # 4 on (50, 100), one run from X0, which is kept: the lone box is column 0, whose band has no width
    boxes, cells = grid_4x3()
    keep = [k for k, (r, c) in enumerate(cells) if c > 0 or r == 2]
    cases.append(("first column in 1 of 4 rows", page([boxes[k] for k in keep]),
                  {"row": [cells[k][0] for k in keep], "col0": [cells[k][1] for k in keep], "col1": [cells[k][1] for k in keep], "R": 4, "S": 2,
                   "separators": [(0.0, 100.0), (145.0, 200.0)]}, {}))

    # ragged right: column 0 is 20, 60, 35, 80 wide; c reaches 2 at 35; the 80-wide box still lies in column 0 alone
    widths = [20, 60, 35, 80]
    boxes = [b for r, w in enumerate(widths) for b in (box(0, 20 * r, w, 10), box(100, 20 * r, 50, 10))]
    cases.append(("ragged right", page(boxes), {"row": [0, 0, 1, 1, 2, 2, 3, 3], "col0": [0, 1] * 4, "col1": [0, 1] * 4, "R": 4, "S": 1,
                                                "separators": [(35.0, 100.0)]}, {}))

    # two rows whose gaps (40, 60) and (55, 75) share (55, 60), 5 wide: with both rows required, no separator
    two = page([box(0, 0, 40, 10), box(60, 0, 40, 10), box(0, 20, 55, 10), box(75, 20, 25, 10)])
    cases.append(("gaps overlap by less than tx", two, {"row": [0, 0, 1, 1], "col0": [0] * 4, "col1": [0] * 4, "R": 2, "S": 0, "K": 2,
                                                          "separators": []}, {"min_support": 1.0}))
    # and with one row enough the two gaps merge into one run, which ends at 75: the box from 60 to 100 spans both columns
    cases.append(("gaps overlap, one row enough", two, {"col0": [0, 0, 0, 1], "col1": [0, 1, 0, 1], "S": 1, "K": 1, "separators": [(40.0, 75.0)]}, {"min_support": 0.5}))

    # an indented table under an outdented row: c = 3 on (0, 20), a run that starts at X0 and is kept; the outdented box
    # spans the columns 0 and 1
    boxes = [box(0, 0, 30, 10)] + [b for r in (1, 2, 3) for b in (box(20, 20 * r, 40, 10), box(80, 20 * r, 40, 10))]
    cases.append(("indented under outdented", page(boxes), {"row": [0, 1, 1, 2, 2, 3, 3], "col0": [0, 1, 2, 1, 2, 1, 2], "col1": [1, 1, 2, 1, 2, 1, 2],
                                                            "R": 4, "S": 2, "separators": [(0.0, 20.0), (60.0, 80.0)]}, {}))

    # a zero-width quad (it has a height) inside a gutter of row 0, and a zero-height one as a row of its own
    boxes = [box(0, 0, 40, 10), box(100, 0, 40, 10), box(0, 20, 40, 10), box(100, 20, 40, 10), box(60, 0, 0, 10), box(100, 40, 40, 0)]
    cases.append(("zero width and zero height", page(boxes), {"row": [0, 0, 1, 1, 0, 2], "col0": [0, 1, 0, 1, 0, 1], "col1": [0, 1, 0, 1, 0, 1], "R": 3,
                                                              "S": 1, "K": 2, "separators": [(40.0, 100.0)]}, {}))
    # only such quads: H = 0, so every positive gap counts; the one run (0, 30) reaches the right edge
    boxes = [box(0, 0, 10, 0), box(20, 0, 10, 0), box(0, 5, 0, 0)]
    cases.append(("only quads without height", page(boxes), {"row": [0, 0, 1], "col0": [0] * 3, "col1": [0] * 3, "R": 2, "S": 0, "separators": []}, {}))

    cases.append(("one quad", page([box(3, 4, 30, 10)]), {"row": [0], "col0": [0], "col1": [0], "R": 1, "S": 0, "K": 1, "separators": []}, {}))
    cases.append(("duplicates", page([box(0, 0, 40, 10), box(100, 0, 40, 10), box(0, 0, 40, 10), box(100, 0, 40, 10)]),
                  {"row": [0] * 4, "col0": [0, 1, 0, 1], "col1": [0, 1, 0, 1], "R": 1, "S": 1, "separators": [(40.0, 100.0)]}, {}))
    return cases


def threshold_edges():
    """gaps equal to their threshold and one float32 below it, on integer boxes (H = 10 exactly)"""
    below = lambda v: float(np.nextafter(F32(v), F32(0)))  # noqa: E731
    cases = []
    cases.append(("x gap equal to tx", page([box(0, 0, 40, 10), box(50, 0, 40, 10)]), {"col0": [0, 1], "S": 1, "separators": [(40.0, 50.0)]}, {}))
    narrow = page([box(0, 0, 40, 10), [[below(50), 0], [90, 0], [90, 10], [below(50), 10]]])
    cases.append(("x gap one float32 below tx", narrow, {"col0": [0, 0], "S": 0, "separators": []}, {}))
    cases.append(("y gap equal to ty", page([box(0, 0, 40, 10), box(0, 12.5, 40, 10)]), {"row": [0, 1], "R": 2}, {}))
    close = page([box(0, 0, 40, 10), [[0, below(12.5)], [40, below(12.5)], [40, 22.5], [0, 22.5]]])
    # the second box is a little higher than 10 then: H > 10 and ty > 2.5 all the more
    cases.append(("y gap one float32 below ty", close, {"row": [0, 0], "R": 1}, {}))
    # a run as wide as tx exactly, between two rows' gaps (40, 60) and (50, 70), and one float32 narrower
    cases.append(("run equal to tx", page([box(0, 0, 40, 10), box(60, 0, 40, 10), box(0, 20, 50, 10), box(70, 20, 30, 10)]),
                  {"col0": [0, 1, 0, 1], "S": 1, "separators": [(50.0, 60.0)]}, {"min_support": 1.0}))
    edge = page([box(0, 0, 40, 10), [[below(60), 0], [100, 0], [100, 10], [below(60), 10]], box(0, 20, 50, 10), box(70, 20, 30, 10)])
    cases.append(("run one float32 below tx", edge, {"col0": [0] * 4, "S": 0, "separators": []}, {"min_support": 1.0}))
    return cases


def support_page():
    """four rows; the gutter (40, 60) shows in 4 of them, (100, 120) in 2, (160, 180) in 1"""
    return page([box(0, 0, 40, 10), box(60, 0, 40, 10), box(120, 0, 40, 10), box(180, 0, 40, 10),
                 box(0, 20, 40, 10), box(60, 20, 40, 10), box(120, 20, 100, 10),
                 box(0, 40, 40, 10), box(60, 40, 160, 10),
                 box(0, 60, 40, 10), box(60, 60, 160, 10)])


def support_cases():
    quads = support_page()
    a, b, c = (40.0, 60.0), (100.0, 120.0), (160.0, 180.0)
    cases = [("min_support 0", quads, {"K": 1, "S": 3, "separators": [a, b, c], "col0": [0, 1, 2, 3, 0, 1, 2, 0, 1, 0, 1], "col1": [0, 1, 2, 3, 0, 1, 3, 0, 3, 0, 3]},
              {"min_support": 0.0}),
             ("min_support 0.5", quads, {"K": 2, "S": 2, "separators": [a, b], "col1": [0, 1, 2, 2, 0, 1, 2, 0, 2, 0, 2]}, {"min_support": 0.5}),
             ("min_support 1", quads, {"K": 4, "S": 1, "separators": [a], "col0": [0, 1, 1, 1, 0, 1, 1, 0, 1, 0, 1]}, {"min_support": 1.0}),
             # 0.75 x 4 = 3 exactly: K = 3, not 4; (100, 120) shows in 2 rows only
             ("min_support 0.75, K integral", quads, {"K": 3, "S": 1, "separators": [a]}, {"min_support": 0.75})]
    # 0.25 x 4 = 1 exactly: K = 1
    cases.append(("min_support 0.25, K integral", quads, {"K": 1, "S": 3}, {"min_support": 0.25}))
    return cases


def grid_page(n, seed, cols=None):
    """n boxes of a table with jittered float coordinates: `cols` columns (seeded 2 .. 6), some cells empty, some reaching
    into the next column, now and then a row over the full width"""
    rng = np.random.default_rng([n, seed])
    cols = int(rng.integers(2, 7)) if cols is None else cols
    pitch, boxes, r = 120.0, [], 0
    while len(boxes) < n:
        y = 22.0 * r + float(rng.uniform(0, 3))
        if rng.random() < 0.05:
            boxes.append(box(float(rng.uniform(0, 4)), y, pitch * cols - 30, float(rng.uniform(9, 12))))
        else:
            for c in range(cols):
                if len(boxes) >= n or rng.random() < 0.15:
                    continue
                w = float(rng.uniform(15, 100)) if rng.random() > 0.05 else float(rng.uniform(110, 200))
                boxes.append(box(pitch * c + float(rng.uniform(0, 6)), y, w, float(rng.uniform(9, 12))))
        r += 1
    quads = page(boxes[:n])
    return quads[rng.permutation(n)] if n else quads


def single_rows(n=2048):
    """n rows of one box each, stepping to the right and back: 2 n margins, the largest number of white intervals"""
    return page([box(7.0 * (k % 13), 15.0 * k, 30 + (k % 5), 10) for k in range(n)])


def single_row(n=2048):
    """n boxes in one row, 10 apart: n - 1 separators, the most a page can have"""
    return page([box(30.0 * k, k % 3, 20, 10) for k in range(n)])


def random_cases():
    cases = [(f"grid {n}", grid_page(n, 0), None, {}) for n in SIZES]
    cases.append(("grid 300, narrow gutters", grid_page(300, 1), None, {"min_gap_x": 0.3, "min_gap_y": 0.1, "min_support": 0.3}))
    cases.append(("grid 300, all rows", grid_page(300, 2, cols=3), None, {"min_support": 1.0}))
    cases.append(("2048 single rows", single_rows(), None, {}))
    cases.append(("2048 in one row", single_row(), {"R": 1, "S": 2047}, {}))
    return cases


def every_case():
    return hand_made() + threshold_edges() + support_cases() + random_cases()


def mixed_batch():
    """a ragged batch with empty pages at both ends and in the middle"""
    e = page([])
    return [e, hand_made()[0][1], e, e, grid_page(65, 3), page([box(0, 0, 30, 10)]), grid_page(257, 4), support_page(), e]


def small_integer_pages(count=300, seed=5):
    """pages of 1 .. 8 boxes on a coarse integer lattice, so that edges coincide and gaps equal their thresholds often"""
    rng = np.random.default_rng(seed)
    pages = []
    for _ in range(count):
        n = int(rng.integers(1, 9))
        boxes = [box(int(rng.integers(0, 12)) * 4, int(rng.integers(0, 6)) * 4, int(rng.integers(0, 5)) * 4, int(rng.integers(0, 3)) * 4) for _ in range(n)]
        rule = {"min_gap_x": float(rng.choice([0.0, 0.5, 1.0, 2.0])), "min_gap_y": float(rng.choice([0.0, 0.25, 1.0])),
                "min_support": float(rng.choice([0.0, 0.5, 0.75, 1.0]))}
        pages.append((page(boxes), rule))
    return pages
