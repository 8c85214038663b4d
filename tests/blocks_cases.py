"""The pages of the block tests (tests/test_blocks_statement_cpu.py, tests/test_blocks_gpu.py): built here from seeded numpy,
nothing is read from a file.  A case is (name, quads float32 (n, 4, 2), blocks or None, rule): the blocks known by hand as
lists of quad indices in reading order (None: whatever the statement says), and the rule's keyword arguments."""
import numpy as np

F32 = np.float32
SIZES = (1, 63, 64, 65, 1025)


def box(x, y, w, h):
    """the quad [tl, tr, br, bl] of the rectangle at (x, y), w wide and h high"""
    return [[x, y], [x + w, y], [x + w, y + h], [x, y + h]]


def page(boxes):
    return np.array(boxes, dtype=F32).reshape(-1, 4, 2)


def flatten(pages):
    """-> (quads (total, 4, 2) float32, offsets (N + 1,) int32)"""
    quads = np.concatenate([page(p) for p in pages]) if len(pages) else page([])
    return quads, np.concatenate([[0], np.cumsum([len(p) for p in pages])]).astype(np.int32)


def shuffled(quads, blocks, seed):
    """the same page with its quads in another input order, and the blocks in the new indices"""
    perm = np.random.default_rng(seed).permutation(len(quads))  # new index k holds old quad perm[k]
    new = np.argsort(perm)
    return quads[perm], [[int(new[j]) for j in b] for b in blocks]


def column(x, y, widths, gaps, h=24.0):
    """boxes h high under each other from (x, y): box k is widths[k] wide, gaps[k] below the one before it (gaps[0] unused)"""
    out = []
    for k, w in enumerate(widths):
        if k:
            y += gaps[k]
        out.append(box(x, y, w, h))
        y += h
    return out


def heading_columns_footer():
    """heading 0; column 1 in two paragraphs 1 2 3 | 4 5; column 2 in two paragraphs 6 7 8 | 9 10 whose break lines up with
    column 1's; footer 11.  Heading gap 40, paragraph gaps 36, footer gap 46, line gaps 6, boxes 24 high, gutter 40."""
    col_gaps = [0, 6, 6, 36, 6]
    boxes = [box(0, 0, 500, 24)] + column(0, 64, [230] * 5, col_gaps) + column(270, 64, [230] * 5, col_gaps) + [box(0, 64 + 5 * 24 + 54 + 46, 500, 24)]
    return page(boxes), [[0], [1, 2, 3], [4, 5], [6, 7, 8], [9, 10], [11]]


def all_at_once_order():
    """what cutting every horizontal gap at once would make of heading_columns_footer: band by band"""
    return [[0], [1, 2, 3], [6, 7, 8], [4, 5], [9, 10], [11]]


def equal_widest():
    """a wide box over two rows of two boxes, both row gaps 40: the topmost gap is cut first, which frees the columns --
    W, L, L2, R, R2; cutting the lower one first would read W, L, R, L2, R2"""
    boxes = [box(0, 0, 300, 32), box(0, 72, 100, 32), box(200, 72, 100, 32), box(0, 144, 100, 32), box(200, 144, 100, 32)]
    return page(boxes), [[0], [1], [3], [2], [4]], [[0], [1], [2], [3], [4]]


def staircase(steps=40, size=20.0, gap=8.0):
    """box 0 stands at the left over the full height of the rest, box 1 lies on top of what remains over its full width,
    box 2 stands at the left of what then remains, ...: every cut peels one box, alternately along x and y"""
    x, y, w, h = 0.0, 0.0, 800.0, 800.0
    boxes = []
    for k in range(steps - 1):
        if k % 2 == 0:
            boxes.append(box(x, y, size, h))
            x, w = x + size + gap, w - size - gap
        else:
            boxes.append(box(x, y, w, size))
            y, h = y + size + gap, h - size - gap
    boxes.append(box(x, y, w, h))
    assert w > 0 and h > 0
    return page(boxes), [[k] for k in range(steps)]


def tall_column(n=2048, h=10.0, gap=10.0):
    """n one-line blocks under each other with equal gaps: every round peels the topmost"""
    return page([box(0, k * (h + gap), 100, h) for k in range(n)]), [[k] for k in range(n)]


def hand_made():
    cases = []
    quads, blocks = heading_columns_footer()
    cases.append(("heading columns footer", *shuffled(quads, blocks, 1), {}))
    two = page(column(0, 0, [200] * 3, [0, 6, 6]) + column(240, 0, [200] * 3, [0, 6, 6]))
    cases.append(("two columns", two, [[0, 1, 2], [3, 4, 5]], {}))
    cases.append(("one column in paragraphs", page(column(0, 0, [300] * 6, [0, 6, 30, 6, 6, 20])), [[0, 1], [2, 3, 4], [5]], {}))
    ragged = page(column(0, 0, [200, 120, 180, 60], [0, 6, 6, 6]) + column(240, 3, [150, 200, 90, 170], [0, 5, 7, 6]))
    cases.append(("ragged", ragged, [[0, 1, 2, 3], [4, 5, 6, 7]], {}))
    sidebar = page(column(0, 0, [200] * 3, [0, 6, 6]) + column(230, 10, [200] * 3, [0, 8, 5]) + column(470, 4, [80] * 2, [0, 12]))
    cases.append(("sidebar", *shuffled(sidebar, [[0, 1, 2], [3, 4, 5], [6, 7]], 2), {}))
    quads, first, _ = equal_widest()
    cases.append(("equal widest gaps", quads, first, {}))
    # five copies of one box and a box beside them: the copies are one block, in index order
    copies = page([box(0, 0, 100, 24)] * 3 + [box(200, 0, 100, 24)] + [box(0, 0, 100, 24)] * 2)
    cases.append(("duplicates", copies, [[0, 1, 2, 4, 5], [3]], {}))
    # a box inside a box, two that overlap, and a third a column away that overlaps nothing
    nested = page([box(0, 0, 300, 200), box(50, 50, 40, 24), box(280, 100, 100, 24), box(600, 0, 100, 24), box(600, 30, 100, 24)])
    cases.append(("nested and overlapping", nested, [[0, 1, 2], [3, 4]], {}))
    # quads without height or width among ordinary ones: they count for the gaps, not for H (24 here)
    flat = page([box(0, 0, 100, 24), box(0, 30, 100, 0), box(0, 36, 0, 24), box(200, 0, 100, 24), box(250, 80, 0, 0)])
    cases.append(("zero height and width", flat, [[0, 1, 2], [3], [4]], {}))
    # only such quads: H = 0, so tx = ty = 0 and every positive gap is cut
    nothing = page([box(0, 0, 100, 0), box(0, 5, 100, 0), box(100, 0, 0, 0), box(101, 0, 0, 0), box(0, 0, 100, 0)])
    cases.append(("only zero heights", nothing, [[0, 4, 2], [1], [3]], {}))
    quads, blocks = staircase()
    cases.append(("staircase", *shuffled(quads, blocks, 3), {"min_gap_x": 0.01, "min_gap_y": 0.01}))
    return cases


def threshold_edges():
    """two boxes 32 high, so H = 32 and t = 32 min_gap exactly (0.75 x 32 = 24): a gap of exactly t is cut, the float32
    just below it is not; with min_gap = 0 a gap of 0 is not cut and the smallest positive float32 is.  (Along y the
    second box of a "just below" case ends at a rounded float32, 56 or 72, and is a hair higher than 32: t only grows.)"""
    cases = []
    below = lambda v: float(np.nextafter(F32(v), F32(0)))  # noqa: E731
    tiny = float(np.nextafter(F32(0), F32(1)))
    for axis, t, rule in (("x", 32.0, {}), ("y", 24.0, {}), ("x", 16.0, {"min_gap_x": 0.5}), ("y", 40.0, {"min_gap_y": 1.25})):
        zero = {"min_gap_x": 0.0} if axis == "x" else {"min_gap_y": 0.0}
        for what, gap, cut, r in (("exactly t", t, True, rule), ("just below t", below(t), False, rule), ("gap 0, min_gap 0", 0.0, False, zero),
                                  ("smallest gap, min_gap 0", tiny, True, zero)):
            # the first box ends at 0, so the gap is the second one's start
            second = box(gap, 0, 50, 32) if axis == "x" else box(0, gap, 50, 32)
            first = box(-50, 0, 50, 32) if axis == "x" else box(0, -32, 50, 32)
            cases.append((f"{axis} {what} ({t})", page([first, second]), [[0], [1]] if cut else [[0, 1]], r))
    return cases


def layout_page(rng, n):
    """n boxes laid out like a page: one to four columns of ragged lines in paragraphs, the odd heading over all of them"""
    boxes, y = [], 0.0
    while len(boxes) < n:
        if rng.random() < 0.3:
            boxes.append(box(float(rng.uniform(0, 40)), y, float(rng.uniform(500, 900)), float(rng.uniform(24, 40))))
            y += 40 + float(rng.uniform(20, 60))
            continue
        columns = int(rng.integers(1, 5))
        width = 900.0 / columns
        bottom = y
        for c in range(columns):
            cy = y + float(rng.uniform(0, 10))
            for _ in range(int(rng.integers(1, 12))):
                h = float(rng.uniform(18, 26))
                boxes.append(box(c * width + float(rng.uniform(0, 5)), cy, float(rng.uniform(0.3, 0.9)) * (width - 40), h))
                cy += h + (float(rng.uniform(2, 8)) if rng.random() < 0.75 else float(rng.uniform(20, 60)))
            bottom = max(bottom, cy)
        y = bottom + float(rng.uniform(10, 80))
    chosen = rng.permutation(len(boxes))[:n]
    return page(boxes)[chosen]


def scatter_page(rng, n):
    """n small boxes thrown into the cells of a grid with lanes of 60 between them, overlapping as they fall; one box in
    sixteen is long enough to bridge a lane along x or y, so that the lanes come apart in an order of their own"""
    cells = int(np.ceil(np.sqrt(n / 6.0)))
    boxes = []
    for _ in range(n):
        cx, cy = (rng.integers(0, cells, 2) * 200.0).tolist()
        x, y = cx + float(rng.uniform(0, 80)), cy + float(rng.uniform(0, 120))
        w, h = float(rng.uniform(5, 60)), float(rng.uniform(8, 20))
        bridge = int(rng.integers(0, 32))
        if bridge == 0:
            w += 150.0
        elif bridge == 1:
            h += 150.0
        boxes.append(box(x, y, w, h))
    return page(boxes)


def random_cases():
    """300 and 2048 random boxes of both kinds, and pages of 1, 63, 64, 65 and 1025"""
    rng = np.random.default_rng(20)
    cases = [(f"layout {n}", layout_page(rng, n), None, {}) for n in (300, 2048)]
    cases += [(f"scatter {n}", scatter_page(rng, n), None, rule) for n, rule in ((300, {}), (2048, {"min_gap_x": 0.5, "min_gap_y": 0.25}))]
    cases += [(f"{'layout' if k % 2 else 'scatter'} {n}", (layout_page if k % 2 else scatter_page)(rng, n), None, {}) for k, n in enumerate(SIZES)]
    return cases


def every_case():
    quads, blocks = tall_column()
    return hand_made() + threshold_edges() + random_cases() + [("column of 2048 blocks", quads, blocks, {})]


def mixed_batch():
    """default-rule cases of every kind with empty pages among them, as one batch"""
    pages = [c[1] for c in hand_made() + threshold_edges() if not c[3]] + [c[1] for c in random_cases() if not c[3] and len(c[1]) <= 300]
    out = [page([])]
    for k, p in enumerate(pages):
        out.append(p)
        if k % 4 == 1:
            out.append(page([]))
    return out + [page([])]
