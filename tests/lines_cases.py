"""Pages for the line-grouping tests (tests/test_lines_statement_cpu.py, tests/test_lines_gpu.py): hand-made ones with known
answers, exact threshold cases, random pages, long chains.  A page is a float32 (n, 4, 2) array of quads [tl, tr, br, bl]."""
import math

import numpy as np

F32 = np.float32


def box(x, y, w, h):
    return [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]


def page(quads):
    return np.array(quads, dtype=F32).reshape(-1, 4, 2)


def rotated(quads, degrees, centre=(0.0, 0.0)):
    q = np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2) - centre
    c, s = math.cos(math.radians(degrees)), math.sin(math.radians(degrees))
    return page(np.stack([q[..., 0] * c - q[..., 1] * s, q[..., 0] * s + q[..., 1] * c], axis=-1) + centre)


def row(x, y, widths, h=10, gap=8):
    """words of the given widths from x on, `gap` apart, tops at y"""
    out = []
    for w in widths:
        out.append(box(x, y, w, h))
        x += w + gap
    return out


def scrambled(quads, lines, seed):
    """the page with its words permuted, and the lines (lists of word indices in reading order) renamed accordingly"""
    quads = page(quads)
    perm = np.random.default_rng(seed).permutation(len(quads))  # new index k holds old word perm[k]
    where = np.argsort(perm)
    return quads[perm], [[int(where[j]) for j in line] for line in lines]


def hand_made():
    """-> list of (name, quads, expected lines, rule): the lines from the top of the page down, each a list of word indices in
    reading order"""
    cases = []
    # three horizontal lines of 4, 1 and 6 words, heights 10, gaps 8 <= 1.5 * 10, rows 40 apart
    words = row(5, 0, [30, 22, 41, 30]) + row(60, 40, [35]) + row(0, 80, [30, 30, 12, 50, 30, 25])
    cases.append(("three lines scrambled",) + scrambled(words, [[0, 1, 2, 3], [4], [5, 6, 7, 8, 9, 10]], 3) + ({},))
    # the second pair continues the first to the right, 5 lower: across = 5 <= 0.5 * 10 joins them; 6 lower does not
    cases.append(("offset just small enough", page(row(0, 0, [30, 30]) + row(76, 5, [30, 30])), [[0, 1, 2, 3]], {}))
    cases.append(("offset just too large", page(row(0, 0, [30, 30]) + row(76, 6, [30, 30])), [[0, 1], [2, 3]], {}))
    # two rows right under each other, 12 apart: never one line
    cases.append(("two rows", page(row(0, 0, [30, 30, 30]) + row(0, 12, [30, 30, 30])), [[0, 1, 2], [3, 4, 5]], {}))
    # a line rotated by 30 degrees reads as before; by 180 degrees it reads along its own axis (right to left on the page)
    line = row(0, 0, [30, 20, 40, 30, 25])
    cases.append(("rotated 30", rotated(line, 30.0), [[0, 1, 2, 3, 4]], {}))
    cases.append(("rotated 180", rotated(line, 180.0, (100.0, 50.0)), [[0, 1, 2, 3, 4]], {}))
    cases.append(("rotated 30 scrambled",) + scrambled(rotated(line + row(0, 40, [30, 30]), 30.0), [[0, 1, 2, 3, 4], [5, 6]], 4) + ({},))
    # a tall word next to a small one, centred on it: 10 < 0.5 * 21
    cases.append(("tall and small", page([box(0, 0, 30, 21), box(38, 5.5, 30, 10)]), [[0], [1]], {}))
    cases.append(("tall and less small", page([box(0, 0, 30, 20), box(38, 5, 30, 10)]), [[0, 1]], {}))
    # degenerate quads are lines of their own: no width, no height, a point; the two real words around them stay together
    flat = [[(70, 20), (70, 20), (70, 30), (70, 30)], [(75, 40), (90, 40), (90, 40), (75, 40)], [(3, 50), (3, 50), (3, 50), (3, 50)]]
    cases.append(("degenerate", page([box(0, 0, 30, 10)] + flat + [box(38, 0, 30, 10)]), [[0, 4], [1], [2], [3]], {}))
    # another rule: a wider gap joins what the default keeps apart
    cases.append(("default gap", page(row(0, 0, [30, 30], gap=16)), [[0], [1]], {}))
    cases.append(("max_gap 2", page(row(0, 0, [30, 30], gap=16)), [[0, 1]], {"max_gap": 2.0}))
    cases.append(("empty", page([]), [], {}))
    cases.append(("one word", page([box(3, 4, 30, 10)]), [[0]], {}))
    return cases


def _ulp_up(values):
    return np.nextafter(np.asarray(values, F32), F32(np.inf))


def exact_thresholds():
    """Axis-aligned boxes with small integer coordinates: u = (1, 0), m = (1, 0), along = |dx|, across = |dy| and the heights
    are exact in float64, so `==` at a threshold is decided by the rule and not by rounding.  -> (name, quads, lines, rule)"""
    cases = []
    a = box(0, 0, 20, 8)
    # gap = 32 - 0.5 (20 + 20) = 12 = 1.5 * 8
    b = page([box(32, 0, 20, 8)])
    cases.append(("gap at the threshold", np.concatenate([page([a]), b]), [[0, 1]], {}))
    b[..., 0] = _ulp_up(b[..., 0])
    cases.append(("gap one ulp above", np.concatenate([page([a]), b]), [[0], [1]], {}))
    # across = 4 = 0.5 * 8
    b = page([box(25, 4, 20, 8)])
    cases.append(("across at the threshold", np.concatenate([page([a]), b]), [[0, 1]], {}))
    b[..., 1] = _ulp_up(b[..., 1])
    cases.append(("across one ulp above", np.concatenate([page([a]), b]), [[0], [1]], {}))
    # min h = 8 = 0.5 * 16, the two centred on y = 8
    a = box(0, 4, 20, 8)
    b = page([box(25, 0, 20, 16)])
    cases.append(("height ratio at the threshold", np.concatenate([page([a]), b]), [[0, 1]], {}))
    b[0, 2:, 1] = _ulp_up(b[0, 2:, 1])
    cases.append(("height ratio one ulp below", np.concatenate([page([a]), b]), [[0], [1]], {}))
    return cases


def random_page(rng, n):
    """n words: text lines of jittered, slightly rotated words, about a tenth of them noise words anywhere"""
    quads = []
    y = 20.0
    while len(quads) < n:
        h = float(rng.uniform(8, 24))
        if rng.random() < 0.1:
            w, angle = float(rng.uniform(0.5, 5) * h), float(rng.uniform(-40, 40))
            x0, y0 = float(rng.uniform(0, 3000)), float(rng.uniform(0, y + 100))
            quads.append(rotated([box(x0, y0, w, h)], angle, (x0, y0))[0])
            continue
        tilt = float(rng.uniform(-3, 3))
        x = float(rng.uniform(0, 400))
        line = []
        for _ in range(int(rng.integers(1, 40))):
            wh = h * float(rng.uniform(0.85, 1.15))
            w = wh * float(rng.uniform(1.2, 6))
            yy = y + float(rng.uniform(-0.12, 0.12)) * h
            line.append(rotated([box(x, yy, w, wh)], float(rng.uniform(-2, 2)), (x, yy))[0])
            x += w + h * float(rng.uniform(0.15, 1.0)) * (3.0 if rng.random() < 0.05 else 1.0)
        quads.extend(rotated(line, tilt, (0.0, y)))
        y += h * float(rng.uniform(1.6, 3.0))
    quads = page(quads[:n])
    return quads[rng.permutation(n)] if n else quads


BATCH_SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 2048]  # the wave, workgroup and capacity boundaries
BATCH_SEED = 11       # chosen on the CPU: the margin of every page stays above 1e-9 (test_lines_statement_cpu.py)
SMALL_SEEDS = (1, 2, 3)
SMALL_SIZES = (5, 40, 130)
# every parameter away from its default; the margins of the small pages hold under each of them as well
OTHER_RULES = ({"max_angle": 2.0}, {"min_height_ratio": 0.9}, {"max_offset": 0.2}, {"max_gap": 0.4},
               {"max_angle": 30.0, "min_height_ratio": 0.0, "max_offset": 3.0, "max_gap": 6.0})


def small_pages(shift=0):
    return [random_page(np.random.default_rng(seed + shift), n) for seed, n in zip(SMALL_SEEDS, SMALL_SIZES)]


def random_batch(seed=BATCH_SEED, pages=64):
    """64 pages: the boundary sizes, the rest between 4 and 120 words"""
    rng = np.random.default_rng(seed)
    sizes = BATCH_SIZES + [int(v) for v in rng.integers(4, 121, pages - len(BATCH_SIZES))]
    sizes = [sizes[k] for k in rng.permutation(pages)]
    return [random_page(rng, n) for n in sizes]


def chain(n=512, broken=False, seed=9):
    """n words of 20 x 10, 10 apart (the next but one is 40 away: no link), in scrambled index order; `broken`: the gap in
    the middle is 16 > 1.5 * 10.  -> (quads, lines)"""
    xs = [30.0 * k + (6.0 if broken and k >= n // 2 else 0.0) for k in range(n)]
    lines = [list(range(n // 2)), list(range(n // 2, n))] if broken else [list(range(n))]
    return scrambled([box(x, 100, 20, 10) for x in xs], lines, seed)


def flatten(pages):
    """-> quads (total, 4, 2) float32, offsets (N + 1,) int32"""
    quads = np.concatenate([page(p) for p in pages]) if len(pages) else page([])
    return np.ascontiguousarray(quads), np.concatenate([[0], np.cumsum([len(p) for p in pages])]).astype(np.int32)
