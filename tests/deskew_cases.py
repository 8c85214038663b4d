"""The pages of the deskew tests (tests/test_deskew_statement_cpu.py, tests/test_deskew_gpu.py): the pages of
tests/blocks_cases.py rotated about the origin in float64 and rounded to float32.  Nothing is read from a file."""
import numpy as np

from tests import blocks_cases as bc

F32 = np.float32
ANGLES = (3.0, 7.0, 30.0, 90.0, 180.0, -20.0)
SIZES = (0, 1, 2, 63, 64, 65, 257, 1025, 2048)  # the wave edge, the block edge, one and two candidates per lane


def rotated(quads, degrees):
    """the quads turned by ``degrees`` about the origin (y grows down the page: (1, 0) goes to (cos, sin)), computed in
    float64 and rounded to float32"""
    q = np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2)
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    return np.stack([q[:, :, 0] * c - q[:, :, 1] * s, q[:, :, 0] * s + q[:, :, 1] * c], axis=2).astype(F32)


def hand_pages():
    """(name, quads, blocks by hand) of the three unrotated pages that are rotated"""
    quads, blocks = bc.heading_columns_footer()
    by_name = {c[0]: c for c in bc.hand_made()}
    return [("heading columns footer", quads, blocks)] + [(n, by_name[n][1], by_name[n][2]) for n in ("two columns", "one column in paragraphs")]


def rotated_hand_cases():
    """(name, quads, blocks by hand, degrees): every hand page at every angle"""
    return [(f"{name} at {a:g}", rotated(quads, a), blocks, a) for name, quads, blocks in hand_pages() for a in ANGLES]


def outliers(degrees, count=6, size=22.0):
    """``count`` near-square quads (size x size + 1) beside the heading-columns-footer page, turned by a further 90 degrees:
    what a min-area rectangle makes of a short word.  Their summed length, count x size = 132, is far below a quarter of
    the page's (12 quads of 230 or 500)."""
    boxes = [bc.box(600.0 + 40.0 * k, 10.0 + 30.0 * k, size, size + 1.0) for k in range(count)]
    # the same squares with tl -> tr running down their left side: [tr, br, bl, tl] of the upright square
    turned = bc.page(boxes)[:, [1, 2, 3, 0], :]
    return rotated(turned, degrees)


def page_with_outliers(degrees):
    """-> (quads, number of ordinary quads in front): the rotated heading-columns-footer page and its outliers behind it"""
    main = rotated(bc.heading_columns_footer()[0], degrees)
    return np.concatenate([main, outliers(degrees)]), len(main)


def zero_width_page():
    """only quads without width: no direction anywhere, the axis is (1, 0)"""
    return bc.page([bc.box(0, 0, 0, 24), bc.box(0, 30, 0, 24), bc.box(100, 0, 0, 24), bc.box(100, 70, 0, 0)])


def sized_pages():
    """(name, quads): layout pages of every size of SIZES, each rotated by its own seeded angle in (-180, 180)"""
    rng = np.random.default_rng(31)
    out = []
    for n in SIZES:
        angle = float(rng.uniform(-180, 180))
        out.append((f"layout {n} at {angle:.2f}", rotated(bc.layout_page(rng, n), angle) if n else bc.page([])))
    return out


def gpu_cases():
    """(name, quads, rule) of every page the device is compared on"""
    cases = [(name, quads, {}) for name, quads in sized_pages()]
    cases += [(name, quads, {}) for name, quads, _, _ in rotated_hand_cases()]
    cases.append(("only zero widths", zero_width_page(), {}))
    cases.append(("outliers at 12", page_with_outliers(12.0)[0], {}))
    cases.append(("outliers at 0", page_with_outliers(0.0)[0], {}))
    rng = np.random.default_rng(32)
    cases.append(("scatter 300 at -35, other gaps", rotated(bc.scatter_page(rng, 300), -35.0), {"min_gap_x": 0.5, "min_gap_y": 0.25}))
    return cases


def with_empty_pages(pages):
    """the pages as one batch with empty pages in front, behind and among them -> (pages, the position of every given page)"""
    out, at = [bc.page([])], []
    for k, p in enumerate(pages):
        at.append(len(out))
        out.append(p)
        if k % 5 == 1:
            out.append(bc.page([]))
    return out + [bc.page([])], at
