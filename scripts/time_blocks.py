#!/usr/bin/env python
"""Timing record of the XY-cut on the device ("Blocks"): the milliseconds of the profiler rows
blocks_cut and lines_pack (kocr_profile_report) for
  1. the worst case of the round loop, one column of 2048 one-line blocks (2047 cutting rounds),
  2. a batch of 32 pages of 64 lines laid out in columns and paragraphs,
  3. one page of 2048 boxes laid out in columns and paragraphs,
each after a warm-up call, as the median of several calls, with the statement's answer checked on the first.  Writes the
record to --out.  Needs a GPU; exits non-zero on the first failure.

--deskew times the cut in the page's own frame instead ("Rotated pages"): every workload rotated by 5 degrees with
KOCR_LINES_DESKEW, the rows blocks_axis, blocks_frame, blocks_cut, blocks_unframe and lines_pack, checked against
tests/deskew_statement.py; and, from the same run, plain block mode on the unrotated workloads, so that the record
shows what the axis costs on top of the cut.  Its default --out is profiles/blocks_deskew_times.txt.

usage: python scripts/time_blocks.py [--deskew] [--out profiles/blocks_times.txt] [--runs 9]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import blocks_cases as bc  # noqa: E402
from tests import blocks_statement as bs  # noqa: E402
from tests import deskew_cases as dc  # noqa: E402
from tests import deskew_statement as ds  # noqa: E402

PLAIN_ROWS = ("blocks_cut", "lines_pack")
DESKEW_ROWS = ("blocks_axis", "blocks_frame", "blocks_cut", "blocks_unframe", "lines_pack")
DESKEW_ANGLE = 5.0


def measure(ctx, pages, runs, deskew=False):
    quads, offsets = bc.flatten(pages)
    want = (ds if deskew else bs).group_batch(pages)
    call = ctx.group_blocks_deskewed if deskew else ctx.group_blocks
    got = call(quads, offsets)  # warm-up, and the check
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), "the device disagrees with the statement"
    rows = {name: [] for name in (DESKEW_ROWS if deskew else PLAIN_ROWS)}
    for _ in range(runs):
        ctx.profile_reset()
        call(quads, offsets)
        report = ctx.profile_report()
        for name, values in rows.items():
            assert report[name]["launches"] == 1, (name, report.get(name))
            values.append(report[name]["ms"])
    return int(want[2].sum()), {name: (statistics.median(v), min(v), max(v)) for name, v in rows.items()}


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=None)
    parser.add_argument("--runs", type=int, default=9)
    parser.add_argument("--deskew", action="store_true")
    args = parser.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "blocks_deskew_times.txt" if args.deskew else "blocks_times.txt")
    import keras_ocr_amd

    rng = np.random.default_rng(7)
    workloads = [("one column of 2048 one-line blocks", [bc.tall_column()[0]]),
                 ("32 pages of 64 lines", [bc.layout_page(rng, 64) for _ in range(32)]),
                 ("one page of 2048 boxes", [bc.layout_page(rng, 2048)])]
    ctx = keras_ocr_amd.Context(0)
    mode = "KOCR_LINES_BLOCKS | KOCR_LINES_DESKEW" if args.deskew else "KOCR_LINES_BLOCKS"
    lines = [f"kocr_group_lines with {mode}, profiler rows in ms: median (min .. max) of {args.runs} calls after a warm-up"]
    show = lambda rows: "; ".join(f"{row} {m:.3f} ({lo:.3f} .. {hi:.3f})" for row, (m, lo, hi) in rows.items())  # noqa: E731
    try:
        ctx.profile_enable(True)
        for name, pages in workloads:
            if args.deskew:
                blocks, rows = measure(ctx, [dc.rotated(p, DESKEW_ANGLE) for p in pages], args.runs, deskew=True)
                lines.append(f"{name}, rotated by {DESKEW_ANGLE:g} degrees: {blocks} blocks; {show(rows)}")
                blocks, rows = measure(ctx, pages, args.runs)
                lines.append(f"{name}, not rotated, plain block mode: {blocks} blocks; {show(rows)}")
                continue
            blocks, rows = measure(ctx, pages, args.runs)
            lines.append(f"{name}: {blocks} blocks; {show(rows)}")
    finally:
        ctx.profile_enable(False)
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
