#!/usr/bin/env python
"""Timing record of the XY-cut on the device ("Blocks"): the milliseconds of the profiler rows
blocks_cut and lines_pack (kocr_profile_report) for
  1. the worst case of the round loop, one column of 2048 one-line blocks (2047 cutting rounds),
  2. a batch of 32 pages of 64 lines laid out in columns and paragraphs,
  3. one page of 2048 boxes laid out in columns and paragraphs,
each after a warm-up call, as the median of several calls, with the statement's answer checked on the first.  Writes the
record to --out.  Needs a GPU; exits non-zero on the first failure.

usage: python scripts/time_blocks.py [--out profiles/blocks_times.txt] [--runs 9]"""
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


def measure(ctx, pages, runs):
    quads, offsets = bc.flatten(pages)
    want = bs.group_batch(pages)
    got = ctx.group_blocks(quads, offsets)  # warm-up, and the check
    assert all(np.array_equal(g, w) for g, w in zip(got, want)), "the device disagrees with the statement"
    rows = {"blocks_cut": [], "lines_pack": []}
    for _ in range(runs):
        ctx.profile_reset()
        ctx.group_blocks(quads, offsets)
        report = ctx.profile_report()
        for name, values in rows.items():
            assert report[name]["launches"] == 1, (name, report.get(name))
            values.append(report[name]["ms"])
    return int(want[2].sum()), {name: (statistics.median(v), min(v), max(v)) for name, v in rows.items()}


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "blocks_times.txt"))
    parser.add_argument("--runs", type=int, default=9)
    args = parser.parse_args()
    import keras_ocr_amd

    rng = np.random.default_rng(7)
    workloads = [("one column of 2048 one-line blocks", [bc.tall_column()[0]]),
                 ("32 pages of 64 lines", [bc.layout_page(rng, 64) for _ in range(32)]),
                 ("one page of 2048 boxes", [bc.layout_page(rng, 2048)])]
    ctx = keras_ocr_amd.Context(0)
    lines = [f"kocr_group_lines with KOCR_LINES_BLOCKS, profiler rows in ms: median (min .. max) of {args.runs} calls after a warm-up"]
    try:
        ctx.profile_enable(True)
        for name, pages in workloads:
            blocks, rows = measure(ctx, pages, args.runs)
            lines.append(f"{name}: {blocks} blocks; " + "; ".join(f"{row} {m:.3f} ({lo:.3f} .. {hi:.3f})" for row, (m, lo, hi) in rows.items()))
    finally:
        ctx.profile_enable(False)
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
