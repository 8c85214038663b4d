#!/usr/bin/env python
"""Timing record of the table grid on the device ("Tables"): the milliseconds of the profiler rows
table_grid and lines_pack (kocr_profile_report) for
  1. a batch of 32 pages of 64 quads in a grid of 4 columns (about 16 x 4; some cells empty, some spanning),
  2. one grid page of 2048 quads,
  3. one page of 2048 quads in a single row (2047 separators, the most a page can have),
each after a warm-up call, as the median of several calls, with the statement's answer checked on the first; and, from
the same run, plain block mode (rows blocks_cut, lines_pack) on the same boxes as the yardstick.  Writes the record to
--out.  Needs a GPU; exits non-zero on the first failure.

usage: python scripts/time_table.py [--out profiles/table_times.txt] [--runs 9]"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import blocks_statement as bs  # noqa: E402
from tests import table_cases as tc  # noqa: E402
from tests import table_statement as ts  # noqa: E402

TABLE_ROWS = ("table_grid", "lines_pack")
BLOCK_ROWS = ("blocks_cut", "lines_pack")


def timed(ctx, call, names, runs):
    rows = {name: [] for name in names}
    for _ in range(runs):
        ctx.profile_reset()
        call()
        report = ctx.profile_report()
        for name, values in rows.items():
            assert report[name]["launches"] == 1, (name, report.get(name))
            values.append(report[name]["ms"])
    return {name: (statistics.median(v), min(v), max(v)) for name, v in rows.items()}


def measure(ctx, pages, runs):
    """-> (bands, table rows, blocks, block rows) of one workload"""
    quads, offsets = tc.flatten(pages)
    wants = [ts.table_page(p) for p in pages]
    got = ctx.group_table(quads, offsets)  # warm-up, and the check
    assert np.array_equal(got[0], np.concatenate([w["row"] for w in wants])) and np.array_equal(got[1], np.concatenate([w["col0"] for w in wants])) \
        and np.array_equal(got[2], np.concatenate([w["col1"] for w in wants])), "the device disagrees with the statement"
    assert got[5].tobytes() == b"".join(w["row_boxes"].tobytes() for w in wants) and got[6].tobytes() == b"".join(w["col_boxes"].tobytes() for w in wants)
    table = timed(ctx, lambda: ctx.group_table(quads, offsets), TABLE_ROWS, runs)
    want = bs.group_batch(pages)
    assert all(np.array_equal(g, w) for g, w in zip(ctx.group_blocks(quads, offsets), want)), "block mode disagrees with its statement"
    blocks = timed(ctx, lambda: ctx.group_blocks(quads, offsets), BLOCK_ROWS, runs)
    return int(sum(w["R"] + w["S"] + 1 for w in wants)), table, int(want[2].sum()), blocks


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "table_times.txt"))
    parser.add_argument("--runs", type=int, default=9)
    args = parser.parse_args()
    import keras_ocr_amd

    workloads = [("32 pages of 64 quads in 4 columns", [tc.grid_page(64, 100 + k, cols=4) for k in range(32)]),
                 ("one grid page of 2048 quads", [tc.grid_page(2048, 0)]),
                 ("one page of 2048 quads in a single row", [tc.single_row()])]
    ctx = keras_ocr_amd.Context(0)
    lines = [f"kocr_group_lines with KOCR_LINES_TABLE, profiler rows in ms: median (min .. max) of {args.runs} calls after a warm-up"]
    show = lambda rows: "; ".join(f"{row} {m:.3f} ({lo:.3f} .. {hi:.3f})" for row, (m, lo, hi) in rows.items())  # noqa: E731
    try:
        ctx.profile_enable(True)
        for name, pages in workloads:
            bands, table, blocks, cut = measure(ctx, pages, args.runs)
            lines.append(f"{name}: {bands} bands; {show(table)}")
            lines.append(f"{name}, plain block mode on the same boxes: {blocks} blocks; {show(cut)}")
    finally:
        ctx.profile_enable(False)
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
