#!/usr/bin/env python
"""Timing record of the windowed route ("Long words"): per workload the milliseconds of the profiler rows
window_plan, window_stitch and ctc_scores_ragged (kocr_profile_report; window_stitch runs once per recogniser batch, the row is
their sum) in profiled calls, and the host clock around the whole Context.recognize_boxes_windowed call with the profiler off,
each as the median (min .. max) of several calls after a warm-up, for
  (a) 512 short boxes, every K = 1 -- with Context.recognize_boxes(return_scores=True) on the same boxes beside it, measured in
      the same run on THIS build (not on an earlier commit): the windowed route should cost that plus the plan and the stitch;
  (b) 26 boxes of 1661 x 8 at overlap 40: K = 40 each, 1040 windows, 1608 frames a word;
  (c) one page of 64 boxes with K = 4.
Random-init weights with fc_12 doubled; the K = 1 rows of (a) are checked against recognize_boxes, bit for bit, on the first
call.  Writes the record to --out.  Needs a GPU; exits non-zero on the first failure.

usage: python scripts/time_windows.py [--out profiles/windows_times.txt] [--runs 9]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import windows_cases as wc  # noqa: E402
from tests import windows_statement as ws  # noqa: E402

ROWS = ("window_plan", "window_stitch", "ctc_scores_ragged")


def spread(values):
    return f"{statistics.median(values):.3f} ({min(values):.3f} .. {max(values):.3f})"


def profiled(ctx, call, names, runs):
    rows = {name: [] for name in names}
    ctx.profile_enable(True)
    try:
        for _ in range(runs):
            ctx.profile_reset()
            call()
            report = ctx.profile_report()
            for name, values in rows.items():
                values.append(report[name]["ms"])
    finally:
        ctx.profile_enable(False)
    return "; ".join(f"{name} {spread(v)}" for name, v in rows.items())


def wall(call, runs):
    values = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        values.append((time.perf_counter() - t0) * 1e3)
    return spread(values)


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "windows_times.txt"))
    parser.add_argument("--runs", type=int, default=9)
    args = parser.parse_args()
    import keras_ocr_amd

    rng = np.random.default_rng(3)
    short = np.stack([wc.rect(int(rng.integers(0, 330)), int(rng.integers(0, 95)), int(rng.integers(40, 70)), int(rng.integers(12, 24)))
                      for _ in range(512)])
    edge = np.stack([wc.long_box(4 + 10 * i) for i in range(26)])
    four = np.stack([wc.rect(10 + 340 * (i % 2), 4 + 18 * (i // 2), 270, 14) for i in range(64)])
    workloads = [("(a) 512 short boxes on a 120 x 400 page", wc.page(), short),
                 ("(b) 26 boxes of 1661 x 8 on a 270 x 1700 page", wc.page(270, 1700, seed=11), edge),
                 ("(c) 64 boxes of 270 x 14 on a 600 x 700 page", wc.page(600, 700, seed=12), four)]
    ctx = keras_ocr_amd.Context(0)
    lines = [f"kocr_recognize_boxes_windowed at aspect 10, overlap 40; ms: median (min .. max) of {args.runs} calls after a warm-up; profiler "
             "rows from profiled calls, whole calls by the host clock with the profiler off (image upload and result download included)"]
    try:
        weights = keras_ocr_amd.weights.synthetic_crnn_weights(4321)
        weights["fc_12/kernel"] = weights["fc_12/kernel"] * np.float32(2)
        weights["fc_12/bias"] = weights["fc_12/bias"] * np.float32(2)
        ctx.load_crnn(weights)
        for name, page, boxes in workloads:
            k, _, _, frames = ws.plan_boxes(boxes)
            run = lambda: ctx.recognize_boxes_windowed(page[None], [boxes])  # noqa: E731
            got = run()  # warm-up, and the check
            assert got[4].tolist() == k.tolist() and got[3].tolist() == frames.tolist(), "the device disagrees with the statement's plan"
            lines.append(f"{name}: {len(boxes)} words, {int(k.sum())} windows, {int(frames.sum())} frames, rows {int(frames.max())} wide")
            lines.append(f"  {profiled(ctx, run, ROWS, args.runs)}")
            lines.append(f"  whole call {wall(run, args.runs)}")
            if (k == 1).all():
                plain = lambda: ctx.recognize_boxes(page[None], [boxes], return_scores=True)  # noqa: E731
                want = plain()
                assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes(), \
                    "K = 1 rows differ from recognize_boxes"
                lines.append(f"  recognize_boxes(return_scores=True) on the same boxes, this build in the same run (not an earlier commit's number): {profiled(ctx, plain, ('ctc_scores',), args.runs)}; "
                             f"whole call {wall(plain, args.runs)}")
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
