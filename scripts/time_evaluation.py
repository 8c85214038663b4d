#!/usr/bin/env python
"""Timing record of evaluation on the device ("Evaluation"): on the benchmark's 32 pages of 768 x 768
(bench.make_pages, the detector head calibrated as bench.py calibrates it), with truths derived from the predictions by
jitter, the wall time of
  1. Pipeline.recognize,
  2. evaluation.score on the host,
  3. evaluation.score on the device, with and without the results dictionary,
each after warm-up, as the median of several runs, plus the per-kernel milliseconds of the device path from
kocr_profile_report.  Writes the record to --out.  Needs a GPU; runs its GPU work once and exits non-zero on the first failure.

usage: python scripts/time_evaluation.py [--out profiles/r07_evaluation.txt] [--host-runs 3] [--runs 9]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the page generator and the workload's constants)


def calibrated_pipeline(k, ctx):
    """the pipeline of bench.py: synthetic weights, the head calibrated to about bench.WORDS_PER_PAGE boxes per page.
    bench.py keeps its calibration inside main(), where it cannot be imported, and bench.py does not change for this
    script: the loop is restated here, and the record names the words found per page, where a drift between the two would
    show."""
    craft_w = k.weights.synthetic_craft_weights(1234)
    crnn_w = k.weights.synthetic_crnn_weights(4321)
    ctx.load_craft(craft_w)
    sample = ctx.resize_pad(bench.make_pages(8, bench.SIDE, seed=4), (bench.SIDE * bench.SCALE, bench.SIDE * bench.SCALE))
    raw = ctx.craft_forward(sample)
    best = None
    for frac in (0.012, 0.0095, 0.008, 0.007, 0.0062, 0.0055, 0.0049, 0.0044, 0.0039, 0.0034, 0.003, 0.0025):
        cand = k.weights.calibrate_craft_head(craft_w, raw, text_frac=frac, link_frac=frac / 3, top_q=0.9999)
        a = cand["conv_cls.8.weight"].reshape(2, -1)[:, :1] / craft_w["conv_cls.8.weight"].reshape(2, -1)[:, :1]
        heat = (raw - craft_w["conv_cls.8.bias"]) * a.ravel() + cand["conv_cls.8.bias"]
        nb = np.mean([len(b) for b in ctx.get_boxes(heat.astype(np.float32))])
        if best is None or abs(nb - bench.WORDS_PER_PAGE) < abs(best[0] - bench.WORDS_PER_PAGE):
            best = (nb, cand)
    det = k.detection.Detector(weights=best[1], ctx=ctx)
    rec = k.recognition.Recognizer(weights=crnn_w, ctx=ctx)
    return k.pipeline.Pipeline(detector=det, recognizer=rec, scale=bench.SCALE)


def truths_from(predictions, seed=1):
    """labelled pages from predictions: every word's box jittered by up to 3 px, one in ten words dropped, one in ten
    ignored, one text in five edited"""
    rng = np.random.default_rng(seed)
    true = {}
    for i, group in enumerate(predictions):
        anns = []
        for text, box in group:
            if rng.random() < 0.1:
                continue
            ann = {"text": text if rng.random() < 0.8 else ("x" + text[1:] if text else "x"), "vertices": box + rng.uniform(-3, 3, box.shape).astype(np.float32)}
            if rng.random() < 0.1:
                ann["ignore"] = True
            anns.append(ann)
        true[i] = anns
    return true


def median_seconds(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_evaluation.txt"))
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--host-runs", type=int, default=3)
    args = ap.parse_args()

    import keras_ocr_amd as k
    from keras_ocr_amd import evaluation

    ctx = k.Context(0)
    pipe = calibrated_pipeline(k, ctx)
    pages = bench.make_pages(bench.BATCH, bench.SIDE, seed=4)
    predictions = pipe.recognize(pages)
    pred = {i: [{"text": t, "vertices": b} for t, b in group] for i, group in enumerate(predictions)}
    true = truths_from(predictions)
    pairs = sum(len(true[i]) * len(pred[i]) for i in true)

    want = evaluation.score(true, pred)
    got = evaluation.score(true, pred, ctx=ctx)
    if got != want:
        raise SystemExit("time_evaluation: the device path does not return what the host path returns")
    if evaluation.score(true, pred, ctx=ctx, return_results=False) != (None, want[1]):
        raise SystemExit("time_evaluation: return_results=False disagrees")

    t_rec = median_seconds(lambda: pipe.recognize(pages), args.runs, 2)
    t_host = median_seconds(lambda: evaluation.score(true, pred), args.host_runs, 1)
    t_dev = median_seconds(lambda: evaluation.score(true, pred, ctx=ctx), args.runs, 2)
    t_cnt = median_seconds(lambda: evaluation.score(true, pred, ctx=ctx, return_results=False), args.runs, 2)
    ctx.profile_reset()
    ctx.profile_enable(True)
    for _ in range(args.runs):
        evaluation.score(true, pred, ctx=ctx)
    rows = {name: row for name, row in ctx.profile_report().items() if name.startswith("eval_")}
    ctx.profile_enable(False)
    ctx.close()

    def fmt(t):
        return f"{t[0] * 1e3:10.3f} ms  (min {t[1] * 1e3:.3f}, max {t[2] * 1e3:.3f})"

    lines = [
        "evaluation on the device: timing record (scripts/time_evaluation.py)",
        f"{bench.BATCH} pages of {bench.SIDE} x {bench.SIDE}, {sum(len(g) for g in predictions)} predicted words "
        f"({sum(len(g) for g in predictions) / bench.BATCH:.1f} per page; bench.py aims at {bench.WORDS_PER_PAGE}), "
        f"{sum(len(v) for v in true.values())} truths, {pairs} (truth, prediction) pairs",
        f"precision / recall {want[1][0]:.4f} / {want[1][1]:.4f}; device result == host result: yes",
        f"medians of {args.runs} runs after 2 warm-up runs (host score: {args.host_runs} runs after 1); wall time of the Python call",
        "",
        f"Pipeline.recognize (host arrays in, strings out)     {fmt(t_rec)}",
        f"evaluation.score, host path                          {fmt(t_host)}",
        f"evaluation.score, ctx, results dictionary            {fmt(t_dev)}",
        f"evaluation.score, ctx, return_results=False          {fmt(t_cnt)}",
        "",
        f"host / device (with dictionary)      {t_host[0] / t_dev[0]:8.1f} x",
        f"host / device (counts only)          {t_host[0] / t_cnt[0]:8.1f} x",
        f"device scoring with dictionary / recognize  {t_dev[0] / t_rec[0]:6.3f}  "
        f"({'less' if t_dev[0] < t_rec[0] else 'NOT less'} than the recognize call it scores)",
        "",
        f"kernels (kocr_profile_report, mean of {args.runs} calls):",
    ]
    for name in ("eval_iou", "eval_text", "eval_reduce"):
        row = rows.get(name)
        if row is None:
            raise SystemExit(f"time_evaluation: no profiler row {name}")
        lines.append(f"  {name:12s} {row['ms'] / max(1, row['launches']):8.4f} ms / launch  ({row['launches']} launches)")
    kernel_ms = sum(r["ms"] / max(1, r["launches"]) for r in rows.values())
    lines.append(f"  the three together {kernel_ms:.4f} ms of the {t_cnt[0] * 1e3:.3f} ms call: the rest is the host's flattening of the "
                 "dictionaries, staging and, with the dictionary, its assembly")
    if not t_dev[0] < t_host[0]:
        lines.append("REQUIREMENT MISSED: the device path is not faster than the host path")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    if not t_dev[0] < t_host[0]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
