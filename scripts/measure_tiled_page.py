"""Measures Pipeline.recognize_tiled on one A4 page at 300 dpi (2480 x 3508, a synthetic text page repeated 4 x 4) at one
scale: wall time per call, and the profiler rows of the two tile copies, the resize and the detector.  Writes one JSON file.
    python scripts/measure_tiled_page.py --scale 2 --out profiles/tiled_a4_scale2.json
Random-init weights with the head calibrated on the GPU's own heat-map of the base page, as bench.py does: the numbers say
what the path costs, not how well it reads."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=2)
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--overlap", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    import keras_ocr_amd as k
    from tests import synth

    scale = int(args.scale) if float(args.scale).is_integer() else args.scale
    base = synth.text_page(877, 620, 60, seed=7)
    page = np.ascontiguousarray(np.tile(base, (4, 4, 1)))
    assert page.shape == (3508, 2480, 3)
    ctx = k.Context(0)
    craft_w = k.weights.synthetic_craft_weights(1234)
    ctx.load_craft(craft_w)
    dh, dw = int(base.shape[0] * scale), int(base.shape[1] * scale)
    sample = ctx.resize_pad(base[None], (dw, dh), out_hw=((dh + 31) // 32 * 32, (dw + 31) // 32 * 32))
    craft_w = k.weights.calibrate_craft_head(craft_w, ctx.craft_forward(sample), text_frac=0.01, link_frac=0.0033, top_q=0.9999)
    det = k.detection.Detector(weights=craft_w, ctx=ctx)
    rec = k.recognition.Recognizer(weights=k.weights.synthetic_crnn_weights(4321), ctx=ctx)
    pipe = k.pipeline.Pipeline(detector=det, recognizer=rec)
    plan = k.tools.tile_plan(int(page.shape[0] * scale), int(page.shape[1] * scale), args.tile, args.overlap)

    def step():
        return pipe.recognize_tiled([page], tile=args.tile, overlap=args.overlap, scale=scale)

    words = len(step()[0])  # warm-up: arenas sized, kernels loaded
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        step()
        times.append(time.perf_counter() - t0)
    ctx.profile_reset()
    ctx.profile_enable(True)
    step()
    rows = {name: row for name, row in ctx.profile_report().items() if row["launches"]}
    ctx.profile_enable(False)

    def rate(name):
        row = rows[name]
        return {"launches": row["launches"], "ms": row["ms"], "bytes": row["bytes"], "GB_per_s": row["bytes"] / row["ms"] / 1e6}

    conv = {name: row for name, row in rows.items() if name.startswith("conv_")}
    result = {
        "page": list(page.shape[:2]), "scale": scale, "tile": args.tile, "overlap": args.overlap,
        "detector_input": [int(page.shape[0] * scale), int(page.shape[1] * scale)], "canvas": list(plan.canvas),
        "tiles": list(plan.counts), "words": words, "wall_s": times, "wall_s_median": float(np.median(times)),
        "tile_gather": rate("tile_gather"), "heat_stitch": rate("heat_stitch"), "resize_pad": rate("resize_pad"),
        "detector_conv_ms": sum(row["ms"] for row in conv.values()),
        "detector_conv_tflops": sum(row["flops"] for row in conv.values()) / sum(row["ms"] for row in conv.values()) / 1e9,
        "all_rows_ms": sum(row["ms"] for row in rows.values()),
        "rows_ms": {name: round(row["ms"], 4) for name, row in sorted(rows.items(), key=lambda kv: -kv[1]["ms"])},
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({key: result[key] for key in ("scale", "canvas", "tiles", "words", "wall_s_median", "tile_gather", "heat_stitch",
                                                   "detector_conv_ms")}))
    ctx.close()


if __name__ == "__main__":
    main()
