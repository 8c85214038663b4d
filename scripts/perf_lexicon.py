"""Developer probe: what the lexicon match costs (output kept as profiles/lexicon_stats.txt).
  perf_lexicon.py run V [same]   under `rocprofv3 --kernel-trace --stats`: 2 + 5 rounds of kocr_crnn_lexicon (top_words 5) on 704
                                 device-resident crops against V random words of 3 .. 12 labels (`same`: every label 0 -- the
                                 same instructions, but the per-lane gather lq_t(label) hits one LDS address: no bank conflicts);
  perf_lexicon.py pairs          under rocprofv3 likewise: the route without the feature, Context.ctc_batch_cost on the
                                 replicated (crop, word) pairs of 704 crops x 64 of those words (45 056 rows: ctc_loss_kernel,
                                 unchanged by the feature);
  perf_lexicon.py report TAG CSV one line from a run's kernel statistics (every round counts, the two warm-up rounds too);
  perf_lexicon.py pipeline       not under a profiler: Pipeline.recognize on bench.py's 32-page batch with the match off and
                                 with 10 000 words (top 5), alternating, median of 7."""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M, ROUNDS, K, PAIR_WORDS = 704, 7, 5, 64


def words(v, same=False):
    rng = np.random.default_rng(7)
    lengths = rng.integers(3, 13, v).astype(np.int32)
    labels = rng.integers(0, 36, (v, 12)).astype(np.int32)
    return (np.zeros_like(labels) if same else labels), lengths


def crops():
    import bench

    return bench.make_crops(M)


def run(v, same):
    import torch
    import keras_ocr_amd as k

    ctx = k.Context(0)
    ctx.load_crnn(k.weights.synthetic_crnn_weights(4321))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ctx.set_lexicon(*words(v, same))
    x = torch.from_numpy(crops()).cuda()
    index = torch.empty((M, K), dtype=torch.int32, device="cuda")
    logp = torch.empty((M, K), dtype=torch.float32, device="cuda")
    for _ in range(ROUNDS):
        ctx.crnn_lexicon_device(x.data_ptr(), M, K, index.data_ptr(), logp.data_ptr())
    torch.cuda.synchronize()
    ctx.close()


def pairs():
    import keras_ocr_amd as k

    ctx = k.Context(0)
    ctx.load_crnn(k.weights.synthetic_crnn_weights(4321))
    _, probs = ctx.crnn_forward(crops(), return_probs=True)
    labels, lengths = words(PAIR_WORDS)
    y = np.repeat(probs, PAIR_WORDS, axis=0)
    lab, ln = np.tile(labels, (M, 1)), np.tile(lengths, M)
    for _ in range(3):
        ctx.ctc_batch_cost(y, lab, ln, np.full(len(y), probs.shape[1]))
    ctx.close()


def report(tag, path):
    rows = {r["Name"]: (int(r["Calls"]), float(r["TotalDurationNs"])) for r in csv.DictReader(open(path))}

    def avg(key):
        hit = [v for name, v in rows.items() if key in name]
        return sum(v[1] for v in hit) / max(1, sum(v[0] for v in hit)) / 1e3, sum(v[0] for v in hit)

    if tag == "pairs":
        us, calls = avg("ctc_loss_kernel")
        n = M * PAIR_WORDS
        print(f"pairs   M {M} x {PAIR_WORDS} words = {n} rows: ctc_loss_kernel {us:10.1f} us  = {us * 1e3 / n:8.2f} ns per pair  [{calls} calls]")
        return
    v = int(tag.split("-")[0])
    _, lengths = words(v)
    updates = M * float((2 * lengths + 1).sum()) * 48  # states x frames, the masked corners included
    lq, calls = avg("lexicon_logq_kernel")
    sc, _ = avg("lexicon_score_kernel")
    se, _ = avg("lexicon_select_kernel")
    print(f"lexicon M {M} V {tag:>10} K {K}: lexicon_logq {lq:8.1f} us  lexicon_score {sc:10.1f} us  lexicon_select {se:9.1f} us  "
          f"all three {(lq + sc + se) * 1e3 / (M * v):7.3f} ns per pair  score {updates / sc / 1e3:7.1f} G state updates/s  [{calls} calls]")


def pipeline():
    import torch
    import keras_ocr_amd as k
    import bench

    ctx = k.Context(0)
    craft_w, crnn_w = k.weights.synthetic_craft_weights(1234), k.weights.synthetic_crnn_weights(4321)
    pages = bench.make_pages(bench.BATCH, bench.SIDE, seed=4)
    ctx.load_craft(craft_w)
    raw = ctx.craft_forward(ctx.resize_pad(pages[:8], (bench.SIDE * bench.SCALE, bench.SIDE * bench.SCALE)))
    best = None
    for frac in (0.012, 0.0095, 0.008, 0.007, 0.0062, 0.0055, 0.0049, 0.0044, 0.0039, 0.0034, 0.003, 0.0025):
        cand = k.weights.calibrate_craft_head(craft_w, raw, text_frac=frac, link_frac=frac / 3, top_q=0.9999)
        a = cand["conv_cls.8.weight"].reshape(2, -1)[:, :1] / craft_w["conv_cls.8.weight"].reshape(2, -1)[:, :1]
        heat = (raw - craft_w["conv_cls.8.bias"]) * a.ravel() + cand["conv_cls.8.bias"]
        nb = np.mean([len(b) for b in ctx.get_boxes(heat.astype(np.float32))])
        if best is None or abs(nb - bench.WORDS_PER_PAGE) < abs(best[0] - bench.WORDS_PER_PAGE):
            best = (nb, cand)
    rec = k.recognition.Recognizer(weights=crnn_w, ctx=ctx)
    pipe = k.pipeline.Pipeline(detector=k.detection.Detector(weights=best[1], ctx=ctx), recognizer=rec, scale=bench.SCALE)
    labels, lengths = words(10000)
    rec.set_lexicon(sorted({"".join(rec.alphabet[c] for c in row[:n]) for row, n in zip(labels, lengths)}))
    times = {None: [], K: []}
    for r in range(8):
        for top in (None, K):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = pipe.recognize(pages, recognition_kwargs={"lexicon_top": top})
            dt = time.perf_counter() - t0
            if r:
                times[top].append(dt * 1e3)
    n = sum(len(g) for g in out)
    off, on = np.median(times[None]), np.median(times[K])
    print(f"pipeline {bench.BATCH} pages, {n} crops, V {len(rec.lexicon)} K {K}: recognize off {off:7.2f} ms (min {min(times[None]):7.2f}, max "
          f"{max(times[None]):7.2f})  on {on:7.2f} ms (min {min(times[K]):7.2f}, max {max(times[K]):7.2f})  +{on - off:6.2f} ms  [median of 7, alternating]")
    ctx.close()


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "run":
        run(int(sys.argv[2]), len(sys.argv) > 3 and sys.argv[3] == "same")
    elif mode == "pairs":
        pairs()
    elif mode == "report":
        report(sys.argv[2], sys.argv[3])
    else:
        pipeline()
