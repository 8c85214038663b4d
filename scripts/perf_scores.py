"""Developer probe: what the scores cost.  (a) the recogniser's tail on 512 crops -- the ctc_greedy row
of kocr_crnn_forward against the ctc_scores row of kocr_crnn_forward_scores, and the two calls' wall time; (b) the
bench-shaped pipeline (bench.py's headline: 32 pages, head calibrated to ~20 boxes per page) with return_scores off and
on, alternating, median of the rounds."""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import keras_ocr_amd as k
import bench

M = 512
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
ctx = k.Context(0)
crnn_w = k.weights.synthetic_crnn_weights(4321)
ctx.load_crnn(crnn_w)
ctx.set_stream(torch.cuda.current_stream().cuda_stream)
crops = torch.rand((M, 31, 200), dtype=torch.float32, device="cuda")
labels = torch.empty((M, 48), dtype=torch.int32, device="cuda")
logw = torch.empty((M,), dtype=torch.float32, device="cuda")
chars = torch.empty((M, 48), dtype=torch.float32, device="cuda")
calls = {"off": lambda: ctx.crnn_forward_device(crops.data_ptr(), M, labels.data_ptr()),
         "on": lambda: ctx.crnn_forward_scores_device(crops.data_ptr(), M, labels.data_ptr(), logw.data_ptr(), chars.data_ptr())}


def wall(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e3


for name, row in (("off", "ctc_greedy"), ("on", "ctc_scores")):
    ms = sorted(wall(calls[name]) for _ in range(ROUNDS))
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(5):
        calls[name]()
    rep = ctx.profile_report()
    ctx.profile_enable(False)
    print(f"CRNN {M} crops, scores {name}: {ms[len(ms) // 2]:.3f} ms (min {ms[0]:.3f}, max {ms[-1]:.3f}); "
          f"{row} {rep[row]['ms'] / rep[row]['launches'] * 1e3:.1f} us per launch")

# bench-shaped pipeline
pages = bench.make_pages(bench.BATCH, bench.SIDE, seed=4)
craft_w = k.weights.synthetic_craft_weights(1234)
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
pipe = k.pipeline.Pipeline(detector=k.detection.Detector(weights=best[1], ctx=ctx),
                           recognizer=k.recognition.Recognizer(weights=crnn_w, ctx=ctx), scale=bench.SCALE)
d_pages = torch.from_numpy(pages).cuda()
times = {False: [], True: []}
for r in range(ROUNDS + 1):
    for on in (False, True):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(3):
            out = pipe.recognize_device(d_pages.data_ptr(), bench.BATCH, bench.SIDE, bench.SIDE, return_scores=on)
        torch.cuda.synchronize()
        if r:  # round 0 warms up
            times[on].append((time.perf_counter() - t) / 3 * 1e3)
off, on = (sorted(times[f]) for f in (False, True))
words = sum(len(g) for g in out)
print(f"pipeline {bench.BATCH} pages, {words} words: scores off {off[len(off) // 2]:.2f} ms (min {off[0]:.2f}, max {off[-1]:.2f}), "
      f"on {on[len(on) // 2]:.2f} ms (min {on[0]:.2f}, max {on[-1]:.2f}); median difference "
      f"{on[len(on) // 2] - off[len(off) // 2]:+.2f} ms = {100 * (on[len(on) // 2] / off[len(off) // 2] - 1):+.2f} % of the step")
