"""Developer probe: what the decode launches cost with and without a character set ("Character sets").
  perf_charsets.py off     N rounds of kocr_crnn_forward, kocr_crnn_forward_scores, kocr_crnn_beam(16, top_paths 3) and
                           kocr_crnn_lexicon(top_words 3, 1000 words) on 512 device-resident crops with the switch off -- this
                           mode runs on a tree without the feature as well;
  perf_charsets.py SIZE    the same under a set of the first SIZE classes (10: the digits).
One line per decode row of the library's own profiler (kocr_profile_report: HIP events around every launch): ctc_greedy,
ctc_scores, ctc_beam, lexicon_logq, lexicon_score, lexicon_select -- launches and the mean time of one."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M, N, B, K, V = 512, 10, 16, 3, 1000
ROWS = ("ctc_greedy", "ctc_scores", "ctc_beam", "lexicon_logq", "lexicon_score", "lexicon_select")


def run(size):
    import torch
    import keras_ocr_amd as k

    ctx = k.Context(0)
    ctx.load_crnn(k.weights.synthetic_crnn_weights(4321))
    classes = ctx.crnn_classes()
    rng = np.random.default_rng(7)
    lengths = rng.integers(3, 11, V).astype(np.int32)
    words = np.full((V, 10), -1, np.int32)
    for v, n in enumerate(lengths):
        words[v, :n] = rng.integers(0, classes - 1, n)
    ctx.set_lexicon(words, lengths)
    if size:
        allowed = np.zeros((1, classes - 1), np.uint8)
        allowed[0, :size] = 1
        ctx.set_charsets(allowed)
        ctx.set_charset(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    crops = torch.rand((M, 31, 200), dtype=torch.float32, device="cuda")
    labels = torch.empty((M, 48), dtype=torch.int32, device="cuda")
    logw = torch.empty((M,), dtype=torch.float32, device="cuda")
    chars = torch.empty((M, 48), dtype=torch.float32, device="cuda")
    beam_labels = torch.empty((M, K, 48), dtype=torch.int32, device="cuda")
    beam_logp = torch.empty((M, K), dtype=torch.float32, device="cuda")
    index = torch.empty((M, K), dtype=torch.int32, device="cuda")
    logp = torch.empty((M, K), dtype=torch.float32, device="cuda")

    def round_():
        ctx.crnn_forward_device(crops.data_ptr(), M, labels.data_ptr())
        ctx.crnn_forward_scores_device(crops.data_ptr(), M, labels.data_ptr(), logw.data_ptr(), chars.data_ptr())
        ctx.crnn_beam_device(crops.data_ptr(), M, B, K, beam_labels.data_ptr(), beam_logp.data_ptr())
        ctx.crnn_lexicon_device(crops.data_ptr(), M, K, index.data_ptr(), logp.data_ptr())

    for _ in range(2):  # warm up, outside the figures
        round_()
    torch.cuda.synchronize()
    ctx.profile_enable(True)
    ctx.profile_reset()
    for _ in range(N):
        round_()
    torch.cuda.synchronize()
    rows = ctx.profile_report()
    ctx.profile_enable(False)
    what = f"set of {size} classes" if size else "switch off"
    print(f"M {M}  beam_width {B}  top_paths {K}  lexicon {V} words  {what}:")
    for name in ROWS:
        r = rows[name]
        print(f"  {name:15s} {r['launches']:4d} launches  {1e3 * r['ms'] / r['launches']:9.1f} us each")
    ctx.close()


if __name__ == "__main__":
    run(0 if sys.argv[1] == "off" else int(sys.argv[1]))
