"""Developer probe: what the pattern launches cost next to the other decodes ("Patterns").
  perf_patterns.py off      N rounds of kocr_crnn_forward, kocr_crnn_forward_scores, kocr_crnn_beam(16, top_paths 3) and
                            kocr_crnn_lexicon(top_words 3, 1000 words) on 512 device-resident crops of a 96-class recogniser
                            with the switch off -- this mode runs on a tree without the feature as well;
  perf_patterns.py REGEX    the same rounds, each followed by kocr_crnn_pattern under that regular expression over the digits,
                            the letters, the capitals, the punctuation and the space (date: \\d{2}/\\d{2}/\\d{4}; .{0,40}).
One line per decode row of the library's own profiler (kocr_profile_report: HIP events around every launch): ctc_greedy,
ctc_scores, ctc_beam, lexicon_logq, lexicon_score, lexicon_select, pattern_viterbi, pattern_rescore -- launches and the mean
time of one.  Under a pattern lexicon_logq runs twice per round (the lexicon's and the pattern's)."""
import os
import string
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M, N, B, K, V, C = 512, 10, 16, 3, 1000, 96
ROWS = ("ctc_greedy", "ctc_scores", "ctc_beam", "lexicon_logq", "lexicon_score", "lexicon_select", "pattern_viterbi", "pattern_rescore")
ALPHABET = string.digits + string.ascii_lowercase + string.ascii_uppercase + string.punctuation + " "


def run(regex):
    import torch
    import keras_ocr_amd as k

    ctx = k.Context(0)
    ctx.load_crnn(k.weights.synthetic_crnn_weights(4321, n_classes=C))
    rng = np.random.default_rng(7)
    lengths = rng.integers(3, 11, V).astype(np.int32)
    words = np.full((V, 10), -1, np.int32)
    for v, n in enumerate(lengths):
        words[v, :n] = rng.integers(0, C - 1, n)
    ctx.set_lexicon(words, lengths)
    what = "switch off"
    if regex:
        from keras_ocr_amd import patterns

        pats = patterns.Patterns(ALPHABET, {"p": regex})
        ctx.set_patterns(*pats.tables())
        ctx.set_pattern(0)
        what = f"pattern {regex} ({len(pats.delta[0])} states, {patterns.label_nodes(pats.delta[0])} label nodes)"
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    crops = torch.rand((M, 31, 200), dtype=torch.float32, device="cuda")
    labels = torch.empty((M, 48), dtype=torch.int32, device="cuda")
    logw = torch.empty((M,), dtype=torch.float32, device="cuda")
    chars = torch.empty((M, 48), dtype=torch.float32, device="cuda")
    beam_labels = torch.empty((M, K, 48), dtype=torch.int32, device="cuda")
    beam_logp = torch.empty((M, K), dtype=torch.float32, device="cuda")
    index = torch.empty((M, K), dtype=torch.int32, device="cuda")
    logp = torch.empty((M, K), dtype=torch.float32, device="cuda")
    pat_labels = torch.empty((M, 48), dtype=torch.int32, device="cuda")
    pat_path = torch.empty((M,), dtype=torch.float32, device="cuda")
    pat_prob = torch.empty((M,), dtype=torch.float32, device="cuda")

    def round_():
        ctx.crnn_forward_device(crops.data_ptr(), M, labels.data_ptr())
        ctx.crnn_forward_scores_device(crops.data_ptr(), M, labels.data_ptr(), logw.data_ptr(), chars.data_ptr())
        ctx.crnn_beam_device(crops.data_ptr(), M, B, K, beam_labels.data_ptr(), beam_logp.data_ptr())
        ctx.crnn_lexicon_device(crops.data_ptr(), M, K, index.data_ptr(), logp.data_ptr())
        if regex:
            ctx.crnn_pattern_device(crops.data_ptr(), M, pat_labels.data_ptr(), pat_path.data_ptr(), pat_prob.data_ptr())

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
    print(f"M {M}  classes {C}  beam_width {B}  top_paths {K}  lexicon {V} words  {what}:")
    for name in ROWS:
        if name in rows:
            r = rows[name]
            print(f"  {name:15s} {r['launches']:4d} launches  {1e3 * r['ms'] / r['launches']:9.1f} us each")
    if regex:
        fitted = int(torch.isfinite(pat_prob).sum())
        print(f"  {fitted} of {M} crops have a reading the pattern accepts")
    ctx.close()


if __name__ == "__main__":
    run(None if sys.argv[1] == "off" else sys.argv[1])
