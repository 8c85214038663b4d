"""Where the recogniser's backbone difference to the float32 oracle comes from: the crops of
tests/test_ctc_loss_gpu.py::test_backbone_matches_the_oracle through the tapped GPU forward, then the oracle's float32
forward RESTARTED from the GPU's own tensor after each stage.  The stage after which the difference to the GPU's features
collapses is the one that accounts for it.  Needs a GPU:  python scripts/crnn_backbone_error.py"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import keras_ocr_amd  # noqa: E402
from oracle import crnn as o  # noqa: E402
from tests import synth  # noqa: E402


def tail(w, stage, t):
    """the oracle's float32 forward from `stage`'s output t to the backbone features (recognition.py:268-319)"""
    t = torch.from_numpy(np.ascontiguousarray(t))
    M = t.shape[0]
    if stage == "keras":  # bn_7 in Keras layout (M, 50, 7, 512): the STN
        x = t.permute(0, 3, 1, 2)
        loc = o._conv(w, "stn_conv_2", o._conv(w, "stn_conv_1", x)).permute(0, 2, 3, 1).reshape(M, -1)
        loc = F.relu(loc @ o._t(w["stn_dense_1/kernel"]) + o._t(w["stn_dense_1/bias"]))
        theta = loc @ o._t(w["stn_dense_2/kernel"]) + o._t(w["stn_dense_2/bias"])
        t, stage = o.stn_transform(t, theta), "stn"
    if stage == "stn":
        t, stage = F.relu(t.reshape(M, 50, -1) @ o._t(w["fc_9/kernel"]) + o._t(w["fc_9/bias"])), "fc_9"
    if stage == "fc_9":
        t = t.reshape(M, 50, -1)
        t, stage = o._lstm(w, "lstm_10", t, False) + o._lstm(w, "lstm_10_back", t, True), "rnn_1"
    t = t.reshape(M, 50, -1)
    return torch.cat([o._lstm(w, "lstm_11", t, False), o._lstm(w, "lstm_11_back", t, True)], -1).numpy()


def main():
    torch.set_num_threads(16)
    w = keras_ocr_amd.weights.synthetic_crnn_weights(4321)
    x = np.stack([synth.text_page(31, 200, 3, seed=40 + i)[..., 0] / np.float32(255) for i in range(6)]).astype(np.float32)
    ctx = keras_ocr_amd.Context(0)
    ctx.load_crnn(w)
    ctx.crnn_set_taps(["*"])
    ctx.crnn_forward(x, return_probs=True)
    taps = ctx.crnn_taps()
    ctx.crnn_set_taps([])
    feats = taps["lstm_11"]["out"][0].reshape(6, 50, 256)
    ref = o.crnn_forward(w, x[..., None], return_intermediates=True)[1]["rnn_2"]
    print(f"GPU features vs the whole oracle forward:        {np.abs(feats - ref).max():.3g}")
    keras = "cells_to_keras" if "cells_to_keras" in taps else "crnn_to_keras"
    r1 = taps["lstm_10"]["out"][0].reshape(6, 50, 256)
    for label, stage, t in [("the conv stack (conv_1 .. conv_7)", "keras", taps[keras]["out"][0]),
                            ("the STN", "stn", taps["stn_sample"]["out"][0]),
                            ("fc_9", "fc_9", taps["fc_9"]["out"][0]),
                            ("lstm_10 (+ Add)", "rnn_1", r1[..., :128] + r1[..., 128:])]:
        print(f"oracle restarted from the GPU's output of {label:34s} {np.abs(feats - tail(w, stage, t)).max():.3g}")
    ctx.close()


if __name__ == "__main__":
    main()
