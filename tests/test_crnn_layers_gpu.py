"""Every launch of the CRNN recogniser forward, in its real schedule, against a float64 statement of that launch ON THE
GPU'S OWN INPUT (kocr_crnn_set_taps records what each launch read and wrote): errors do not compound, and each launch is
judged by the bound of the kernel family that ran it (tests/layer_bounds.py, tests/crnn_layer_check.py):

    convolutions / GEMMs      the detector's family bounds (Winograd 5e-6 with the +-3-column window, direct split kernels
                              and conv_k5 1.5e-6, conv_mfma K 2^-24), pooled outputs to the pooled bound
    crnn_conv1_cells          gamma_10 (a 9-term fp32 fma chain from the bias)
    dense_splitk              gamma_475 (448-term chunks, 25 partials, the bias)
    stn_sample                float64 bilinear interpolation at the corners the GPU chose
    lstm recurrences          teacher-forced running bound (oracle.crnn.lstm_teacher_forced)
    ctc                       (C + 8) 2^-24 relative to the float64 softmax of the GPU's logits; labels exact
    permutes, poolings        exact

The float64 statements are built from the Keras weight dict (oracle.crnn.layer_f64), and every tapped tensor is mapped to
Keras orientation first, so a wrong kernel flip, BN fold or LSTM stacking in crnn_load fails here.  Each launch's input must
equal, bit for bit, what its producer wrote; every max-|x| slot is an upper bound of its crop's max |x|, at most twice it,
exactly 0 for an all-zero tensor; the gutters of the cell grid and the padding columns of the 52-wide layout are exactly 0;
taps change no result."""
import os

import numpy as np
import pytest

from oracle import crnn as ocrnn
from tests import crnn_layer_check as chk
from tests.layer_bounds import family, kernel_row, pool2

pytestmark = pytest.mark.gpu

# natural-orientation geometry of the three conv levels: (crop rows, crop columns)
LEVELS = {1: (31, 200), 2: (15, 100), 3: (7, 50)}
LEVEL_OF = {"conv_1": 1, "conv_2": 1, "conv_3": 1, "conv_4": 2, "conv_5": 2, "conv_6": 3, "conv_7": 3}
IN_LEVEL = {"conv_1": 1, "conv_2": 1, "conv_3": 1, "conv_4": 2, "conv_5": 2, "conv_6": 3, "conv_7": 3,
            "pool_3": 1, "pool_5": 2, "cells_to_keras": 3, "crnn_to_keras": 3}
POOLED = {"conv_3": 2, "conv_5": 3, "pool_3": 2, "pool_5": 3}


def _crops(M, seed=7):
    """random [0, 1], all-zero, all-one and single-hot-pixel crops, mixed (crop m is of kind m % 4)"""
    rng = np.random.default_rng(seed + M)
    x = np.zeros((M, 31, 200), np.float32)
    for m in range(M):
        kind = m % 4
        if kind == 0:
            x[m] = rng.random((31, 200), dtype=np.float32)
        elif kind == 2:
            x[m] = 1
        elif kind == 3:
            x[m, (7 * m) % 31, (13 * m) % 200] = 1
    return x


def _selected(M):
    """crops whose convolutions are evaluated in float64: all for small batches, else the first, the last and the two
    either side of the first cell-row edge"""
    if M < 17:
        return list(range(M))
    cn = 8 if M <= 8 else 16
    return sorted({0, cn - 1, cn, M - 1})


def _strip(t, level, label):
    """a recorded conv-stack tensor (cell per crop, 52-wide, or dense) -> its crops (M, h, w, C) in natural orientation,
    after asserting that the gutters / padding columns are exactly zero"""
    h, w = LEVELS[level]
    if t.shape[1] == h + 1:  # a cell: zero row 0, zero columns w .. cellW - 1
        assert not t[:, 0].any() and not t[:, :, w:].any(), f"{label}: non-zero cell gutter"
        return t[:, 1:, :w]
    assert t.shape[1] == h, (label, t.shape)
    assert not t[:, :, w:].any(), f"{label}: non-zero padding columns"
    return t[:, :, :w]


def _check_slots(part, label):
    x, slots = part
    if slots is None:
        return float("nan")
    m = np.abs(x).reshape(x.shape[0], -1).max(axis=1)
    assert (slots >= m).all(), f"{label}: max-|x| slot {slots} below the crop's max {m}"
    assert (slots[m == 0] == 0).all(), f"{label}: non-zero slot of an all-zero crop"
    r = slots[m > 0] / m[m > 0]
    ratio = float(r.max()) if r.size else 0.0
    assert ratio <= 2.0, f"{label}: slot / max|x| = {ratio}"
    return ratio


def _producers(taps):
    p = {"conv_2": "conv_1", "conv_3": "conv_2", "pool_3": "conv_3", "conv_5": "conv_4", "pool_5": "conv_5",
         "conv_7": "conv_6", "stn_conv_2": "stn_conv_1", "stn_dense_1": "stn_conv_2", "stn_dense_2": "stn_dense_1",
         "stn_sample.theta": "stn_dense_2", "lstm_10_xproj": "fc_9", "lstm_10": "lstm_10_xproj",
         "lstm_11_xproj": "lstm_10", "lstm_11": "lstm_11_xproj", "fc_12": "lstm_11", "ctc": "fc_12"}
    out = {k: (v, "out") for k, v in p.items()}
    out["conv_4"] = ("pool_3", "out") if "pool_3" in taps else ("conv_3", "pool")
    out["conv_6"] = ("pool_5", "out") if "pool_5" in taps else ("conv_5", "pool")
    keras = "cells_to_keras" if "cells_to_keras" in taps else "crnn_to_keras"
    out[keras] = ("conv_7", "out")
    out["stn_conv_1"] = out["stn_sample"] = (keras, "out")
    out["fc_9"] = ("stn_sample", "out") if "stn_sample" in taps else (keras, "out")
    return out


def _weight_shape(w, name):
    if name.endswith("_xproj"):
        k = w[name[: -len("_xproj")] + "/kernel"]
        cin = k.shape[0] * (2 if name.startswith("lstm_11") else 1)
        return (2 * k.shape[1], cin, 1, 1)
    k = w[name + "/kernel"]
    if k.ndim == 4:
        kh, kw, cin, cout = k.shape
        return (cout, cin, kh, kw)
    return (k.shape[1], k.shape[0], 1, 1)


def check_forward(ctx, w, crops, label, only=None, quiet=False):
    """Runs the forward with every launch tapped; asserts the exact properties (taps change nothing, producers, gutters,
    permutes, poolings, slots, labels) and returns ({name: (max ratio, rms ratio, row, slot ratio)}, taps, probs)."""
    M = crops.shape[0]
    ctx.crnn_set_taps(["*"])
    try:
        lab_t, prob_t = ctx.crnn_forward(crops, return_probs=True)
        taps = ctx.crnn_taps()
    finally:
        ctx.crnn_set_taps([])
    lab, prob = ctx.crnn_forward(crops, return_probs=True)
    assert np.array_equal(prob_t.view(np.uint32), prob.view(np.uint32)) and np.array_equal(lab_t, lab), \
        f"{label}: taps changed the result"
    assert np.array_equal(taps["ctc"]["out"][0].reshape(prob.shape), prob)
    assert np.isfinite(prob).all()
    for name, (src, part) in _producers(taps).items():
        if name in taps and src in taps:
            a, b = taps[name]["in"][0], taps[src][part][0]
            assert np.array_equal(a.reshape(M, -1).view(np.uint32), b.reshape(M, -1).view(np.uint32)), \
                f"{label}: {name}'s input differs from what {src} wrote"
    assert np.array_equal(taps["conv_1"]["in"][0][..., 0], crops)
    sel = _selected(M)
    discard = 50 - lab.shape[1]
    report = {}
    for name, t in taps.items():
        if only is not None and name not in only:
            continue
        row = kernel_row(t["kernel"])
        sr = max([_check_slots(t[p], f"{label} {name}.{p}") for p in ("in", "out", "pool") if t[p] is not None],
                 key=lambda v: -1 if np.isnan(v) else v)
        if name in IN_LEVEL and name != "conv_1":
            x_nat = _strip(t["in"][0], IN_LEVEL[name], f"{label} {name}.in")
        if name in ("cells_to_keras", "crnn_to_keras"):
            assert np.array_equal(t["out"][0], ocrnn.keras_from_natural(x_nat)), f"{label}: {name} is not the permute"
            report[name] = (0.0, 0.0, row, sr)
            continue
        if name in ("pool_3", "pool_5"):
            want = _strip(t["out"][0], POOLED[name], f"{label} {name}.out")
            got = pool2(ocrnn.keras_from_natural(x_nat))
            assert np.array_equal(ocrnn.keras_from_natural(want), got), f"{label}: {name} is not maxpool2x2"
            report[name] = (0.0, 0.0, row, sr)
            continue
        if name == "stn_sample.theta":
            continue
        if name in LEVEL_OF or name.startswith("stn_conv"):
            if name in LEVEL_OF:
                x = taps["conv_1"]["in"][0] if name == "conv_1" else x_nat
                x = ocrnn.keras_from_natural(x[sel])
                out = None if t["out"] is None else ocrnn.keras_from_natural(
                    _strip(t["out"][0], LEVEL_OF[name], f"{label} {name}.out")[sel])
                pool = None if t["pool"] is None else ocrnn.keras_from_natural(
                    _strip(t["pool"][0], POOLED[name], f"{label} {name}.pool")[sel])
            else:
                x, out, pool = t["in"][0][sel], t["out"][0][sel], None
            if row == "crnn_conv1_cells":
                k, window = chk.CONV1_CELLS_K, 0
            else:
                k, window = family(row, _weight_shape(w, name))
            amax = None if t["in"][1] is None else t["in"][1][sel]
            r = chk.check_conv(w, name, x, k, window, out=out, pool=pool, amax=amax)
            if pool is not None and out is not None:
                assert np.array_equal(pool, pool2(out)), f"{label} {name}: pooled != maxpool2x2(full)"
        elif name == "stn_sample":
            th = taps["stn_sample.theta"]["in"][0].reshape(M, 6)
            r = chk.check_stn(t["in"][0][sel], th[sel], t["out"][0][sel])
        elif name in ("lstm_10", "lstm_11"):
            assert row.startswith("lstm_recurrence"), row
            r = chk.check_lstm(w, name, t["in"][0].reshape(M, 50, -1), t["out"][0].reshape(M, 50, -1))
        elif name == "ctc":
            lg = t["in"][0].reshape(M, 50, -1)
            r = chk.check_ctc(lg, t["out"][0], discard)
            assert np.array_equal(lab, ocrnn.greedy_labels(lg[:, discard:], lab.shape[1])), f"{label}: labels"
        else:  # the GEMMs
            k = chk.DENSE_SPLITK_K if row == "dense_splitk" else family(row, _weight_shape(w, name))[0]
            r = chk.check_gemm(w, name, t["in"][0].reshape(M * t["in"][0].shape[1], -1), t["out"][0], k)
        report[name] = (r[0], r[1], row, sr)
    if not quiet:
        print(f"\n{label}: launch, max err / bound, rms err / bound, kernel row, slot / max|x|")
        for name, (r, rms, row, sr) in report.items():
            print(f"  {name:16s} {r:7.3f} {rms:9.2e}  {row:34s} {sr:.3f}")
    bad = {n: v for n, v in report.items() if not (v[0] <= 1.0 and v[1] <= chk.RMS_GATE)}
    assert not bad, f"{label}: launches beyond their stated bound: {bad}"
    return report, taps, prob


def _rows(taps):
    return {n: kernel_row(t["kernel"]) for n, t in taps.items()}


@pytest.fixture
def fresh_ctx(monkeypatch):
    """contexts made with KOCR_* switches set in this process (switches are read when a context is created)"""
    import keras_ocr_amd

    if any(k.startswith("KOCR_") and k != "KOCR_DISPATCH_LOG" for k in os.environ):
        pytest.skip("a KOCR_* switch is set for the whole process")
    made = []

    def make(switches, weights):
        for k, v in switches.items():
            monkeypatch.setenv(k, v)
        try:
            c = keras_ocr_amd.Context(0)
        finally:
            for k in switches:
                monkeypatch.delenv(k)
        made.append(c)
        c.load_crnn(weights)
        return c

    yield make
    for c in made:
        c.close()


_CASES = [  # (configuration, switches, M)
    ("default", {}, 1), ("default", {}, 3), ("default", {}, 17), ("default", {}, 81), ("default", {}, 82),
    ("lstm32", {"KOCR_LSTM16": "0"}, 33), ("no_splitk", {"KOCR_DENSE_SPLITK": "0"}, 3),
    ("dense_batch", {"KOCR_CELLS": "0"}, 3), ("bf16x3", {"KOCR_SPLIT": "bf16"}, 3), ("no_k5", {"KOCR_K5": "0"}, 3),
]


@pytest.mark.parametrize("cfg,switches,M", _CASES, ids=[f"{c[0]}-M{c[2]}" for c in _CASES])
def test_every_launch_within_its_bound(fresh_ctx, crnn_weights, cfg, switches, M):
    """Every launch of the recogniser within the bound of the kernel that ran it, on its own input; the tap's kernel row
    proves the configuration's path ran"""
    c = fresh_ctx(switches, crnn_weights)
    _, taps, _ = check_forward(c, crnn_weights, _crops(M), f"{cfg} M={M}")
    rows = _rows(taps)
    cells = "cells_to_keras" in taps
    if cfg == "default":
        assert cells and rows["conv_1"] == "crnn_conv1_cells", rows
        assert rows["stn_dense_1"] == "dense_splitk" and rows["lstm_10"] == "lstm_recurrence", rows
        assert rows["stn_conv_1"].startswith("conv_k5"), rows
        # the 1x1 kernel switch at 4096 pixels: 81 crops x 50 steps = 4050 on conv_mfma, 82 x 50 = 4100 on conv_ds
        if M in (81, 82):
            for n in ("fc_9", "lstm_10_xproj", "lstm_11_xproj", "fc_12"):
                assert rows[n].startswith("conv_mfma" if M == 81 else "conv_ds"), (n, rows[n])
    elif cfg == "lstm32":
        assert rows["lstm_10"] == rows["lstm_11"] == "lstm_recurrence32", rows
    elif cfg == "no_splitk":
        assert rows["stn_dense_1"].startswith("conv_") and rows["stn_dense_1"] != "dense_splitk", rows
    elif cfg == "dense_batch":
        assert not cells and "pool_3" in taps and "pool_5" in taps and "crnn_to_keras" in taps, rows
        assert taps["conv_6"]["in"][0].shape[2] == 52, "conv_6 / conv_7 not on the 52-wide layout"
    elif cfg == "bf16x3":
        assert rows["conv_6"].startswith("conv_ws") and rows["conv_7"].startswith("conv_ws"), rows
    elif cfg == "no_k5":
        assert rows["stn_conv_1"].startswith("conv_mfma"), rows


def _variant(w, **kw):
    from keras_ocr_amd import weights as kw_

    v = dict(w)
    if kw.get("stn") is False:
        v = {k: a for k, a in v.items() if not k.startswith("stn_")}
    if "classes" in kw:
        full = kw_.synthetic_crnn_weights(4321, n_classes=kw["classes"])
        v["fc_12/kernel"], v["fc_12/bias"] = full["fc_12/kernel"], full["fc_12/bias"]
    if "theta" in kw:
        v["stn_dense_2/kernel"] = np.zeros_like(v["stn_dense_2/kernel"])
        v["stn_dense_2/bias"] = np.asarray(kw["theta"], np.float32)
    return v


@pytest.mark.parametrize("build", ["no_stn", "classes96"])
def test_every_launch_other_builds(fresh_ctx, crnn_weights, build):
    """the build without the localisation network, and 96 classes (two classes per lane in the ctc kernel)"""
    w = _variant(crnn_weights, stn=False) if build == "no_stn" else _variant(crnn_weights, classes=96)
    c = fresh_ctx({}, w)
    _, taps, prob = check_forward(c, w, _crops(3), build)
    if build == "no_stn":
        assert not any(n.startswith("stn_") for n in taps), list(taps)
    else:
        assert prob.shape[-1] == 96


THETAS = {
    "identity": [1, 0, 0, 0, 1, 0],    # last column / row exactly on W / H: the clipped corners, weights summing to zero
    "zoom_out": [1.25, 0, 0, 0, 1.25, 0],
    "shift+0.5": [1, 0, 0.5, 0, 1, 0],  # coordinates beyond W - 1
    "shift-1.5": [1, 0, -1.5, 0, 1, 0],  # negative floors
    "flip": [-1, 0, 0, 0, 1, 0],
    "shear": [1, 0.3, 0, 0.2, 1, 0],
}


@pytest.mark.parametrize("theta", list(THETAS))
def test_stn_sampler_at_edge_thetas(fresh_ctx, crnn_weights, theta):
    """stn_dense_2 = 0 x + theta: the sampler against float64 bilinear interpolation, and its end result against
    oracle.crnn.stn_transform (pinned to the reference's _transform) wherever the corner choice is not ambiguous"""
    import torch

    w = _variant(crnn_weights, theta=THETAS[theta])
    c = fresh_ctx({}, w)
    only = {"stn_dense_2", "stn_sample", "fc_9"}
    report, taps, _ = check_forward(c, w, _crops(3), f"theta {theta}", only=only)
    th = taps["stn_sample.theta"]["in"][0].reshape(-1, 6)
    assert np.array_equal(th, np.tile(np.float32(THETAS[theta]), (3, 1)))
    x, got = taps["stn_sample"]["in"][0], taps["stn_sample"]["out"][0]
    vals, bnd = ocrnn.stn_sample_f64(x, th)
    ambiguous = np.ptp(np.stack(vals), axis=0) > 0
    want = ocrnn.stn_transform(torch.from_numpy(x), torch.from_numpy(th)).numpy()
    err = np.abs(got.astype(np.float64) - want)[~ambiguous]
    assert (err <= 2 * bnd[~ambiguous] + 1e-30).all(), f"{theta}: stn_transform differs by {err.max():.3g}"
