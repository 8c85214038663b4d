"""The recogniser's per-launch checkers (tests/crnn_layer_check.py, used by tests/test_crnn_layers_gpu.py) can fail: each
accepts a float32 torch evaluation of its launch, and rejects a planted defect of just the size that matters -- operands
rounded to bf16 (one piece of a bf16x3 split dropped), h U in bf16 in the recurrence, one missing 64-term chunk of
stn_dense_1's K = 11 200, one crop's output taken from a neighbour that differs by one grey level at one pixel, the
sampler scaled by W - 1 instead of W, BatchNorm eps 1e-5 instead of 1e-3, gates i and f swapped.  (The fp32 MFMA
family's K 2^-24 is loose enough to admit bf16 operands at these K: its own kernel has no split to drop.)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import crnn as ocrnn
from tests import crnn_layer_check as chk

WINOGRAD, SPLIT = 5e-6, 1.5e-6  # tests/layer_bounds.family
KERAS_SHAPES = {"conv_1": (200, 31, 1), "conv_3": (200, 31, 128), "conv_4": (100, 15, 256), "conv_7": (50, 7, 512),
                "stn_conv_1": (50, 7, 512)}
GEMM_IN = {"stn_dense_1": 11200, "stn_dense_2": 64, "fc_9": 3584, "lstm_10_xproj": 128, "lstm_11_xproj": 256, "fc_12": 256}


@pytest.fixture(scope="module")
def w():
    from keras_ocr_amd import weights

    return weights.synthetic_crnn_weights(4321)


def _bf16(a):
    return torch.as_tensor(a).to(torch.bfloat16).to(torch.float32)


def _input(shape, n=2, seed=0):
    x = np.maximum(np.random.default_rng(seed).standard_normal((n, *shape)), 0).astype(np.float32)
    return x


def _conv_f32(w, name, x, round_bf16=False, eps=ocrnn.BN_EPS):
    """a float32 torch evaluation of one convolution launch (Keras orientation), Keras semantics"""
    xt = torch.from_numpy(x).permute(0, 3, 1, 2)
    k = torch.from_numpy(w[name + "/kernel"]).permute(3, 2, 0, 1)
    if round_bf16:
        xt, k = _bf16(xt), _bf16(k)
    y = F.relu(F.conv2d(xt, k, torch.from_numpy(w[name + "/bias"]), padding=k.shape[2] // 2))
    bn = ocrnn.CONV_LAYERS[name][1]
    if bn:
        y = F.batch_norm(y, *(torch.from_numpy(w[f"{bn}/{p}"]) for p in ("moving_mean", "moving_variance", "gamma", "beta")),
                         training=False, eps=eps)
    return y.permute(0, 2, 3, 1).numpy()


def _gemm_f32(w, name, x, round_bf16=False, drop=None):
    k, b, relu = ocrnn._gemm_weights(w, name)
    kt, xt = torch.from_numpy(k.astype(np.float32)), torch.from_numpy(x)
    if round_bf16:
        xt, kt = _bf16(xt), _bf16(kt)
    if drop is not None:
        kt = kt.clone()
        kt[drop] = 0
    y = xt @ kt + torch.from_numpy(b.astype(np.float32))
    return (F.relu(y) if relu else y).numpy()


def _ok(r):
    return r[0] <= 1.0 and r[1] <= chk.RMS_GATE


@pytest.mark.parametrize("name", list(KERAS_SHAPES))
@pytest.mark.parametrize("k,window", [(WINOGRAD, 3), (SPLIT, 0)], ids=["winograd", "split"])
def test_conv_checker_accepts_fp32_and_rejects_bf16_operands(w, name, k, window):
    x = _input(KERAS_SHAPES[name])
    good = chk.check_conv(w, name, x, k, window, out=_conv_f32(w, name, x))
    bad = chk.check_conv(w, name, x, k, window, out=_conv_f32(w, name, x, round_bf16=True))
    print(name, good, bad)
    assert _ok(good) and not _ok(bad)


def test_pooled_conv_checker(w):
    x = _input(KERAS_SHAPES["conv_3"])
    y, yb = _conv_f32(w, "conv_3", x), _conv_f32(w, "conv_3", x, round_bf16=True)
    pool = lambda t: F.max_pool2d(torch.from_numpy(t).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy()
    assert _ok(chk.check_conv(w, "conv_3", x, WINOGRAD, 3, pool=pool(y)))
    assert not _ok(chk.check_conv(w, "conv_3", x, WINOGRAD, 3, pool=pool(yb)))


def test_conv1_cells_bound_accepts_fp32(w):
    x = np.random.default_rng(1).random((2, 200, 31, 1), dtype=np.float32)
    assert _ok(chk.check_conv(w, "conv_1", x, chk.CONV1_CELLS_K, out=_conv_f32(w, "conv_1", x)))


@pytest.mark.parametrize("name", list(GEMM_IN))
def test_gemm_checker_accepts_fp32_and_rejects_bf16_operands(w, name):
    x = _input((GEMM_IN[name],), n=8, seed=2)
    good = chk.check_gemm(w, name, x, _gemm_f32(w, name, x), SPLIT)
    bad = chk.check_gemm(w, name, x, _gemm_f32(w, name, x, round_bf16=True), SPLIT)
    print(name, good, bad)
    assert _ok(good) and not _ok(bad)


def test_dense_splitk_bound_rejects_a_missing_chunk(w):
    """stn_dense_1 at the dense_splitk bound: one 64-term chunk of K = 11 200 left out fails (every chunk position)"""
    x = _input((11200,), n=8, seed=3)
    assert _ok(chk.check_gemm(w, "stn_dense_1", x, _gemm_f32(w, "stn_dense_1", x), chk.DENSE_SPLITK_K))
    for c in (0, 87, 174):
        bad = chk.check_gemm(w, "stn_dense_1", x, _gemm_f32(w, "stn_dense_1", x, drop=slice(64 * c, 64 * c + 64)),
                             chk.DENSE_SPLITK_K)
        assert not _ok(bad), (c, bad)


def test_conv_checker_rejects_a_neighbours_output(w):
    """crop 1 differs from crop 0 by one grey level (1/255) at one pixel: handing crop 1 crop 0's output fails"""
    x = _input(KERAS_SHAPES["conv_4"])
    x[1] = x[0]
    x[1, 40, 7] += np.float32(1 / 255)
    y = _conv_f32(w, "conv_4", x)
    assert _ok(chk.check_conv(w, "conv_4", x, WINOGRAD, 3, out=y))
    y[1] = y[0]
    assert not _ok(chk.check_conv(w, "conv_4", x, WINOGRAD, 3, out=y))


def test_bn_checker_rejects_eps_1e5(w):
    x = _input(KERAS_SHAPES["conv_7"])
    assert _ok(chk.check_conv(w, "conv_7", x, WINOGRAD, 3, out=_conv_f32(w, "conv_7", x)))
    assert not _ok(chk.check_conv(w, "conv_7", x, WINOGRAD, 3, out=_conv_f32(w, "conv_7", x, eps=1e-5)))


def _lstm_f32(w, layer, xp, bf16_hu=False, swap_if=False):
    """the recurrence in float32 torch, both directions, output [fwd | back] in processing order"""
    xp = torch.from_numpy(xp)
    M, T, _ = xp.shape
    out = torch.zeros(M, T, 256)
    for d, suffix in enumerate(("", "_back")):
        U = torch.from_numpy(w[layer + suffix + "/recurrent_kernel"])
        h, c = torch.zeros(M, 128), torch.zeros(M, 128)
        for t in range(T):
            x = xp[:, T - 1 - t if d else t, d * 512:(d + 1) * 512]
            z = x + (_bf16(h) @ _bf16(U) if bf16_hu else h @ U)
            i, f, g, o = z.split(128, dim=1)
            if swap_if:
                i, f = f, i
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            out[:, t, d * 128:(d + 1) * 128] = h
    return out.numpy()


@pytest.mark.parametrize("layer", ["lstm_10", "lstm_11"])
def test_lstm_checker(w, layer):
    x = _input((50, 128 if layer == "lstm_10" else 256), n=4, seed=4).reshape(200, -1)
    xp = _gemm_f32(w, layer + "_xproj", x).reshape(4, 50, 1024)
    good = chk.check_lstm(w, layer, xp, _lstm_f32(w, layer, xp))
    bf16 = chk.check_lstm(w, layer, xp, _lstm_f32(w, layer, xp, bf16_hu=True))
    swap = chk.check_lstm(w, layer, xp, _lstm_f32(w, layer, xp, swap_if=True))
    print(layer, good, bf16, swap)
    assert _ok(good) and not _ok(bf16) and not _ok(swap)


def _sample_f32(x, theta, scale_w=None):
    """stn_sample_kernel's arithmetic in float32 numpy (coordinates scaled by scale_w, W by default)"""
    M, H, W, C = x.shape
    f = np.float32
    xt = np.linspace(-1, 1, W, dtype=np.float32)[None, None, :]
    yt = np.linspace(-1, 1, H, dtype=np.float32)[None, :, None]
    th = [theta[:, i].astype(f).reshape(-1, 1, 1) for i in range(6)]
    fx = f(0.5) * ((th[0] * xt + th[1] * yt) + th[2] + f(1)) * f(scale_w or W)
    fy = f(0.5) * ((th[3] * xt + th[4] * yt) + th[5] + f(1)) * f(H)
    x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
    x1, y1 = np.clip(x0 + 1, 0, W - 1), np.clip(y0 + 1, 0, H - 1)
    x0, y0 = np.clip(x0, 0, W - 1), np.clip(y0, 0, H - 1)
    m = np.arange(M).reshape(-1, 1, 1)
    wa, wb = ((x1 - fx) * (y1 - fy)).astype(f), ((x1 - fx) * (fy - y0)).astype(f)
    wc, wd = ((fx - x0) * (y1 - fy)).astype(f), ((fx - x0) * (fy - y0)).astype(f)
    return ((wa[..., None] * x[m, y0, x0] + wb[..., None] * x[m, y1, x0]) + wc[..., None] * x[m, y0, x1]) + \
        wd[..., None] * x[m, y1, x1]


@pytest.mark.parametrize("theta", [[1, 0, 0, 0, 1, 0], [1.25, 0, 0, 0, 1.25, 0], [1, 0, -1.5, 0, 1, 0],
                                   [-1, 0, 0, 0, 1, 0], [1, 0.3, 0, 0.2, 1, 0], [0.9, 0.01, 0.02, -0.01, 0.9, 0.0]])
def test_stn_checker(theta):
    rng = np.random.default_rng(5)
    x = rng.standard_normal((2, 50, 7, 16)).astype(np.float32)
    th = np.tile(np.float32(theta), (2, 1))
    assert _ok(chk.check_stn(x, th, _sample_f32(x, th)))
    assert _ok(chk.check_stn(x, th, ocrnn.stn_transform(torch.from_numpy(x), torch.from_numpy(th)).numpy()))
    assert not _ok(chk.check_stn(x, th, _sample_f32(x, th, scale_w=6)))


@pytest.mark.parametrize("C", [37, 96])
def test_ctc_checker(C):
    lg = (np.random.default_rng(C).standard_normal((3, 50, C)) * 8).astype(np.float32)
    p = torch.softmax(torch.from_numpy(lg[:, 2:]), -1).numpy()
    assert _ok(chk.check_ctc(lg, p, 2))
    assert not _ok(chk.check_ctc(lg, p * np.float32(1 + 2.0 ** -14), 2))
    assert not _ok(chk.check_ctc(lg, torch.softmax(torch.from_numpy(lg[:, 2:]).to(torch.bfloat16).float(), -1).numpy(), 2))
