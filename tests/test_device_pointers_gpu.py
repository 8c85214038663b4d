"""Every C-ABI entry point that takes `on_device`, called twice on the same seeded inputs: once with host arrays, once with
torch device tensors.  Both paths run the same kernels on the same data, so the results must be bit-identical.

The entry points are called directly through the ctypes library where no Context method exposes the device path.  Buffers
that include/kocr.h keeps on the host under on_device (counts, boxes / labels of kocr_recognize_boxes and kocr_warp_crops,
the CTC labels and lengths) stay numpy arrays in both calls.
"""
import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu

N_CROPS = 1030  # more than one recogniser batch of 1024 crops


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def _p(a):
    """ctypes argument: a numpy array's address, or a device tensor's data_ptr()"""
    return a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data


class _Abi:
    """Raw calls on one context: every call is made once with host buffers and once with device tensors"""

    def __init__(self, ctx):
        import keras_ocr_amd

        self.lib = keras_ocr_amd.load_library()
        self.ctx = ctx

    def __call__(self, name, *args):
        import torch

        torch.cuda.synchronize()
        rc = getattr(self.lib, name)(self.ctx._h, *[_p(a) if isinstance(a, np.ndarray) or hasattr(a, "data_ptr") else a
                                                   for a in args])
        self.ctx.synchronize()
        return rc


@pytest.fixture(scope="module")
def dctx(craft_weights, crnn_weights):
    import keras_ocr_amd
    from oracle import craft as ocraft
    from oracle import tools as otools

    page = otools.resize_image(synth.text_page(64, 96, 4, seed=3), 2, 2048)[0][None]
    cw = keras_ocr_amd.weights.calibrate_craft_head(craft_weights, ocraft.detector_predict(craft_weights, page),
                                                    text_frac=0.10, link_frac=0.04)
    c = keras_ocr_amd.Context(0)
    c.load_craft(cw)
    c.load_crnn(crnn_weights)
    yield c
    c.close()


@pytest.fixture(scope="module")
def abi(dctx):
    return _Abi(dctx)


@pytest.fixture(scope="module")
def pages():
    """three 128 x 192 detector inputs with words on them"""
    from oracle import tools as otools

    return np.stack([otools.resize_image(synth.text_page(64, 96, 4, seed=s), 2, 2048)[0] for s in (3, 4, 5)])


@pytest.fixture(scope="module")
def crops():
    return np.random.default_rng(7).random((N_CROPS, 31, 200), dtype=np.float32)


@pytest.fixture(scope="module")
def box_groups():
    """rotated rectangles inside a 128 x 192 page, 2 / 0 / 3 per image"""
    rng = np.random.default_rng(11)
    groups = []
    for n in (2, 0, 3):
        g = []
        for _ in range(n):
            cx, cy, w, h, th = rng.uniform(50, 140), rng.uniform(30, 100), rng.uniform(20, 60), rng.uniform(8, 20), \
                rng.uniform(-0.4, 0.4)
            c, s = np.cos(th), np.sin(th)
            corners = [(-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2)]
            g.append([(cx + x * c - y * s, cy + x * s + y * c) for x, y in corners])
        groups.append(np.asarray(g, np.float32).reshape(-1, 4, 2))
    return groups


def _flat(box_groups):
    counts = np.array([len(b) for b in box_groups], np.int32)
    return counts, np.ascontiguousarray(np.concatenate([b for b in box_groups if len(b)]), dtype=np.float32)


def _ctc_inputs(m, t, c, seed):
    rng = np.random.default_rng(seed)
    il = rng.integers(t // 2, t + 1, m).astype(np.int32)
    ll = np.minimum(rng.integers(0, 9, m), il).astype(np.int32)
    labels = rng.integers(0, c - 1, (m, 8)).astype(np.int32)
    return labels, ll, il


def test_craft_forward(abi, pages):
    n, h, w, _ = pages.shape
    for dtype, x in ((0, pages), (1, pages.astype(np.float32) / 255)):
        heat = np.zeros((n, h // 2, w // 2, 2), np.float32)
        assert abi("kocr_craft_forward", x, dtype, n, h, w, heat, 2, 0) == 0
        d_heat = _dev(np.zeros_like(heat))
        assert abi("kocr_craft_forward", _dev(x), dtype, n, h, w, d_heat, 2, 1) == 0
        assert np.array_equal(_host(d_heat), heat)


def test_crnn_forward(abi, dctx, crops):
    lw, c = dctx.crnn_label_width(), dctx.crnn_classes()
    labels, probs = dctx.crnn_forward(crops, return_probs=True)
    d_lab, d_prob = _dev(np.zeros((N_CROPS, lw), np.int32)), _dev(np.zeros((N_CROPS, lw, c), np.float32))
    assert abi("kocr_crnn_forward", _dev(crops), N_CROPS, d_lab, d_prob, 1) == 0
    assert np.array_equal(_host(d_lab), labels)
    assert np.array_equal(_host(d_prob), probs)
    # without probabilities
    d_lab2 = _dev(np.zeros((N_CROPS, lw), np.int32))
    assert abi("kocr_crnn_forward", _dev(crops), N_CROPS, d_lab2, None, 1) == 0
    assert np.array_equal(_host(d_lab2), labels)


def test_crnn_beam(abi, dctx, crops):
    bw, k = 4, 2
    labels, log_prob = dctx.crnn_beam(crops, bw, k)
    assert labels.shape == (N_CROPS, k, dctx.crnn_label_width()) and (labels[:, 0] >= 0).any()
    d_lab, d_logp = _dev(np.full_like(labels, -1)), _dev(np.full_like(log_prob, -np.inf))
    assert abi("kocr_crnn_beam", _dev(crops), N_CROPS, bw, k, d_lab, d_logp, 1) == 0
    assert np.array_equal(_host(d_lab), labels)
    assert np.array_equal(_host(d_logp).view(np.uint32), log_prob.view(np.uint32))


def test_crnn_lexicon(abi, dctx, crops):
    from tests import batch_edge_cases as bc

    k = 3
    words, lengths = bc.lexicon(dctx.crnn_classes())
    try:
        dctx.set_lexicon(words, lengths)
        index, log_prob, values = dctx.crnn_lexicon(crops, k, return_values=True)
        assert values.shape == (N_CROPS, len(words)) and index.min() >= 0
        d_idx, d_logp = _dev(np.full_like(index, -1)), _dev(np.full_like(log_prob, -np.inf))
        d_val = _dev(np.full_like(values, -np.inf))
        assert abi("kocr_crnn_lexicon", _dev(crops), N_CROPS, k, d_idx, d_logp, d_val, 1) == 0
        assert np.array_equal(_host(d_idx), index)
        assert np.array_equal(_host(d_logp).view(np.uint32), log_prob.view(np.uint32))
        assert np.array_equal(_host(d_val).view(np.uint32), values.view(np.uint32))
        # without the values
        d_idx2, d_logp2 = _dev(np.full_like(index, -1)), _dev(np.full_like(log_prob, -np.inf))
        assert abi("kocr_crnn_lexicon", _dev(crops), N_CROPS, k, d_idx2, d_logp2, None, 1) == 0
        assert np.array_equal(_host(d_idx2), index)
        assert np.array_equal(_host(d_logp2).view(np.uint32), log_prob.view(np.uint32))
    finally:
        dctx.set_lexicon(None)


def test_ctc_batch_cost(abi, dctx):
    m, t, c = 9, 20, 11
    y = np.random.default_rng(5).random((m, t, c), dtype=np.float32)
    labels, ll, il = _ctc_inputs(m, t, c, 6)
    loss = np.zeros(m, np.float32)
    assert abi("kocr_ctc_batch_cost", y, m, t, c, labels, labels.shape[1], ll, il, loss, 0) == 0
    d_loss = _dev(np.zeros(m, np.float32))
    assert abi("kocr_ctc_batch_cost", _dev(y), m, t, c, labels, labels.shape[1], ll, il, d_loss, 1) == 0
    assert np.array_equal(_host(d_loss), loss, equal_nan=True)


def test_crnn_ctc_loss(abi, dctx, crops):
    labels, ll, il = _ctc_inputs(N_CROPS, dctx.crnn_label_width(), dctx.crnn_classes(), 8)
    loss = np.zeros(N_CROPS, np.float32)
    assert abi("kocr_crnn_ctc_loss", crops, N_CROPS, labels, labels.shape[1], ll, il, loss, 0) == 0
    d_loss = _dev(np.zeros(N_CROPS, np.float32))
    assert abi("kocr_crnn_ctc_loss", _dev(crops), N_CROPS, labels, labels.shape[1], ll, il, d_loss, 1) == 0
    assert np.array_equal(_host(d_loss), loss, equal_nan=True)


def test_crnn_features(abi, crops):
    feats = np.zeros((N_CROPS, 50, 256), np.float32)
    assert abi("kocr_crnn_features", crops, N_CROPS, feats, 0) == 0
    d_feats = _dev(np.zeros_like(feats))
    assert abi("kocr_crnn_features", _dev(crops), N_CROPS, d_feats, 1) == 0
    assert np.array_equal(_host(d_feats), feats)


def test_get_boxes(abi):
    heat = synth.heatmap_batch()
    n, h, w, _ = heat.shape
    cap = 64
    boxes, counts = np.zeros((n, cap, 4, 2), np.float32), np.zeros(n, np.int32)
    rc = abi("kocr_get_boxes", heat, n, h, w, 0.7, 0.4, 0.4, 10, boxes, counts, cap, 0)
    assert rc in (0, -6) and counts.sum() > 0
    d_boxes, d_counts = _dev(np.zeros_like(boxes)), np.zeros(n, np.int32)
    assert abi("kocr_get_boxes", _dev(heat), n, h, w, 0.7, 0.4, 0.4, 10, d_boxes, d_counts, cap, 1) == rc
    assert np.array_equal(d_counts, counts)
    got = _host(d_boxes)
    for i in range(n):
        assert np.array_equal(got[i, :counts[i]], boxes[i, :counts[i]])


def test_detect(abi, pages):
    n, h, w, _ = pages.shape
    cap = 64
    boxes, counts = np.zeros((n, cap, 4, 2), np.float32), np.zeros(n, np.int32)
    assert abi("kocr_detect", pages, 0, n, h, w, 0.7, 0.4, 0.4, 10, 2, boxes, counts, cap, 0) == 0
    assert counts.sum() > 0
    d_boxes, d_counts = _dev(np.zeros_like(boxes)), np.zeros(n, np.int32)
    assert abi("kocr_detect", _dev(pages), 0, n, h, w, 0.7, 0.4, 0.4, 10, 2, d_boxes, d_counts, cap, 1) == 0
    assert np.array_equal(d_counts, counts)
    got = _host(d_boxes)
    for i in range(n):
        assert np.array_equal(got[i, :counts[i]], boxes[i, :counts[i]])


def test_recognize_boxes(abi, dctx, pages, box_groups):
    n, h, w, _ = pages.shape
    counts, flat = _flat(box_groups)
    m, lw = int(counts.sum()), dctx.crnn_label_width()
    labels = np.full((m, lw), -1, np.int32)
    assert abi("kocr_recognize_boxes", pages, n, h, w, flat, counts, labels, 0) == 0
    labels_dev = np.full((m, lw), -1, np.int32)  # a HOST buffer under on_device too
    assert abi("kocr_recognize_boxes", _dev(pages), n, h, w, flat, counts, labels_dev, 1) == 0
    assert np.array_equal(labels_dev, labels)


def test_warp_crops(abi, pages, box_groups):
    n, h, w, _ = pages.shape
    counts, flat = _flat(box_groups)
    m = int(counts.sum())
    out = np.zeros((m, 31, 200), np.float32)
    assert abi("kocr_warp_crops", pages, n, h, w, flat, counts, 31, 200, out, 0) == 0
    assert out.any()
    d_out = _dev(np.zeros_like(out))
    assert abi("kocr_warp_crops", _dev(pages), n, h, w, flat, counts, 31, 200, d_out, 1) == 0
    assert np.array_equal(_host(d_out), out)


def test_resize_pad(abi):
    src = np.random.default_rng(2).integers(0, 256, (2, 37, 53, 3), dtype=np.uint8)
    dh, dw, hmax, wmax = 74, 106, 80, 112
    out = np.zeros((2, hmax, wmax, 3), np.uint8)
    assert abi("kocr_resize_pad", src, 2, 37, 53, dh, dw, hmax, wmax, 255, out, 0) == 0
    d_out = _dev(np.zeros_like(out))
    assert abi("kocr_resize_pad", _dev(src), 2, 37, 53, dh, dw, hmax, wmax, 255, d_out, 1) == 0
    assert np.array_equal(_host(d_out), out)
