"""Every launch of the CRAFT forward, in its real schedule, against a float64 evaluation of that launch ON THE GPU'S OWN
INPUT (kocr_craft_set_taps records the input each launch read and what it wrote): errors do not compound, and each layer
is judged by the bound stated for the kernel family that ran it (the tap names the profiler row):

    Winograd F(4,3) / F(2,3)   |err| <= 5e-6   (T|x| conv |w|) s + |b|  + 2^-36 max|x| (1 conv |w|) s    (tests/test_range_gpu.py:
                               T|x| = max of |x| over the +-3 columns of the tile, at the layer's dilation)
    direct split kernels       |err| <= 1.5e-6 ( |x| conv |w|) s + |b|  + the same second term
    fp32 MFMA fallback         |err| <= K 2^-24 (|x| conv |w|) s + |b|  + the same,  K = Cin kh kw
    head tail (fp32 fma)       |err| <= 34 2^-24 (|W8| (|W6| |x| + |b6|) + |b8|)   (two chains of 16 + 1 terms)

s, b: the folded BatchNorm scale and shift (oracle.craft.layer_f64).  Pooled outputs are held to the pooled bound and,
where the full tensor is written too, equal maxpool2x2(full) bit for bit; maxpool3x3s1 and the skip channels of the concat
buffers are exact; resize is within 1e-6 bilinear(|y|).  Every tracked input's per-image max-|x| slot is an upper bound of
that image's max |x| when its consumer is launched, and at most twice it (exactly the source's slot where the producer
copies it; the first layer's slot on uint8 input is a constant bound, within that factor on pages: see _image).  The
checker is shown to be sensitive: the reduced-precision KOCR_SPLIT_F16X1 mode fails it on every F(4,3) layer."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import synth
from tests.layer_bounds import family as _family, kernel_row as _kernel_row, pool2 as _pool2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lctx(ctx, craft_weights):
    ctx.load_craft(craft_weights)
    yield ctx
    ctx.craft_set_taps([])


def _image(case):
    """"page_375x500_u8", or "NxHxW_f32" (normalised input, standard normal) / "1xHxW_u8" (a synthetic page, raw RGB bytes).
    The uint8 inputs are pages -- white with dark, striped words -- because the first layer's output slot is not measured
    but is the layer's constant bound over all uint8 inputs (prepare_conv: ConvLayer::first_bound), and "at most twice
    the image's maximum" is then a property of images that hold black next to white: 1.88 - 1.97 on these pages, but
    2.3 - 2.4 on uniform noise, 2.27 on a blank white page and 27 on a uniformly grey one (float64, from the weights)."""
    if case == "page_375x500_u8":
        return synth.text_page(375, 500, 12, seed=91)[None]
    shape, _, dtype = case.partition("_")
    n, h, w = (int(v) for v in shape.split("x"))
    if dtype == "u8":
        assert n == 1
        return synth.text_page(h, w, 2, seed=h * w, scale=0.2)[None]
    return np.random.default_rng(h * w).standard_normal((n, h, w, 3)).astype(np.float32)


def _weight_shape(w, name):
    base, _, part = name.partition("#")
    if base == "basenet.slice5":
        return (512, 512, 3, 3)
    cout, cin, kh, kw = w[base + ".weight"].shape
    if part:
        n = int(base[len("upconv")])
        c_y = 1024 if n == 1 else w[f"upconv{n - 1}.conv.3.weight"].shape[0]
        cin = c_y if part == "y" else cin - c_y
    return (cout, cin, kh, kw)


# the producer of each launch's input (name, part): the input a launch read must be exactly what its producer wrote
_PRODUCER = {
    "basenet.slice1.3": ("basenet.slice1.0", "out"), "basenet.slice1.7": ("basenet.slice1.3", "pool"),
    "basenet.slice1.10": ("basenet.slice1.7", "out"), "basenet.slice2.14": ("basenet.slice1.10", "pool"),
    "basenet.slice2.17": ("basenet.slice2.14", "out"), "basenet.slice3.20": ("basenet.slice2.17", "out"),
    "basenet.slice3.24": ("basenet.slice3.20", "pool"), "basenet.slice3.27": ("basenet.slice3.24", "out"),
    "basenet.slice4.30": ("basenet.slice3.27", "out"), "basenet.slice4.34": ("basenet.slice4.30", "pool"),
    "basenet.slice4.37": ("basenet.slice4.34", "out"), "maxpool3x3s1": ("basenet.slice4.37", "out"),
    "basenet.slice5#fold": ("maxpool3x3s1", "out"), "basenet.slice5.1": ("maxpool3x3s1", "out"),
    "basenet.slice5.2": ("basenet.slice5.1", "out"), "upconv1.conv.0#skip": ("basenet.slice4.37", "out"),
    "conv_cls.0": ("upconv4.conv.3", "out"), "conv_cls.2": ("conv_cls.0", "out"), "conv_cls.4": ("conv_cls.2", "out"),
    "head_tail": ("conv_cls.4", "out"),
}
_SKIP = {1: "basenet.slice4.37", 2: "basenet.slice3.27", 3: "basenet.slice2.17", 4: "basenet.slice1.10"}
for _n in (2, 3, 4):
    _PRODUCER[f"upconv{_n}.conv.0#y"] = (f"upconv{_n - 1}.conv.3", "out")
    _PRODUCER[f"resize:upconv{_n}"] = (f"upconv{_n - 1}.conv.3", "out")
    _PRODUCER[f"upconv{_n}.conv.0#skip"] = (_SKIP[_n], "out")


def _producers(taps):
    """_PRODUCER plus upconvN.conv.3, whose input comes from upconvN.conv.0 or its #skip form, whichever ran (the unfolded
    upconvN.conv.0 reads a concat buffer: checked part by part)"""
    prod = dict(_PRODUCER)
    for n in (1, 2, 3, 4):
        prod[f"upconv{n}.conv.3"] = (f"upconv{n}.conv.0#skip" if f"upconv{n}.conv.0#skip" in taps else f"upconv{n}.conv.0", "out")
    return prod


def _check_forward(ctx, w, img, label, quiet=False):
    """Runs the forward with every launch tapped; returns {name: (max err / bound, rms err / bound term, row, slot ratio)}
    after asserting the exact properties (bit identities, slots); the caller asserts the ratios."""
    from oracle import craft as ocraft

    ctx.craft_set_taps(["*"])
    heat_tapped = ctx.craft_forward(img)
    taps = ctx.craft_taps()
    ctx.craft_set_taps([])
    heat = ctx.craft_forward(img)
    assert np.array_equal(heat_tapped.view(np.uint32), heat.view(np.uint32)), f"{label}: taps changed the heat-map"
    assert np.array_equal(taps["head_tail"]["out"][0], heat)
    producers = _producers(taps)

    report = {}
    for name, t in taps.items():
        row = _kernel_row(t["kernel"])
        x, slots = t["in"] if t["in"] is not None else (None, None)
        # the input is what its producer wrote, untouched since
        pr = producers.get(name)
        if pr is not None and x is not None:
            assert np.array_equal(x.view(np.uint32), taps[pr[0]][pr[1]][0].view(np.uint32)), f"{label} {name}: input != {pr}"
        if name == "basenet.slice1.0":
            if x is None:  # uint8 image: conv_first / conv_mfma MODE 2 on the normalisation table
                x = np.stack([ocraft.compute_input(im) for im in img])
            else:
                assert np.array_equal(x, img)
        slot_ratio = float("nan")
        if slots is not None:
            m = np.abs(x).reshape(x.shape[0], -1).max(axis=1)
            assert (slots >= m).all(), f"{label} {name}: max-|x| slot {slots} below the input's max {m}"
            slot_ratio = float((slots / np.maximum(m, 1e-30)).max())
            if name in ("basenet.slice5#fold", "basenet.slice5.1"):  # h0's slots: a copy of s4's (|maxpool(s4)| <= max|s4|)
                src = taps["maxpool3x3s1"]["in"][1]
                assert src is not None and (slots <= src).all(), f"{label} {name}: slot {slots} above its source {src}"
            else:
                assert slot_ratio <= 2.0, f"{label} {name}: slot / max|x| = {slot_ratio}"
        if name == "maxpool3x3s1":
            assert x.min() < 0, "s4 (a BN output without ReLU) should hold negative values"
            want = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1).numpy()
            assert np.array_equal(t["out"][0], want), f"{label}: maxpool3x3s1 differs from the 3x3 max of s4"
            report[name] = (0.0, 0.0, row, slot_ratio)
            continue
        if name.startswith("resize:"):
            n = int(name[len("resize:upconv"):])
            cat = t["out"][0]
            c_y = x.shape[3]
            xt = torch.from_numpy(x).double().permute(0, 3, 1, 2)
            size = cat.shape[1:3]
            want = ocraft.resize_f64(xt, size).permute(0, 2, 3, 1).numpy()
            mag = ocraft.resize_f64(xt.abs(), size).permute(0, 2, 3, 1).numpy()
            r = np.abs(cat[..., :c_y] - want) / np.maximum(1e-6 * mag, 1e-300)
            assert np.array_equal(cat[..., c_y:], taps[_SKIP[n]]["out"][0]), f"{label}: skip channels of {name} overwritten"
            consumer = taps[f"upconv{n}.conv.0"]["in"][0]
            assert np.array_equal(consumer.view(np.uint32), cat.view(np.uint32)), f"{label}: concat changed before upconv{n}.conv.0"
            report[name] = (float(r.max()), float(np.sqrt((r ** 2).mean())) * 1e-6, row, slot_ratio)
            continue
        if name == "upconv1.conv.0":  # unfolded: cat1 = [s5 | s4]
            assert np.array_equal(x[..., :1024], taps["basenet.slice5.2"]["out"][0]), f"{label}: s5 in cat1 overwritten"
            assert np.array_equal(x[..., 1024:], taps["basenet.slice4.37"]["out"][0]), f"{label}: s4 in cat1 overwritten"
        up = None
        if name.endswith("#skip"):
            n = int(name[len("upconv")])
            up = taps["basenet.slice5#fold" if n == 1 else f"upconv{n}.conv.0#y"]["out"][0]
        if name == "head_tail":
            assert row == "conv_head_tail", row
            k, window = 34 * 2.0 ** -24, 0
        else:
            k, window = _family(row, _weight_shape(w, name))
        val, bnd, unit = ocraft.layer_f64(w, name, x, up=up, window=window)
        amax = np.abs(x).reshape(x.shape[0], -1).max(axis=1).astype(np.float64).reshape(-1, 1, 1, 1)
        allowed = k * bnd + 2.0 ** -36 * amax * unit
        ratios = []
        if t["out"] is not None:
            got = t["out"][0]
            err = np.abs(got.astype(np.float64) - val)
            ratios.append(float((err / np.maximum(allowed, 1e-300)).max()))
            rms = float(np.sqrt(((err / np.maximum(bnd, 1e-300)) ** 2).mean()))
        if t["pool"] is not None:
            pooled = t["pool"][0]
            err = np.abs(pooled.astype(np.float64) - _pool2(val))
            ratios.append(float((err / np.maximum(_pool2(allowed), 1e-300)).max()))
            if t["out"] is None:
                rms = float(np.sqrt(((err / np.maximum(_pool2(bnd), 1e-300)) ** 2).mean()))
            else:
                assert np.array_equal(pooled, _pool2(t["out"][0])), f"{label} {name}: pooled != maxpool2x2(full)"
        report[name] = (max(ratios), rms, row, slot_ratio)
    if not quiet:
        print(f"\n{label}: layer, max err / stated bound, rms err / bound term, kernel row, input slot / max|x|")
        for name, (r, rms, row, sr) in report.items():
            print(f"  {name:24s} {r:7.3f} {rms:9.2e}  {row:34s} {sr:.3f}")
    return report, taps, heat


_CASES = [("default", "1x64x512_f32"), ("default", "1x50x70_f32"), ("default", "page_375x500_u8"),
          ("bf16x3", "1x64x512_f32"), ("bf16x3", "1x50x70_f32"), ("bf16x3", "page_375x500_u8"),
          ("bf16x3_unfolded", "page_375x500_u8"),
          # the smallest and the most lopsided pages.  16 x 16 is the smallest legal one (levels 8, 4, 2, 1: the deepest
          # layers run on ONE pixel); 17 x 19 has every level odd or 1 x 1 (floor pooling everywhere); three 18 x 22 images
          # put all three into one flattened tile at the deep levels; 16 x 272 is a strip (widths 272, 136, 68, 34, 17)
          ("default", "1x16x16_u8"), ("default", "1x16x16_f32"), ("default", "1x17x19_u8"), ("default", "3x18x22_f32"),
          ("default", "1x16x272_f32"), ("default", "1x33x16_f32"),
          ("bf16x3", "1x17x19_u8"), ("bf16x3", "3x18x22_f32"), ("bf16x3_unfolded", "1x17x19_u8")]


@pytest.mark.parametrize("mode,case", _CASES, ids=[f"{m}-{c}" for m, c in _CASES])
def test_every_layer_within_its_fp32_class_bound(lctx, craft_weights, mode, case):
    """Every launch of the detector within the bound of the kernel that ran it, on its own input (module docstring).
    "default": the context's arithmetic (fp16x2 unless the environment says otherwise); "bf16x3": the exact split;
    "_unfolded": also the layer-by-layer slice5 chain and resize + concat decoder (kocr_set_schedule(0, 0))."""
    from oracle import craft as ocraft
    from tests.test_craft_gpu import HEAT_TOL

    img = _image(case)
    prev, sched = lctx.get_split_mode(), lctx.get_schedule()  # a context made under KOCR_LINFOLD / KOCR_UPFOLD keeps them
    try:
        if mode.startswith("bf16x3"):
            lctx.set_split_mode("bf16x3")
        if mode.endswith("unfolded"):
            lctx.set_schedule(False, False)
        report, taps, heat = _check_forward(lctx, craft_weights, img, f"{mode} {case}")
    finally:
        lctx.set_split_mode(prev)
        lctx.set_schedule(*sched)
    # ... and the heat-map they add up to within the forward's own tolerance of the oracle
    want = ocraft.detector_predict(craft_weights, img) if img.dtype == np.uint8 else ocraft.craft_forward(craft_weights, img)
    assert heat.shape == want.shape == (img.shape[0], img.shape[1] // 2, img.shape[2] // 2, 2)
    heat_err = float(np.abs(heat - want).max())
    print(f"heat-map error against the oracle: {heat_err:.2e}")
    assert heat_err <= HEAT_TOL, f"max abs heat-map error {heat_err}"
    worst = max(report.items(), key=lambda kv: kv[1][0])
    print(f"largest: {worst[0]} {worst[1][0]:.3f} ({worst[1][2]})")
    assert sum(1 for n in taps if n.startswith(("basenet", "upconv", "conv_cls"))) >= 25
    if mode.endswith("unfolded"):
        assert "resize:upconv2" in taps and "basenet.slice5.2" in taps
    bad = {n: r for n, r in report.items() if not r[0] <= 1.0}
    assert not bad, f"layers beyond their stated bound: {bad}"


def test_fp32_class_checker_rejects_the_f16x1_mode(lctx, craft_weights):
    """Negative control: in KOCR_SPLIT_F16X1 (one fp16 piece, 2^-12 relative: the opt-in fast mode) the per-layer check
    must fail on every F(4,3) layer that runs one piece -- the checker sees an fp32-class bound being missed."""
    prev = lctx.get_split_mode()
    lctx.set_split_mode("f16x1")
    try:
        report, _, _ = _check_forward(lctx, craft_weights, _image("1x64x512_f32"), "f16x1 1x64x512_f32")
    finally:
        lctx.set_split_mode(prev)
    one_piece = {n: r[0] for n, r in report.items() if r[2].startswith("conv_w4q")}
    print(f"one-piece F(4,3) layers, max err / stated bound: {one_piece}")
    assert len(one_piece) >= 3, report
    assert all(r > 1.0 for r in one_piece.values()), one_piece


@pytest.mark.parametrize("h,w", [(15, 16), (16, 15)])
def test_page_below_16x16_is_refused_and_harmless(lctx, h, w):
    """A page with a side under 16 pixels has no 1/16 level: KOCR_EINVAL with its reason, and the next forward on the same
    context gives what it gave before."""
    import keras_ocr_amd

    page = _image("1x16x16_u8")
    before = lctx.craft_forward(page)
    for dtype in (np.uint8, np.float32):
        with pytest.raises(keras_ocr_amd.KocrError, match=r"libkocr error -1: .*smaller than 16x16"):  # -1: KOCR_EINVAL
            lctx.craft_forward(np.zeros((1, h, w, 3), dtype))
    after = lctx.craft_forward(page)
    assert before.shape == (1, 8, 8, 2) and np.isfinite(before).all()
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))


def _part0(taps):
    parts = {(n, p): (v[0][:1], None if v[1] is None else v[1][:1]) for n, t in taps.items() for p in ("in", "out", "pool")
             if (v := t[p]) is not None}
    return {n: t["kernel"] for n, t in taps.items()}, parts


def _same(a, b):
    """equal taps (launch order: the first difference names the launch that broke independence), run by the same kernels"""
    (ka, a), (kb, b) = a, b
    assert ka == kb, {n: (ka[n], kb.get(n)) for n in ka if ka[n] != kb.get(n)}
    assert a.keys() == b.keys()
    for k in a:
        d = np.abs(a[k][0].astype(np.float64) - b[k][0]).max()
        assert np.array_equal(a[k][0].view(np.uint32), b[k][0].view(np.uint32)), f"{k} differs by up to {d:.3g}"
        assert (a[k][1] is None) == (b[k][1] is None) and (a[k][1] is None or np.array_equal(a[k][1], b[k][1])), k


def _alone_after_hot_and_batched(lctx):
    x0 = _image("1x64x512_f32")
    hot = np.float32(4096) * np.random.default_rng(5).standard_normal(x0.shape).astype(np.float32)
    lctx.craft_set_taps(["*"])
    try:
        h0 = lctx.craft_forward(x0)
        t0 = _part0(lctx.craft_taps())
        lctx.craft_forward(hot)
        h1 = lctx.craft_forward(x0)
        t1 = _part0(lctx.craft_taps())
        hb = lctx.craft_forward(np.concatenate([x0, hot]))
        tb = _part0(lctx.craft_taps())
    finally:
        lctx.craft_set_taps([])
    return (h0, t0), (h1, t1), (hb[:1], tb)


def test_fp32_class_no_stale_slot_after_a_hot_image(lctx):
    """Image 0's taps, slots and heat-map are bit-identical whether it runs first or right after a forward of a 4096x
    louder image on the same context (the max-|x| slots start from zero every call)."""
    (h0, t0), (h1, t1), _ = _alone_after_hot_and_batched(lctx)
    _same(t0, t1)
    assert np.array_equal(h0, h1)


def test_fp32_class_images_are_independent_in_a_batch(lctx):
    """Image 0's taps, slots and heat-map are bit-identical alone and batched with a 4096x louder image: no slot, tile or
    kernel choice is shared between images (at 1x64x512 upconv4.conv.0#y reads 2048 pixels per image -- under the 4096
    of launch_conv's small-GEMM cut-off alone, over it with a second image; craft.cpp keeps the 1x1 layers on conv_ds)."""
    (h0, t0), _, (hb, tb) = _alone_after_hot_and_batched(lctx)
    _same(t0, tb)
    assert np.array_equal(h0, hb)
