"""Oracle: CRAFT detector forward (torch CPU, fp32).  TEST INFRASTRUCTURE ONLY.

Follows the Keras graph of the reference, ``keras_ocr/detection.py``:
  compute_input            :34-42
  make_vgg_block           :87-103   (conv 3x3 same + BN eps=1e-5 + ReLU [+ maxpool 2x2 valid])
  build_vgg_backbone       :312-335  (s1/s2/s3 = ReLU outputs .12/.19/.29, s4 = BN output .38)
  build_keras_model        :353-413  (slice5, concats, upconv, UpsampleLike, conv_cls)
  upconv                   :65-84
  UpsampleLike             :290-303  (resize_bilinear half_pixel_centers == torch
                                      interpolate(align_corners=False), detection.py:605-619)
Weights use the PyTorch state-dict naming that load_torch_weights consumes (:428-468).
"""
import numpy as np
import torch
import torch.nn.functional as F

MEAN = np.array([0.485, 0.456, 0.406])
VARIANCE = np.array([0.229, 0.224, 0.225])


def compute_input(image):
    """detection.py:34-42 — float32 image, in-place subtract / divide by float64 constants."""
    image = np.asarray(image).astype("float32")
    image -= MEAN * 255
    image /= VARIANCE * 255
    return image


def _t(w, name, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(w[name]))
    return t if dtype is None else t.to(dtype)


# Every convolution of the graph: conv name -> (BatchNorm name or None, padding, dilation, ReLU), as build_vgg_backbone /
# build_keras_model / upconv wire them; craft_forward and layer_f64 both evaluate layers through this one table.
LAYERS = {}
for _blk, _ns in (("basenet.slice1", (0, 3, 7, 10)), ("basenet.slice2", (14, 17)), ("basenet.slice3", (20, 24, 27)),
                  ("basenet.slice4", (30, 34, 37))):
    for _n in _ns:  # make_vgg_block: conv 3x3 same + BN + ReLU (:87-103); s4 is the BN output, no ReLU (:333)
        LAYERS[f"{_blk}.{_n}"] = (f"{_blk}.{_n + 1}", 1, 1, _n != 37)
LAYERS["basenet.slice5.1"] = (None, 6, 6, False)  # :365-378, no activation
LAYERS["basenet.slice5.2"] = (None, 0, 1, False)
for _u in (1, 2, 3, 4):  # upconv (:65-84): 1x1 + BN + ReLU, 3x3 same + BN + ReLU
    LAYERS[f"upconv{_u}.conv.0"] = (f"upconv{_u}.conv.1", 0, 1, True)
    LAYERS[f"upconv{_u}.conv.3"] = (f"upconv{_u}.conv.4", 1, 1, True)
for _c, _p, _r in ((0, 1, True), (2, 1, True), (4, 1, True), (6, 0, True), (8, 0, False)):  # head (:392-412), linear output
    LAYERS[f"conv_cls.{_c}"] = (None, _p, 1, _r)


def _conv(w, name, x, padding=0, dilation=1):
    return F.conv2d(x, _t(w, name + ".weight", x.dtype), _t(w, name + ".bias", x.dtype), padding=padding, dilation=dilation)


def _bn(w, name, x, eps=1e-5):
    return F.batch_norm(
        x, _t(w, name + ".running_mean", x.dtype), _t(w, name + ".running_var", x.dtype), _t(w, name + ".weight", x.dtype),
        _t(w, name + ".bias", x.dtype), training=False, eps=eps)


def _layer(w, name, x):
    bn, padding, dilation, relu = LAYERS[name]
    x = _conv(w, name, x, padding=padding, dilation=dilation)
    if bn:
        x = _bn(w, bn, x)
    return F.relu(x) if relu else x


def _vgg_block(w, prefix, n, x, pooling):
    x = _layer(w, f"{prefix}.{n}", x)
    if pooling:
        x = F.max_pool2d(x, 2, 2)
    return x


def _upconv(w, n, x):
    return _layer(w, f"upconv{n}.conv.3", _layer(w, f"upconv{n}.conv.0", x))


def _upsample_like(src, tgt):
    return F.interpolate(src, size=tgt.shape[2:], mode="bilinear", align_corners=False)


def resize_f64(t, size):
    """Bilinear resize (NCHW float64 tensor) with half-pixel centres (UpsampleLike, detection.py:290-303), the sampling
    positions as an fp32 evaluation has them -- scale = in / out rounded to float32, source = (dst + 0.5) scale - 0.5 in
    one fused multiply-add, rounded once to float32 (torch's float upsample_bilinear2d; the library's kernels) -- and the
    blend in float64.  Positions in float64 would differ from every fp32 evaluation by up to 2^-24 x the source
    coordinate wherever in / out is not a power of two."""
    idx = []
    for n_in, n_out in zip(t.shape[2:], size):
        sc = np.float64(np.float32(n_in / n_out))
        src = np.maximum((np.arange(n_out) + 0.5) * sc - 0.5, 0).astype(np.float32)
        i0 = np.floor(src).astype(np.int64)
        i1 = np.minimum(i0 + 1, n_in - 1)
        lam = torch.from_numpy((src - i0.astype(np.float32)).astype(np.float64))
        idx.append((torch.from_numpy(i0), torch.from_numpy(i1), lam))
    (y0, y1, ly), (x0, x1, lx) = idx
    ly, lx = ly.view(1, 1, -1, 1), lx.view(1, 1, 1, -1)
    top = t[:, :, y0][..., x0] * (1 - lx) + t[:, :, y0][..., x1] * lx
    bot = t[:, :, y1][..., x0] * (1 - lx) + t[:, :, y1][..., x1] * lx
    return top * (1 - ly) + bot * ly


def _affine_f64(w, name):
    """(scale, shift) of the BatchNorm-folded epilogue of conv `name` in float64: conv(x) * scale + shift."""
    bn = LAYERS[name][0]
    b = _t(w, name + ".bias", torch.float64)
    if not bn:
        return torch.ones_like(b), b
    sc = _t(w, bn + ".weight", torch.float64) / torch.sqrt(_t(w, bn + ".running_var", torch.float64) + 1e-5)
    return sc, (b - _t(w, bn + ".running_mean", torch.float64)) * sc + _t(w, bn + ".bias", torch.float64)


def _y_channels(w, n):
    """channels of the up-sampled decoder tensor at the head of upconv{n}'s concat: upconv{n-1}'s output (:380-389)"""
    return w[f"upconv{n - 1}.conv.3.weight"].shape[0]


@torch.no_grad()
def layer_f64(w, name, x, up=None, window=0):
    """One launch of the detector forward in float64, on the given input (N,H,W,C) -- the layer semantics of LAYERS,
    i.e. of craft_forward.  Returns (value, bound, unit), all (N,H,W,Cout) float64:
      value  the layer's output,
      bound  (|x| conv |W|) |scale| + |shift| (+ |scale| bilinear(|up|)): the magnitude an fp32-class error is relative to,
      unit   (1 conv |W|) |scale|: the factor of an absolute input error (e.g. 2^-36 max|x| of the fp16x2 split).
    window > 0 replaces |x| in `bound` by its maximum over +-window taps along W at the layer's dilation (the Winograd
    F(4,3) tile: an output shares its input tile with three neighbours, whose products cancel only to THEIR magnitude).
    Besides the LAYERS names, the library's split / composed forms (craft.cpp):
      "upconvN.conv.0#y"       the y columns of the 1x1 over concat(resize(y), skip): no bias, BN or ReLU;
      "upconvN.conv.0#skip"    the skip columns with the layer's epilogue, plus `up` (the #y output) resized to x's size;
      "basenet.slice5#fold"    slice5.1 -> slice5.2 -> upconv1.conv.0's first 1024 columns composed into one dilated 3x3;
      "upconv1.conv.0#skip"    upconv1.conv.0's s4 columns plus `up` (the #fold output), the composed bias, BN and ReLU;
      "head_tail"              conv_cls.6 -> ReLU -> conv_cls.8, bound and unit through the chain."""
    f64 = torch.float64
    xt = torch.from_numpy(np.ascontiguousarray(x)).to(f64).permute(0, 3, 1, 2)
    if name == "head_tail":
        v6, b6, u6 = (t.permute(0, 3, 1, 2) for t in map(torch.from_numpy, layer_f64(w, "conv_cls.6", x)))
        w8 = _t(w, "conv_cls.8.weight", f64)
        val = F.conv2d(v6, w8, _t(w, "conv_cls.8.bias", f64))
        bnd = F.conv2d(b6, w8.abs()) + _t(w, "conv_cls.8.bias", f64).abs().view(1, -1, 1, 1)
        unit = F.conv2d(u6, w8.abs())
        return tuple(t.permute(0, 2, 3, 1).numpy() for t in (val, bnd, unit))
    base, _, part = name.partition("#")
    relu = False
    if base == "basenet.slice5":  # (Wu_a W2) W1: Wu_a = upconv1.conv.0's first 1024 columns
        wu = _t(w, "upconv1.conv.0.weight", f64)[:, :1024, 0, 0]
        w2 = _t(w, "basenet.slice5.2.weight", f64)[:, :, 0, 0]
        wgt = torch.einsum("oc,cd,dikl->oikl", wu, w2, _t(w, "basenet.slice5.1.weight", f64))
        sc = torch.ones(wgt.shape[0], dtype=f64)
        sh = torch.zeros_like(sc)
        padding, dilation = LAYERS["basenet.slice5.1"][1:3]
    else:
        _, padding, dilation, relu = LAYERS[base]
        wgt = _t(w, base + ".weight", f64)
        sc, sh = _affine_f64(w, base)
        if part:
            n = int(base[len("upconv")])
            c_y = 1024 if n == 1 else _y_channels(w, n)
            if part == "y":
                wgt, sc, sh, relu = wgt[:, :c_y], torch.ones_like(sc), torch.zeros_like(sh), False
            else:
                wgt = wgt[:, c_y:]
                if n == 1:  # the composed bias: Wu_a (W2 b1 + b2), inside the BN like the conv bias
                    wu = _t(w, "upconv1.conv.0.weight", f64)[:, :1024, 0, 0]
                    c0 = wu @ (_t(w, "basenet.slice5.2.weight", f64)[:, :, 0, 0] @ _t(w, "basenet.slice5.1.bias", f64) +
                               _t(w, "basenet.slice5.2.bias", f64))
                    sh = sh + c0 * sc
    acc = F.conv2d(xt, wgt, padding=padding, dilation=dilation)
    xa = xt.abs()
    if window:
        xa = F.max_pool2d(F.pad(xa, (window * dilation, window * dilation)), kernel_size=(1, 2 * window + 1), stride=1,
                          dilation=(1, dilation))
    mag = F.conv2d(xa, wgt.abs(), padding=padding, dilation=dilation)
    if part == "skip":
        ut = torch.from_numpy(np.ascontiguousarray(up)).to(f64).permute(0, 3, 1, 2)
        if ut.shape[2:] != acc.shape[2:]:
            acc = acc + resize_f64(ut, acc.shape[2:])
            mag = mag + resize_f64(ut.abs(), acc.shape[2:])
        else:
            acc, mag = acc + ut, mag + ut.abs()
    v = acc * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)
    if relu:
        v = F.relu(v)
    bnd = mag * sc.abs().view(1, -1, 1, 1) + sh.abs().view(1, -1, 1, 1)
    unit = F.conv2d(torch.ones_like(xt[:1]), wgt.abs(), padding=padding, dilation=dilation) * sc.abs().view(1, -1, 1, 1)
    return tuple(t.permute(0, 2, 3, 1).numpy() for t in (v, bnd, unit))


@torch.no_grad()
def craft_forward(w, x_nhwc, return_intermediates=False):
    """x_nhwc: (N,H,W,3) float32, already normalised.  Returns (N,H//2,W//2,2) float32."""
    x = torch.from_numpy(np.ascontiguousarray(x_nhwc, dtype=np.float32)).permute(0, 3, 1, 2)
    inter = {}
    p = "basenet.slice1"
    x = _vgg_block(w, p, 0, x, False)
    inter["basenet.slice1.2"] = x
    x = _vgg_block(w, p, 3, x, True)
    x = _vgg_block(w, p, 7, x, False)
    # slice1.10 block: s1 is the ReLU output (.12); pooling (.13) follows
    s1 = _vgg_block(w, p, 10, x, False)
    x = F.max_pool2d(s1, 2, 2)
    x = _vgg_block(w, "basenet.slice2", 14, x, False)
    x = _vgg_block(w, "basenet.slice2", 17, x, False)
    s2 = x
    x = _vgg_block(w, "basenet.slice3", 20, x, True)
    x = _vgg_block(w, "basenet.slice3", 24, x, False)
    x = _vgg_block(w, "basenet.slice3", 27, x, False)
    s3 = x
    x = _vgg_block(w, "basenet.slice4", 30, x, True)
    x = _vgg_block(w, "basenet.slice4", 34, x, False)
    s4 = _vgg_block(w, "basenet.slice4", 37, x, False)  # BN output, no ReLU (:333)
    # slice5 (:365-378): maxpool 3x3/s1/same (padding ignored), dilated conv, 1x1 conv
    s5 = F.max_pool2d(s4, 3, 1, 1)
    s5 = _layer(w, "basenet.slice5.1", s5)
    s5 = _layer(w, "basenet.slice5.2", s5)
    inter.update(s1=s1, s2=s2, s3=s3, s4=s4, s5=s5)
    y = torch.cat([s5, s4], 1)
    y = _upconv(w, 1, y)
    y = torch.cat([_upsample_like(y, s3), s3], 1)
    y = _upconv(w, 2, y)
    y = torch.cat([_upsample_like(y, s2), s2], 1)
    y = _upconv(w, 3, y)
    y = torch.cat([_upsample_like(y, s1), s1], 1)
    feat = _upconv(w, 4, y)
    inter["features"] = feat
    y = feat
    for c in (0, 2, 4, 6, 8):  # conv_cls.8: linear output for the vgg backbone (:411-412)
        y = _layer(w, f"conv_cls.{c}", y)
    out = y.permute(0, 2, 3, 1).contiguous().numpy()
    if return_intermediates:
        return out, {k: v.permute(0, 2, 3, 1).contiguous().numpy() for k, v in inter.items()}
    return out


def detector_predict(w, images_u8):
    """Detector.detect's device half (detection.py:777-779): compute_input + model.predict."""
    x = np.stack([compute_input(im) for im in images_u8])
    return craft_forward(w, x)
