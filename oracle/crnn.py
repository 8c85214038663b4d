"""Oracle: CRNN recogniser forward + CTC greedy decode (torch CPU, fp32).
TEST INFRASTRUCTURE ONLY.

Follows ``keras_ocr/recognition.py`` with Keras/TensorFlow layer semantics (SURVEY.md
Appendix C).  TensorFlow cannot be installed here; status: the STN sampler is **pinned** to the reference's own
``_transform`` (executed through a numpy stand-in of the TF ops it uses, tests/golden/make_golden.py); the LSTM, the
conv / BatchNorm / pooling stack and the CTC rule are **cross-checked by independent implementations** (torch.nn.LSTM /
Conv2d / BatchNorm2d modules with Keras-ordered weights, itertools.groupby: tests/test_thirdparty_crosscheck_cpu.py).
Every step cites the line it restates:

  Permute((2,1,3)) + flip axis 2                         :215-216
  conv_1..conv_7 3x3 same ReLU; BN *after* ReLU (Keras default eps=1e-3) at 3/5/7;
  MaxPooling2D(2) valid after bn_3, bn_5                 :217-242
  STN localisation net (5x5 conv16, 5x5 conv32, Flatten, Dense64 ReLU, Dense6) :268-278
  _transform bilinear sampler (scale by W/H, clipped corners) :73-166
  Reshape (W/4, H/4*512)                                 :282-288
  fc_9 Dense ReLU                                        :290
  lstm_10 / lstm_10_back (go_backwards, NOT re-reversed) -> Add :292-305
  lstm_11 / lstm_11_back -> Concatenate                  :306-319
  fc_12 Dense softmax; drop first rnn_steps_to_discard=2 :321-328
  CTCDecoder: keras.backend.ctc_decode greedy, -1 padding :169-184
  string assembly                                        :527-536

Keras LSTM (tf.keras >= 2.0 defaults): z = x@W + h@U + b, gate order [i, f, c~, o],
recurrent_activation = sigmoid, activation = tanh, zero initial state.
"""
import string

import numpy as np
import torch
import torch.nn.functional as F

DEFAULT_ALPHABET = string.digits + string.ascii_lowercase  # recognition.py:25
BN_EPS = 1e-3


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def _conv(w, name, x, relu=True):
    k = _t(w[name + "/kernel"]).permute(3, 2, 0, 1)  # HWIO -> OIHW
    pad = (k.shape[2] // 2, k.shape[3] // 2)
    y = F.conv2d(x, k, _t(w[name + "/bias"]), padding=pad)
    return F.relu(y) if relu else y


def _bn(w, name, x):
    return F.batch_norm(x, _t(w[name + "/moving_mean"]), _t(w[name + "/moving_variance"]), _t(w[name + "/gamma"]),
                        _t(w[name + "/beta"]), training=False, eps=BN_EPS)


def stn_transform(x_nhwc, theta):
    """recognition._transform (:73-166).  x_nhwc: (M,H,W,C) torch; theta: (M,6)."""
    M, H, W, C = x_nhwc.shape
    theta = theta.reshape(M, 2, 3)
    xs = torch.linspace(-1.0, 1.0, W)
    ys = torch.linspace(-1.0, 1.0, H)
    yy, xx = torch.meshgrid(ys, xs, indexing="ij")  # tf.meshgrid(x, y): rows = y
    xt = xx.reshape(-1)
    yt = yy.reshape(-1)
    x_s = (theta[:, 0, 0:1] * xt[None] + theta[:, 0, 1:2] * yt[None]) + theta[:, 0, 2:3]
    y_s = (theta[:, 1, 0:1] * xt[None] + theta[:, 1, 1:2] * yt[None]) + theta[:, 1, 2:3]
    x = 0.5 * (x_s + 1.0) * float(W)
    y = 0.5 * (y_s + 1.0) * float(H)
    x0 = torch.floor(x).to(torch.int64)
    x1 = x0 + 1
    y0 = torch.floor(y).to(torch.int64)
    y1 = y0 + 1
    x0 = x0.clamp(0, W - 1)
    x1 = x1.clamp(0, W - 1)
    y0 = y0.clamp(0, H - 1)
    y1 = y1.clamp(0, H - 1)
    flat = x_nhwc.reshape(M, H * W, C)

    def gather(yi, xi):
        idx = (yi * W + xi)[..., None].expand(-1, -1, C)
        return torch.gather(flat, 1, idx)

    pa, pb, pc, pd = gather(y0, x0), gather(y1, x0), gather(y0, x1), gather(y1, x1)
    x0f, x1f, y0f, y1f = x0.float(), x1.float(), y0.float(), y1.float()
    a = ((x1f - x) * (y1f - y))[..., None]
    b = ((x1f - x) * (y - y0f))[..., None]
    c = ((x - x0f) * (y1f - y))[..., None]
    d = ((x - x0f) * (y - y0f))[..., None]
    out = ((a * pa + b * pb) + c * pc) + d * pd
    return out.reshape(M, H, W, C)


def _lstm(w, name, x, go_backwards):
    """Keras LSTM, return_sequences=True.  x: (M,T,in).  Outputs in processing order."""
    W, U, b = _t(w[name + "/kernel"]), _t(w[name + "/recurrent_kernel"]), _t(w[name + "/bias"])
    M, T, _ = x.shape
    units = U.shape[0]
    h = torch.zeros(M, units)
    c = torch.zeros(M, units)
    outs = []
    steps = range(T - 1, -1, -1) if go_backwards else range(T)
    for t in steps:
        z = x[:, t] @ W + h @ U + b
        i, f, g, o = z.split(units, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        outs.append(h)
    return torch.stack(outs, 1)


@torch.no_grad()
def crnn_forward(w, X, rnn_steps_to_discard=2, return_intermediates=False):
    """X: (M,31,200,1) float32 in [0,1].  Returns softmax probabilities (M,48,C+1)."""
    X = _t(X)
    if X.ndim == 3:
        X = X[..., None]
    inter = {}
    x = X.permute(0, 2, 1, 3)           # Permute((2,1,3)) -> (M,200,31,1)
    x = torch.flip(x, dims=[2])         # x[:, :, ::-1]
    x = x.permute(0, 3, 1, 2)           # NCHW with H=200, W=31
    x = _conv(w, "conv_1", x)
    x = _conv(w, "conv_2", x)
    x = _bn(w, "bn_3", _conv(w, "conv_3", x))
    x = F.max_pool2d(x, 2)
    x = _conv(w, "conv_4", x)
    x = _bn(w, "bn_5", _conv(w, "conv_5", x))
    x = F.max_pool2d(x, 2)
    x = _conv(w, "conv_6", x)
    x = _bn(w, "bn_7", _conv(w, "conv_7", x))
    inter["bn_7"] = x.permute(0, 2, 3, 1)
    # STN (recognition.py:243-281: only `if stn:`; a weight set without stn_* tensors = build_params["stn"] False)
    if "stn_conv_1/kernel" in w:
        loc = _conv(w, "stn_conv_1", x)
        loc = _conv(w, "stn_conv_2", loc)
        loc = loc.permute(0, 2, 3, 1).reshape(loc.shape[0], -1)  # Keras Flatten of NHWC
        loc = F.relu(loc @ _t(w["stn_dense_1/kernel"]) + _t(w["stn_dense_1/bias"]))
        theta = loc @ _t(w["stn_dense_2/kernel"]) + _t(w["stn_dense_2/bias"])
        inter["theta"] = theta
        x = stn_transform(x.permute(0, 2, 3, 1).contiguous(), theta)  # (M,50,7,512)
    else:
        x = x.permute(0, 2, 3, 1).contiguous()
    inter["stn"] = x
    M = x.shape[0]
    x = x.reshape(M, x.shape[1], -1)    # Reshape((W//4, (H//4)*512))
    x = F.relu(x @ _t(w["fc_9/kernel"]) + _t(w["fc_9/bias"]))
    inter["fc_9"] = x
    f1 = _lstm(w, "lstm_10", x, False)
    b1 = _lstm(w, "lstm_10_back", x, True)
    x = f1 + b1
    inter["rnn_1_add"] = x
    f2 = _lstm(w, "lstm_11", x, False)
    b2 = _lstm(w, "lstm_11_back", x, True)
    x = torch.cat([f2, b2], -1)
    inter["rnn_2"] = x
    logits = x @ _t(w["fc_12/kernel"]) + _t(w["fc_12/bias"])
    p = torch.softmax(logits, -1)[:, rnn_steps_to_discard:]
    inter["logits"] = logits[:, rnn_steps_to_discard:]
    if return_intermediates:
        return p.numpy(), {k: v.numpy() for k, v in inter.items()}
    return p.numpy()


def ctc_greedy_decode(probs):
    """keras.backend.ctc_decode(greedy=True) + the -1 re-padding of CTCDecoder (:169-184):
    per-step argmax (lowest index on ties), merge repeats, drop blank = last class."""
    probs = np.asarray(probs)
    M, T, C = probs.shape
    blank = C - 1
    out = np.full((M, T), -1, dtype=np.int64)
    best = np.log(probs + 1e-7).argmax(-1)
    for m in range(M):
        prev = -1
        k = 0
        for t in range(T):
            c = int(best[m, t])
            if c != prev and c != blank:
                out[m, k] = c
                k += 1
            prev = c
    return out


def decode_strings(labels, alphabet=DEFAULT_ALPHABET):
    """recognition.py:527-534."""
    blank = len(alphabet)
    return ["".join(alphabet[i] for i in row if i not in (blank, -1)) for row in labels]


def recognize_crops(w, X, alphabet=DEFAULT_ALPHABET):
    probs = crnn_forward(w, X)
    return decode_strings(ctc_greedy_decode(probs), alphabet), probs


# ---- per-launch float64 statements (tests/test_crnn_layers_gpu.py) -------------------------------------------------------
# Each launch of the library's recogniser forward restated in float64 from the KERAS weight dict (not from the library's
# prepared weights, so that a wrong fold in crnn_load fails), on the input the launch read.  Tensors are in Keras orientation:
# the conv stack (M, 200, 31, C) / (M, 100, 15, C) / (M, 50, 7, C), the GEMMs (rows, K).
U32 = 2.0 ** -24  # unit round-off of float32


def gamma(n):
    """gamma_n = n u / (1 - n u): the relative bound of an n-term float32 sum of products"""
    return n * U32 / (1 - n * U32)


def keras_from_natural(t):
    """(M, h, w, C) in the crop's natural orientation -> Keras orientation (M, w, h, C): x'[w][j] = x[h - 1 - j][w]
    (recognition.py:215-216; for the pooled levels, natural rows 2i + 1, 2i + 2 pool into Keras column h' - 1 - i)"""
    return np.ascontiguousarray(np.asarray(t).transpose(0, 2, 1, 3)[:, :, ::-1, :])


def bn_fold_f32(w, name, eps=BN_EPS):
    """BatchNorm after the ReLU as v * a + b, folded in float32 like the reference's inference arithmetic"""
    g, be = np.float32(w[name + "/gamma"]), np.float32(w[name + "/beta"])
    mu, var = np.float32(w[name + "/moving_mean"]), np.float32(w[name + "/moving_variance"])
    a = g / np.sqrt(var + np.float32(eps))
    return a.astype(np.float64), (be - mu * a).astype(np.float64)


def _gemm_weights(w, name):
    """(kernel [K][N], bias [N], relu) of a Dense-type launch, float64; the merged LSTM input projections are restated
    here: [W_fwd | W_back], [b_fwd | b_back], and for lstm_11 the Add folded in as [W; W] over the [fwd | back] halves"""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    if name.endswith("_xproj"):
        lay = name[: -len("_xproj")]
        k = np.concatenate([f64(w[lay + "/kernel"]), f64(w[lay + "_back/kernel"])], axis=1)
        b = np.concatenate([f64(w[lay + "/bias"]), f64(w[lay + "_back/bias"])])
        if lay == "lstm_11":
            k = np.concatenate([k, k], axis=0)
        return k, b, False
    return f64(w[name + "/kernel"]), f64(w[name + "/bias"]), name in ("stn_dense_1", "fc_9")


CONV_LAYERS = {f"conv_{i}": (3, f"bn_{i}" if i in (3, 5, 7) else None) for i in range(1, 8)}
CONV_LAYERS.update({"stn_conv_1": (5, None), "stn_conv_2": (5, None)})


@torch.no_grad()
def layer_f64(w, name, x, window=0, bn_eps=BN_EPS):
    """One launch in float64 on its input x.  Returns (value, bound, unit), float64, shaped as the output:
      value  the launch's output (conv / Dense + bias, ReLU, the BatchNorm that follows the ReLU at conv_3/5/7),
      bound  ((|x| conv |K|) + |bias|) |a| + |b|: the magnitude an fp32-class error is relative to (a, b: the BN fold),
      unit   (1 conv |K|) |a|: the factor of an absolute input error (2^-36 max|x| of the fp16x2 split).
    Convolutions: x (M, H, W, C) in Keras orientation; window > 0 replaces |x| in `bound` by its maximum over +-window
    rows along H -- the crop's natural W, the axis the Winograd tiles run along.  GEMMs: x (rows, K)."""
    if name in CONV_LAYERS:
        k, bn = CONV_LAYERS[name]
        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
        kern = torch.from_numpy(np.asarray(w[name + "/kernel"], dtype=np.float64)).permute(3, 2, 0, 1)
        bias = torch.from_numpy(np.asarray(w[name + "/bias"], dtype=np.float64)).view(1, -1, 1, 1)
        a, b = bn_fold_f32(w, bn, bn_eps) if bn else (np.ones(kern.shape[0]), np.zeros(kern.shape[0]))
        a, b = torch.from_numpy(a).view(1, -1, 1, 1), torch.from_numpy(b).view(1, -1, 1, 1)
        p = k // 2
        val = F.relu(F.conv2d(xt, kern, padding=p) + bias) * a + b
        xa = xt.abs()
        if window:
            xa = F.max_pool2d(F.pad(xa, (0, 0, window, window)), kernel_size=(2 * window + 1, 1), stride=1)
        bnd = (F.conv2d(xa, kern.abs(), padding=p) + bias.abs()) * a.abs() + b.abs()
        unit = F.conv2d(torch.ones_like(xt[:1]), kern.abs(), padding=p) * a.abs()
        return tuple(t.permute(0, 2, 3, 1).numpy() for t in (val, bnd, unit))
    kern, bias, relu = _gemm_weights(w, name)
    x = np.asarray(x, dtype=np.float64).reshape(-1, kern.shape[0])
    val = x @ kern + bias
    if relu:
        val = np.maximum(val, 0)
    bnd = np.abs(x) @ np.abs(kern) + np.abs(bias)
    unit = np.broadcast_to(np.abs(kern).sum(axis=0), val.shape)
    return val, bnd, unit


def _sig(z):
    return 0.5 * (1 + np.tanh(0.5 * z))


# stated allowance of the device's gate functions: sigmoid = 1 / (1 + expf(-z)) and tanhf, each within 8 ulp of its value
GATE_ULPS = 8


def lstm_teacher_forced(w, layer, xp, out):
    """The recurrence of lstm_10 / lstm_11 (both directions), TEACHER-FORCED: step t computes z = xp(t) + h_gpu(t-1) U in
    float64 from the GPU's own previous h, carries c in float64, and propagates a running bound of |h_gpu - h64|:
      dz <= gamma_129 (|xp| + |h| |U|);  gates through their derivatives (sup over z +- dz) + GATE_ULPS ulp;
      dc(t) <= (|f| + df) dc(t-1) + df |c| + di |g| + (|i| + di) dg + 3 u (|f c| + |i g|)   (|f| < 1: contractive);
      dh <= do |tanh c| + (|o| + do)(tanh'(c) dc + GATE_ULPS u |tanh c|) + u |h|.
    xp (M, T, 1024) as the launch read it, out (M, T, 256) = [fwd | back] in processing order.  Returns (h64, bound),
    both (M, T, 256) in the same layout."""
    xp = np.asarray(xp, dtype=np.float64)
    out = np.asarray(out, dtype=np.float64)
    M, T, _ = out.shape
    units = 128
    h64 = np.zeros_like(out)
    bound = np.zeros_like(out)
    ug = GATE_ULPS * U32
    for d, suffix in enumerate(("", "_back")):
        U = np.asarray(w[layer + suffix + "/recurrent_kernel"], dtype=np.float64)
        c = np.zeros((M, units))
        dc = np.zeros((M, units))
        for t in range(T):
            tin = T - 1 - t if d else t
            hp = out[:, t - 1, d * units:(d + 1) * units] if t else np.zeros((M, units))
            x = xp[:, tin, d * 4 * units:(d + 1) * 4 * units]
            z = x + hp @ U
            dz = gamma(units + 1) * (np.abs(x) + np.abs(hp) @ np.abs(U))
            zi, zf, zg, zo = np.split(z, 4, axis=1)
            di_, df_, dg_, do_ = np.split(dz, 4, axis=1)

            def sig_b(zz, dd):
                s = _sig(zz)
                m = np.maximum(np.abs(zz) - dd, 0)
                return s, _sig(m) * (1 - _sig(m)) * dd + ug * s

            def tanh_b(zz, dd):
                s = np.tanh(zz)
                m = np.maximum(np.abs(zz) - dd, 0)
                return s, (1 - np.tanh(m) ** 2) * dd + ug * np.abs(s)

            i, di = sig_b(zi, di_)
            f, df = sig_b(zf, df_)
            g, dg = tanh_b(zg, dg_)
            o, do = sig_b(zo, do_)
            dc = (f + df) * dc + df * np.abs(c) + di * np.abs(g) + (i + di) * dg
            c = f * c + i * g
            dc += 3 * U32 * (np.abs(f * c) + np.abs(i * g))
            tc, dtc = tanh_b(c, dc)
            h = o * tc
            h64[:, t, d * units:(d + 1) * units] = h
            bound[:, t, d * units:(d + 1) * units] = do * np.abs(tc) + (o + do) * dtc + U32 * np.abs(h)
    return h64, bound


def stn_sample_f64(x, theta, slack_ulps=8):
    """The bilinear sampler (recognition.py:73-166, the clipped-corner weights of :144-152) in float64 on the feature map
    x (M, H, W, C) and theta (M, 6).  The coordinate x = 0.5 (x_s + 1) W is known to a few float32 ulp only (the device
    may contract the affine map), so where it lies within `dx` of an integer -- a corner or a clip
    boundary -- both corner choices are returned.  Returns (values, bound): values a list of (M, H, W, C) candidates, one
    per corner choice (one everywhere but at the ambiguous pixels), bound the interpolation bound
        (sum_i |w_i p_i|) 4 u + sum_i |p_i| dw_i,  dw from dx, dy through the other factor of each weight."""
    x = np.asarray(x, dtype=np.float64)
    th = np.asarray(theta, dtype=np.float64).reshape(-1, 6)
    M, H, W, C = x.shape
    xt = np.linspace(-1.0, 1.0, W)[None, None, :]
    yt = np.linspace(-1.0, 1.0, H)[None, :, None]
    t = [th[:, i].reshape(-1, 1, 1) for i in range(6)]
    fx = 0.5 * ((t[0] * xt + t[1] * yt) + t[2] + 1.0) * W
    fy = 0.5 * ((t[3] * xt + t[4] * yt) + t[5] + 1.0) * H
    dx = slack_ulps * U32 * 0.5 * W * (np.abs(t[0] * xt) + np.abs(t[1] * yt) + np.abs(t[2]) + 1.0)
    dy = slack_ulps * U32 * 0.5 * H * (np.abs(t[3] * xt) + np.abs(t[4] * yt) + np.abs(t[5]) + 1.0)
    mi = np.arange(M).reshape(-1, 1, 1)

    def interp(x0, y0):
        x1, y1 = x0 + 1, y0 + 1
        x0, x1 = np.clip(x0, 0, W - 1), np.clip(x1, 0, W - 1)
        y0, y1 = np.clip(y0, 0, H - 1), np.clip(y1, 0, H - 1)
        wts = [(x1 - fx) * (y1 - fy), (x1 - fx) * (fy - y0), (fx - x0) * (y1 - fy), (fx - x0) * (fy - y0)]
        dws = [dx * np.abs(y1 - fy) + dy * np.abs(x1 - fx), dx * np.abs(fy - y0) + dy * np.abs(x1 - fx),
               dx * np.abs(y1 - fy) + dy * np.abs(fx - x0), dx * np.abs(fy - y0) + dy * np.abs(fx - x0)]
        ps = [x[mi, y0, x0], x[mi, y1, x0], x[mi, y0, x1], x[mi, y1, x1]]
        val = sum(wi[..., None] * p for wi, p in zip(wts, ps))
        bnd = sum((4 * U32 * np.abs(wi)[..., None] + dw[..., None]) * np.abs(p) for wi, dw, p in zip(wts, dws, ps))
        return val, bnd

    cands = {(int(a), int(b)) for a in (-1, 1) for b in (-1, 1)}
    vals, bnds = [], []
    for sx, sy in sorted(cands):
        v, b = interp(np.floor(fx + sx * dx).astype(np.int64), np.floor(fy + sy * dy).astype(np.int64))
        vals.append(v)
        bnds.append(b)
    return vals, np.maximum.reduce(bnds)


def softmax_f64(logits):
    z = np.asarray(logits, dtype=np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def greedy_labels(logits, width):
    """keras ctc_decode greedy on the logits' argmax (lowest index on ties), blank = last class, -1 padded to width"""
    best = np.asarray(logits).argmax(-1)
    C = np.asarray(logits).shape[-1]
    out = np.full((best.shape[0], width), -1, dtype=np.int64)
    for m in range(best.shape[0]):
        k, prev = 0, -1
        for c in best[m]:
            if c != prev and c != C - 1:
                out[m, k] = c
                k += 1
            prev = c
    return out
