"""Checkers of the recogniser's launches against their float64 statements (oracle/crnn.py), shared by the GPU audit
(tests/test_crnn_layers_gpu.py) and the CPU proof that they can fail (tests/test_crnn_layer_bounds_cpu.py).

Every checker takes one launch's recorded input and output and returns (max ratio, rms ratio) of |error| over the stated
bound of the kernel family that ran it; a launch passes with max <= 1 and rms <= RMS_GATE.  The rms gate is the finer
one: it holds the typical element to a quarter of the worst-case bound, so a defect that only a few elements show beyond
round-off -- one missing chunk of a long sum, one crop scaled by its neighbour -- fails it even where the max alone would
barely notice."""
import numpy as np

from oracle import crnn as ocrnn
from tests.layer_bounds import U32, pool2

RMS_GATE = 0.25
# dense_splitk_partial_kernel: 448-term fp32 fma chains (DSK_KCHUNK), then the 25 partials summed in order, then v * 1 + bias
DENSE_SPLITK_K = ocrnn.gamma(448 + 25 + 2)
# crnn_conv1_cells_kernel: a 9-term fp32 fma chain from the bias, then ReLU
CONV1_CELLS_K = ocrnn.gamma(9 + 1)
# ctc_kernel's softmax: expf within 2 ulp, a C-term sum, one division -- relative to p, (C + 8) u
CTC_ULPS = 8


def _ratios(err, allowed):
    r = err / np.maximum(allowed, 1e-300)
    return float(r.max()) if r.size else 0.0, float(np.sqrt((r ** 2).mean())) if r.size else 0.0


def check_conv(w, name, x, k, window=0, out=None, pool=None, amax=None, bn_eps=ocrnn.BN_EPS):
    """a convolution launch (Keras orientation): out (full) and / or pool (its 2x2 max pooling) against
    k bound + 2^-36 max|x| unit (tests/test_craft_layers_gpu.py)"""
    val, bnd, unit = ocrnn.layer_f64(w, name, x, window=window, bn_eps=bn_eps)
    if amax is None:
        amax = np.abs(x).reshape(x.shape[0], -1).max(axis=1)
    allowed = k * bnd + 2.0 ** -36 * np.asarray(amax, np.float64).reshape(-1, 1, 1, 1) * unit
    res = []
    if out is not None:
        res.append(_ratios(np.abs(out.astype(np.float64) - val), allowed))
    if pool is not None:
        res.append(_ratios(np.abs(pool.astype(np.float64) - pool2(val)), pool2(allowed)))
    return max(r[0] for r in res), max(r[1] for r in res)


def check_gemm(w, name, x, out, k):
    """a Dense-type launch (rows, K) -> (rows, N): |err| <= k bound"""
    val, bnd, _ = ocrnn.layer_f64(w, name, x)
    return _ratios(np.abs(out.reshape(val.shape).astype(np.float64) - val), k * bnd)


def check_lstm(w, layer, xp, out):
    """the recurrence, teacher-forced (oracle.crnn.lstm_teacher_forced)"""
    h64, bound = ocrnn.lstm_teacher_forced(w, layer, xp, out)
    return _ratios(np.abs(np.asarray(out, np.float64) - h64), bound)


def check_stn(x, theta, out):
    """the sampler against float64 bilinear interpolation at the corners the GPU chose (either choice where the
    coordinate is within a few ulp of an integer)"""
    vals, bnd = ocrnn.stn_sample_f64(x, theta)
    err = np.min([np.abs(out.astype(np.float64) - v) for v in vals], axis=0)
    return _ratios(err, bnd)


def check_ctc(logits, probs, discard):
    """probabilities against the float64 softmax of the GPU's own logits, relative bound (C + CTC_ULPS) u"""
    C = logits.shape[-1]
    p64 = ocrnn.softmax_f64(logits[:, discard:])
    # (+ 2^-126: below the smallest normal float32 a probability is only absolutely accurate)
    return _ratios(np.abs(probs.reshape(p64.shape).astype(np.float64) - p64), (C + CTC_ULPS) * U32 * p64 + 2.0 ** -126)
