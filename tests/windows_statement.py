"""The statement of long words ("Long words"; include/kocr_windows.h) in numpy: a box too wide for one
crop is read in overlapping windows.  The reference has no counterpart -- tools.warpBox fits every box into one 31 x 200 crop
-- so this file IS the definition; csrc/windows.hip and ctc_scores_ragged_kernel (csrc/crnn_kernels.hip) follow it.  Integers
are exact (Python ints), the geometry is float64 in the stated order, the stitch is a row selection, the decode is
tests/scores_statement.py on tests/ctc_statement.py, which take any number of frames.

Constants: the crop is CROP_H x CROP_W = 31 x 200, T = 50 frames of PX = 4 pixels, d = rnn_steps_to_discard.  ``frames`` and ``px``
are parameters ONLY so that tests/test_windows_statement_cpu.py can check the stitched decode against a sum over all paths on
a toy crop of 4 frames; the crop is then frames * px wide.
Parameters: aspect A (float64, finite, >= crop_w / 31), overlap O (a multiple of 2 px with 4 px <= O <= 24 px: 16 .. 96 in
steps of 8), S = crop_w - O, f = O / (2 px); ValueError when out of range or when d >= frames - f.

Per box, ob = get_rotated_box(box), (w, h) = the integers of get_rotated_width_height(ob) (a zero one: ZeroDivisionError):
  1. long iff float(w) > A * float(h); not long: K = 1, q_0 = ob.
  2. K = ceil((31 w - crop_w h) / (S h)) + 1, exact integers.
  3. window k spans [a_k, b_k] of the edges tl -> tr and bl -> br: a_k = (k S h) / (31 w), b_k = min(1, ((k S + crop_w) h) /
     (31 w)), each the correctly rounded float64 quotient of the two integers.
  4. the point at fraction a of p -> q: float32(float64(p) + (float64(q) - float64(p)) * a) per component; a == 0 is p itself,
     a == 1 is q itself.
  5. q_k = [top(a_k), top(b_k), bottom(b_k), bottom(a_k)]; behind it tests/orientation_statement.py's quad_params / crop.
  6. window k keeps the frames [lo_k, hi_k): lo_k = d if k == 0 else f, hi_k = frames if k == K - 1 else frames - f.
  7. T' = (K - 1) S / px + frames - d.
  8. T' > FRAMES_MAX is refused.
Stitch: row j of a word's sequence is the logit row of (window k, frame t), k upwards, t from lo_k to hi_k - 1.
Decode on the softmax of that sequence: scores_statement's greedy decode (first maximum, repeats merged -- across seams too --,
blank dropped), its character scores and its word log-probability over all T' frames."""
import numpy as np

from oracle import tools as otools
from tests import orientation_statement as os_
from tests import scores_statement as ss

CROP_H, CROP_W, T, PX = 31, 200, 50, 4
FRAMES_MAX = 2048
DEFAULT_ASPECT, DEFAULT_OVERLAP = 10.0, 40


def check_params(aspect, overlap, discard, frames=T, px=PX):
    crop_w = frames * px
    if not (np.isfinite(aspect) and aspect >= crop_w / CROP_H):
        raise ValueError(f"aspect {aspect}")
    if overlap != int(overlap) or overlap % (2 * px) or not 4 * px <= overlap <= 24 * px:
        raise ValueError(f"overlap {overlap}")
    if not 0 <= discard < frames - overlap // (2 * px):
        raise ValueError(f"discard {discard}")


def plan(w, h, aspect=DEFAULT_ASPECT, overlap=DEFAULT_OVERLAP, discard=2, frames=T, px=PX):
    """(K, [(a_k, b_k)], [(lo_k, hi_k)], T') of a box of w x h pixels"""
    check_params(aspect, overlap, discard, frames, px)
    w, h = int(w), int(h)
    if w == 0 or h == 0:
        raise ZeroDivisionError("division by zero")
    crop_w = frames * px
    stride, f = crop_w - overlap, overlap // (2 * px)
    num, den = CROP_H * w - crop_w * h, stride * h
    long_ = float(w) > float(aspect) * float(h) and num > 0  # num <= 0: A h rounded below crop_w h / 31, one window holds the box
    K = (num + den - 1) // den + 1 if long_ else 1
    if K == 1:
        fractions = [(0.0, 1.0)]
    else:
        fractions = [((k * stride * h) / (CROP_H * w), min(1.0, ((k * stride + crop_w) * h) / (CROP_H * w))) for k in range(K)]
    ranges = [(discard if k == 0 else f, frames if k == K - 1 else frames - f) for k in range(K)]
    return K, fractions, ranges, (K - 1) * (stride // px) + frames - discard


def edge_point(p, q, a):
    """the point at fraction a of the edge p -> q (float32 (2,) each)"""
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    if a == 0.0:
        return p.copy()
    if a == 1.0:
        return q.copy()
    return (p.astype(np.float64) + (q.astype(np.float64) - p.astype(np.float64)) * np.float64(a)).astype(np.float32)


def windows(box, aspect=DEFAULT_ASPECT, overlap=DEFAULT_OVERLAP, discard=2):
    """One box (4, 2): K, quads (K, 4, 2) float32, ranges (K, 2) int, T'"""
    ob, _ = otools.get_rotated_box(np.asarray(box, dtype=np.float32))
    ob = np.asarray(ob, np.float32)
    w, h = otools.get_rotated_width_height(ob)
    K, fractions, ranges, frames = plan(w, h, aspect, overlap, discard)
    if frames > FRAMES_MAX:
        raise ValueError(f"{frames} frames exceed {FRAMES_MAX}")
    if K == 1:
        return 1, ob[None].copy(), np.array(ranges), frames
    tl, tr, br, bl = ob
    quads = np.stack([np.stack([edge_point(tl, tr, a), edge_point(tl, tr, b), edge_point(bl, br, b), edge_point(bl, br, a)])
                      for a, b in fractions]).astype(np.float32)
    return K, quads, np.array(ranges), frames


def plan_boxes(boxes, aspect=DEFAULT_ASPECT, overlap=DEFAULT_OVERLAP, discard=2):
    """boxes (M, 4, 2): K (M,) int32, quads (sum K, 4, 2) float32, ranges (sum K, 2) int32, frames (M,) int32"""
    out = [windows(b, aspect, overlap, discard) for b in boxes]
    if not out:
        return np.zeros(0, np.int32), np.zeros((0, 4, 2), np.float32), np.zeros((0, 2), np.int32), np.zeros(0, np.int32)
    return (np.array([o[0] for o in out], np.int32), np.concatenate([o[1] for o in out]).astype(np.float32),
            np.concatenate([o[2] for o in out]).astype(np.int32), np.array([o[3] for o in out], np.int32))


def crops(image_u8, quads):
    """One RGB uint8 image and ordered source quads (n, 4, 2): crops (n, 31, 200) float32 gray / 255, each the oracle's warp
    of its quad (tests/orientation_statement.py: crop)"""
    gray = otools.rgb2gray_u8(image_u8)
    out = [os_.crop(gray, q) for q in quads]
    return np.array(out, dtype="float32").reshape(len(out), CROP_H, CROP_W) / 255


def stitch(logits, counts, overlap=DEFAULT_OVERLAP, discard=2, frames=T, px=PX):
    """logits (sum K, frames, C), counts (M,) = K per word: a list of M arrays (T'_m, C), rows selected, never recomputed"""
    logits = np.asarray(logits)
    f = overlap // (2 * px)
    out, at = [], 0
    for K in counts:
        K = int(K)
        rows = [logits[at + k, (discard if k == 0 else f):(frames if k == K - 1 else frames - f)] for k in range(K)]
        out.append(np.concatenate(rows))
        at += K
    assert at == len(logits)
    return out


def softmax(logits):
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def decode(seq):
    """one word's stitched logits (T', C): labels (list), character scores (float64 array, one per label), log_word, the
    probabilities (T', C) float64"""
    probs = softmax(seq)
    labels = [r[0] for r in ss.greedy_runs(probs)]
    chars = ss.char_scores(probs[None])[0][:len(labels)]
    return labels, chars, float(ss.log_word(probs[None])[0]), probs


def stitch_decode(logits, counts, overlap=DEFAULT_OVERLAP, discard=2, frames=T, px=PX):
    """per word (labels, chars, log_word, frames, no_ties)"""
    out = []
    for seq in stitch(logits, counts, overlap, discard, frames, px):
        labels, chars, logw, probs = decode(seq)
        out.append((labels, chars, logw, len(seq), ss.no_ties(probs)))
    return out
