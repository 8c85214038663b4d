"""The statement of word orientation ("Orientation"): every box is read in two orientations and the
better reading is kept.  The reference has no counterpart -- its get_rotated_box always names the upper of the two leftmost
corners tl, so an upside-down word is read upside down and a vertical one as a sliver -- so this file IS the definition;
csrc/warp.hip (warp_prepare_turned_hd) and csrc/orient.hip (orient_select_kernel) follow it.  Plain numpy, float64 and
integers; the crop arithmetic is the oracle's (oracle/tools.py), applied to a renamed quad.

For one box (4 points, float32) in mode "flip" or "any" with ``tall_ratio``:
  1. ob = get_rotated_box(box), (w, h) = get_rotated_width_height(ob): what the crop stage computes today.
  2. tall = (mode == "any") and float(h) >= tall_ratio * float(w), in float64; the base turn b is 1 for a tall box, else 0.
  3. candidates c = 0, 1 have t_c = b + 2 c quarter turns: (0, 2), or (1, 3) for a tall box.
  4. candidate c is the source quad q_c[i] = ob[(i + t_c) % 4]: the same four float32 corners, renamed.  Turn 1 reads text
     running down the page, turn 3 up the page, turn 2 upside-down text.
  5. everything behind that is tools.warpBox's scalar half on q_c in place of ob: width and height come from q_c (they swap
     for odd turns), then scale, destination quad, homography, crop size and the warp; a zero width or height stays the
     reference's ZeroDivisionError.
  6. both crops go through the recogniser: a label row, its length n_c (labels >= 0) and the word log-probability v_c.
  7. candidate 1 wins iff (n_1 > 0 and n_0 == 0) or ((n_1 > 0) == (n_0 > 0) and v_1 > v_0)."""
import numpy as np

from oracle import tools as otools

MODES = ("flip", "any")
DEFAULT_TALL_RATIO = 1.5


def candidates(box, mode, tall_ratio=DEFAULT_TALL_RATIO):
    """turns (2,) int and quads (2, 4, 2) float32 of one box"""
    if mode not in MODES:
        raise ValueError(f"mode {mode!r} not in {MODES}")
    ob, _ = otools.get_rotated_box(np.asarray(box, dtype=np.float32))
    w, h = otools.get_rotated_width_height(ob)
    tall = mode == "any" and float(h) >= float(tall_ratio) * float(w)
    base = 1 if tall else 0
    turns = np.array([base, base + 2], dtype=np.int64)
    quads = np.stack([np.stack([ob[(i + t) % 4] for i in range(4)]) for t in turns]).astype(np.float32)
    return turns, quads


def quad_params(quad, target_height=31, target_width=200):
    """tools.warpBox's scalar half (oracle.tools.warp_box_params behind get_rotated_box) on an ordered quad: (w, h), scale,
    destination quad float32, M float64 3x3, crop dsize (cw, ch) before the paste clips it to the canvas"""
    quad = np.asarray(quad, dtype=np.float32)
    w, h = otools.get_rotated_width_height(quad)
    scale = min(target_width / w, target_height / h)  # ZeroDivisionError like the reference
    dst = np.array([[0, 0], [scale * w, 0], [scale * w, scale * h], [0, scale * h]]).astype("float32")
    M = otools.get_perspective_transform(quad, dst)
    return (w, h), scale, dst, M, (int(scale * w), int(scale * h))


def crop(gray_u8, quad, target_height=31, target_width=200):
    """oracle.tools.warp_box on an ordered quad: the warped gray crop pasted into a zero canvas, uint8"""
    _, _, _, M, dsize = quad_params(quad, target_height, target_width)
    warped = otools.warp_perspective_u8(gray_u8, M, dsize)
    full = np.zeros((target_height, target_width), dtype=np.uint8)
    full[: warped.shape[0], : warped.shape[1]] = warped[:target_height, :target_width]
    return full


def crops(image_u8, boxes, mode, tall_ratio=DEFAULT_TALL_RATIO, target_height=31, target_width=200):
    """One RGB uint8 image and its boxes (M, 4, 2): crops (2M, th, tw) float32 gray / 255, turns (2M,) int32, quads
    (2M, 4, 2) float32; crop 2m + c is candidate c of box m"""
    gray = otools.rgb2gray_u8(image_u8)
    out, turns, quads = [], [], []
    for box in boxes:
        t, q = candidates(box, mode, tall_ratio)
        for c in range(2):
            out.append(crop(gray, q[c], target_height, target_width))
            turns.append(int(t[c]))
            quads.append(q[c])
    m2 = len(out)
    return (np.array(out, dtype="float32").reshape(m2, target_height, target_width) / 255, np.array(turns, np.int32).reshape(m2),
            np.array(quads, np.float32).reshape(m2, 4, 2))


def select(labels, log_word):
    """labels (M, 2, L) integer rows (-1 padded), log_word (M, 2): winner (M,) in {0, 1}"""
    labels = np.asarray(labels)
    log_word = np.asarray(log_word)
    winner = np.zeros(len(labels), np.int64)
    for m in range(len(labels)):
        n0, n1 = int((labels[m, 0] >= 0).sum()), int((labels[m, 1] >= 0).sum())
        v0, v1 = log_word[m, 0], log_word[m, 1]
        winner[m] = 1 if (n1 > 0 and n0 == 0) or ((n1 > 0) == (n0 > 0) and bool(v1 > v0)) else 0
    return winner
