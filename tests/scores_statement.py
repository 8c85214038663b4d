"""The scores statement of DESIGN.md section 4 ("Scores"), in float64 numpy.

word log-probability   -tests/ctc_statement.py's loss of (probabilities, their greedy decode, all frames): the log of the
                       summed q-probability (q = the statement's renormalised y + eps) of every path that collapses to the
                       greedy decode;
character scores       for the k-th emitted label, the maximum of probs[t, label] over the frames of the run of arg-maxes
                       that emitted it (first maximum on ties), 0 behind the decode;
detection score        the maximum of the text map over the pixels of a box's connected component (scipy.ndimage.label,
                       cross structure), the component ids being those oracle.postproc.get_boxes reports for the kept boxes.
                       It is the number ``np.max`` gives and ``<`` compares with detection_threshold: a NaN anywhere in the
                       component makes it NaN, and a zero maximum is reported as +0.0 whatever the signs of the zeros it was
                       taken over (-0.0 == +0.0, and np.max may return either).
"""
import itertools

import numpy as np

from tests import ctc_statement as cs


def greedy_runs(probs):
    """(T, C) -> [(label, first frame, last frame + 1)] of the runs that emit a label: arg-max per frame (first maximum),
    a run = consecutive frames with the same non-blank arg-max."""
    path = np.asarray(probs).argmax(-1)
    blank = np.asarray(probs).shape[-1] - 1
    runs, t, T = [], 0, len(path)
    while t < T:
        e = t
        while e < T and path[e] == path[t]:
            e += 1
        if path[t] != blank:
            runs.append((int(path[t]), t, e))
        t = e
    return runs


def greedy_decode(probs):
    """(M, T, C) -> label rows (M, T) int64, -1 padded, and lengths (M,)."""
    probs = np.asarray(probs)
    M, T, _ = probs.shape
    rows = np.full((M, T), -1, np.int64)
    L = np.zeros(M, np.int64)
    for m in range(M):
        lab = [r[0] for r in greedy_runs(probs[m])]
        rows[m, :len(lab)] = lab
        L[m] = len(lab)
    return rows, L


def log_word(probs):
    """(M, T, C) probabilities -> float64 (M,): log of the summed probability of every alignment of the greedy decode."""
    probs = np.asarray(probs)
    rows, L = greedy_decode(probs)
    return -cs.ctc_loss(probs, rows, L, np.full(len(probs), probs.shape[1]))


def greedy_path_log_prob(probs):
    """(M, T, C) -> float64 (M,): the q-log-probability of the arg-max path alone (one of the decode's alignments)."""
    return cs.log_q(probs).max(-1).sum(-1)


def char_scores(probs):
    """(M, T, C) -> (M, T) of probs' dtype: per emitted label the maximum over its run of its probability, 0 behind."""
    probs = np.asarray(probs)
    out = np.zeros(probs.shape[:2], probs.dtype)
    for m in range(len(probs)):
        for k, (c, a, b) in enumerate(greedy_runs(probs[m])):
            out[m, k] = probs[m, a:b, c].max()
    return out


def brute_force_log_word(probs):
    """(T, C) one sample: log of the sum over all C**T paths that collapse to the greedy decode."""
    probs = np.asarray(probs)
    label = [r[0] for r in greedy_runs(probs)]
    lq = cs.log_q(probs[np.newaxis])[0]
    T, C = lq.shape
    total = 0.0
    for path in itertools.product(range(C), repeat=T):
        if cs.collapse(path, C - 1) == label:
            total += np.exp(sum(lq[t, c] for t, c in enumerate(path)))
    return np.log(total)


def no_ties(probs):
    """True when no frame has two exactly equal top probabilities (the arg-max is then unambiguous)."""
    srt = np.sort(np.asarray(probs), -1)
    return bool((srt[..., -1] > srt[..., -2]).all())


def detection_scores(heat, debug, text_threshold=0.4, link_threshold=0.4):
    """heat: (N, h, w, 2) float32; debug: oracle.postproc.get_boxes(..., return_debug=True)[1] for the SAME heat-maps and
    thresholds.  Returns per image a float32 array: max of the text map over each kept box's component (NaN if it holds one;
    a zero as +0.0)."""
    from scipy import ndimage

    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    out = []
    for y, dbg in zip(np.asarray(heat), debug):
        text = np.asarray(y[..., 0], np.float32)
        link = np.asarray(y[..., 1], np.float32)
        labels, _ = ndimage.label((text > np.float32(text_threshold)) | (link > np.float32(link_threshold)), structure=cross)
        out.append(np.array([text[labels == d["component"]].max() for d in dbg], np.float32) + np.float32(0))  # -0.0 + 0.0 = +0.0
    return out
