"""The CTC loss statement of DESIGN.md section 4, in float64 numpy, vectorised over the batch.

keras.backend.ctc_batch_cost(y_true, y_pred, input_length, label_length) feeds log(y_pred + 1e-7) to TF's ctc_loss
(time-major, preprocess_collapse_repeated=False, ctc_merge_repeated=True, blank = C - 1), which takes a softmax of it:
q_t(c) = (y[t, c] + eps) / sum_c' (y[t, c'] + eps).  The loss of sample m is -log of the summed probability of every path
over the first input_length[m] frames that collapses (repeats merged, blanks removed) to labels[m, :label_length[m]].
"""
import itertools

import numpy as np

EPS = 1e-7  # keras.backend.epsilon()


def log_q(y_pred):
    """(M, T, C) probabilities -> float64 log q of the statement."""
    y = np.asarray(y_pred, np.float64) + EPS
    return np.log(y) - np.log(y.sum(-1, keepdims=True))


def ctc_loss_logq(lq, labels, label_length, input_length):
    """The forward algorithm on float64 log q (M, T, C): loss (M,) float64, +inf where no path exists."""
    lq = np.asarray(lq, np.float64)
    M, _, C = lq.shape
    blank = C - 1
    L = np.asarray(label_length, np.int64).reshape(M)
    Tm = np.asarray(input_length, np.int64).reshape(M)
    lab = np.asarray(labels).reshape(M, -1)
    Lmax = int(L.max(initial=0))
    S = 2 * Lmax + 1
    s = np.arange(S)
    ext = np.full((M, S), blank, np.int64)
    if Lmax:
        body = np.where(np.arange(Lmax)[None, :] < L[:, None], lab[:, :Lmax], blank).astype(np.int64)
        ext[:, 1::2] = body
    live = s[None, :] < (2 * L + 1)[:, None]
    skip = np.zeros((M, S), bool)
    if S > 3:
        skip[:, 3:] = (s[3:] % 2 == 1)[None, :] & (ext[:, 3:] != ext[:, 1:-2])
    with np.errstate(divide="ignore", invalid="ignore"):
        la = np.full((M, S), -np.inf)
        g = np.take_along_axis(lq[:, 0, :], ext, axis=1)
        la[:, 0] = g[:, 0]
        if S > 1:
            la[:, 1] = np.where(L >= 1, g[:, 1], -np.inf)
        for t in range(1, int(Tm.max(initial=1))):
            a1 = np.concatenate([np.full((M, 1), -np.inf), la[:, :-1]], 1)
            a2 = np.where(skip, np.concatenate([np.full((M, 2), -np.inf), la[:, :-2]], 1), -np.inf)
            new = np.logaddexp(np.logaddexp(la, a1), a2) + np.take_along_axis(lq[:, t, :], ext, axis=1)
            new = np.where(live, new, -np.inf)
            la = np.where((t < Tm)[:, None], new, la)
        idx = np.arange(M)
        last = la[idx, 2 * L]
        prev = np.where(L > 0, la[idx, np.maximum(2 * L - 1, 0)], -np.inf)
        return -np.logaddexp(last, prev)


def ctc_loss(y_pred, labels, label_length, input_length):
    """The statement on probabilities y_pred (M, T, C): loss (M,) float64."""
    return ctc_loss_logq(log_q(y_pred), labels, label_length, input_length)


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(int(c))
        prev = c
    return out


def brute_force(y_pred, label, input_length):
    """-log sum over all C**T_m paths of one sample (y_pred (T, C)) that collapse to `label`."""
    lq = log_q(np.asarray(y_pred)[np.newaxis])[0][:input_length]
    C = lq.shape[1]
    total = 0.0
    for path in itertools.product(range(C), repeat=input_length):
        if collapse(path, C - 1) == list(label):
            total += np.exp(sum(lq[t, c] for t, c in enumerate(path)))
    return np.inf if total == 0.0 else -np.log(total)
