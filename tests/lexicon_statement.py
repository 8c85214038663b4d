"""The lexicon statement of DESIGN.md section 4 ("Lexicon"), in float64 numpy.

value[m, v] = -ctc_loss(q of crop m, labels of word v, all T frames) with tests/ctc_statement.py's forward algorithm on
log q_t (softmax + 1e-7, renormalised): the exact log-probability of the word given the crop, the sum over all its
alignments.  A word without an alignment -- it needs len + (adjacent equal pairs) frames, more than T -- is -inf.

top_words(value, K): per crop the K largest values; order: the higher value first, then the smaller lexicon index; -inf is
never returned (index -1, value -inf instead).  The decision margin of a crop is what a float32 evaluation must resolve for
that answer to be determined: the smallest gap between consecutive values among ranks 1 .. K + 1 (in the order above),
divided by max(1, |value at rank K + 1|) (by 1 where rank K + 1 does not exist or is -inf); +inf for a single word.
"""
import numpy as np

from tests import ctc_statement as cs


def frames_needed(word):
    word = list(word)
    return len(word) + sum(a == b for a, b in zip(word, word[1:]))


def values(lq, labels, lengths):
    """lq (M, T, C) float64 log q; labels (V, width) int, lengths (V,) -> value (M, V) float64, -inf where no path exists."""
    lq = np.asarray(lq, np.float64)
    labels, lengths = np.asarray(labels), np.asarray(lengths).reshape(-1)
    M, T, C = lq.shape
    V = len(labels)
    out = np.empty((M, V))
    for m in range(M):
        out[m] = -cs.ctc_loss_logq(np.broadcast_to(lq[m], (V, T, C)), labels, lengths, np.full(V, T))
    return out


def top_words(value, K):
    """value (M, V) -> index (M, K) int64 (-1 where fewer than K words are feasible), log_prob (M, K) (-inf there), margin (M,)."""
    value = np.asarray(value, np.float64)
    M, V = value.shape
    index = np.full((M, K), -1, np.int64)
    log_prob = np.full((M, K), -np.inf)
    margin = np.full(M, np.inf)
    for m in range(M):
        order = sorted(range(V), key=lambda v: (-value[m, v], v))
        ranked = value[m, order[:K + 1]]
        keep = [v for v in order[:K] if value[m, v] > -np.inf]
        index[m, :len(keep)] = keep
        log_prob[m, :len(keep)] = value[m, keep]
        scale = max(1.0, abs(ranked[K])) if len(ranked) > K and np.isfinite(ranked[K]) else 1.0
        for a, b in zip(ranked, ranked[1:]):
            if a == -np.inf:  # both -inf: nothing to resolve, neither is returned
                continue
            margin[m] = min(margin[m], (a - b) / scale)
    return index, log_prob, margin


def top_words_ties(value, K, larger_index_first=False):
    """top_words for inputs with exact ties -> index, log_prob, margin, ties (M,): a gap between two values that compare EQUAL
    in float64 is no margin -- the tie rule decides it on both sides -- and is counted in `ties` instead.
    larger_index_first turns the tie rule: the OPPOSITE rule, for showing that an input's answer hangs on it."""
    value = np.asarray(value, np.float64)
    M, V = value.shape
    index = np.full((M, K), -1, np.int64)
    log_prob = np.full((M, K), -np.inf)
    margin = np.full(M, np.inf)
    ties = np.zeros(M, np.int64)
    for m in range(M):
        order = sorted(range(V), key=lambda v: (-value[m, v], -v if larger_index_first else v))
        n = K + 1  # ranks 1 .. K + 1; where a tie straddles the cut, on to the first value that differs
        if V > K and value[m, order[K]] == value[m, order[K - 1]]:
            while n < V and value[m, order[n]] == value[m, order[K]]:
                n += 1
            n += 1
        ranked = value[m, order[:n]]
        keep = [v for v in order[:K] if value[m, v] > -np.inf]
        index[m, :len(keep)] = keep
        log_prob[m, :len(keep)] = value[m, keep]
        scale = max(1.0, abs(ranked[K])) if len(ranked) > K and np.isfinite(ranked[K]) else 1.0
        for a, b in zip(ranked, ranked[1:]):
            if a == -np.inf:
                continue
            if a == b:
                ties[m] += 1
            else:
                margin[m] = min(margin[m], (a - b) / scale)
    return index, log_prob, margin, ties
