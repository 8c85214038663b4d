"""The character-set statement of DESIGN.md section 4 ("Character sets: the statement and its status"), in float64 numpy.

A character set A is a non-empty subset of the non-blank classes [0, C - 2]; the blank C - 1 is always allowed.  A crop decoded
under A is decoded as if fc_12 had written -inf for every class outside A and the blank (`masked`), and everything behind that
is the existing statement on the masked row:

  greedy        the collapsed arg-max path of the masked row, ties to the smaller class (decode_cases.greedy)
  probs         the softmax of the masked row: masked classes are exactly 0
  log_q         ctc_statement.log_q of it: q_t = (p + 1e-7) / sum over ALL C classes -- a masked class keeps the floor
  log_word      minus the CTC loss of the greedy decode on those q_t (scores_statement.log_word)
  char_scores   entries of probs (scores_statement.char_scores)
  lexicon       the CTC log-probabilities of the words on those q_t (lexicon_statement.values): a word that uses a masked
                character keeps a finite, very small value -- it is not removed
  beam          a prefix is extended only by classes of A: beam_statement's search on the columns sorted(A) + [blank] of log_q
                (selected from the full-C q_t, NOT renormalised), ranked by the same columns of the logits, the labels mapped
                back through sorted(A).  The map is monotone, so both tie rules carry over; E = min(beam_width, |A|).

A = None is the unconstrained statement itself (set index -1 of the library)."""
import numpy as np

from tests import beam_statement as bs
from tests import ctc_statement as cs
from tests import decode_cases as dc
from tests import lexicon_statement as ls
from tests import scores_statement as ss


def check_set(allowed, classes):
    """sorted(A) as a list of ints; ValueError for an empty set or a class outside [0, classes - 2]"""
    a = sorted({int(c) for c in allowed})
    if not a:
        raise ValueError("a character set needs at least one class")
    if a[0] < 0 or a[-1] > classes - 2:
        raise ValueError(f"class {a[0] if a[0] < 0 else a[-1]} outside [0, {classes - 2}] (the blank is always allowed)")
    return a


def masked(lg, allowed):
    """logits (..., C) -> float64 logits with -inf outside A and the blank; allowed None: unchanged"""
    lg = np.array(lg, np.float64)
    if allowed is None:
        return lg
    keep = np.zeros(lg.shape[-1], bool)
    keep[check_set(allowed, lg.shape[-1])] = True
    keep[-1] = True
    lg[..., ~keep] = -np.inf
    return lg


def probs(lg, allowed):
    return dc.softmax(masked(lg, allowed))


def log_q(lg, allowed):
    """(To, C) logits -> (To, C) float64 log q_t of the masked rows, normalised over all C classes"""
    return cs.log_q(probs(lg, allowed)[None])[0]


def greedy(lg, allowed, last=False):
    return dc.greedy(masked(lg, allowed), last)


def log_word(lg, allowed):
    return float(ss.log_word(probs(lg, allowed)[None])[0])


def char_scores(lg, allowed):
    return ss.char_scores(probs(lg, allowed)[None])[0]


def lexicon_values(lg, allowed, labels, lengths):
    """(V,) float64"""
    return ls.values(log_q(lg, allowed)[None], labels, lengths)[0]


def beam(lg, allowed, beam_width, top_paths, larger_class_first=False, larger_row_first=False):
    """beam_statement.beam_search_ties under A -> (labels (top_paths, To) int64 in the recogniser's classes, log_prob, stats)"""
    lg = np.asarray(lg, np.float64)
    C = lg.shape[-1]
    cols = (list(range(C - 1)) if allowed is None else check_set(allowed, C)) + [C - 1]
    lq = log_q(lg, allowed)
    labels, log_prob, stats = bs.beam_search_ties(lq[:, cols], beam_width, top_paths, rank=lg[:, cols],
                                                  larger_class_first=larger_class_first, larger_row_first=larger_row_first)
    back = np.array(cols[:-1] + [-1])  # -1 (the padding) indexes the last entry
    return back[labels], log_prob, stats
