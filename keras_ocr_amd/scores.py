"""Confidence scores of the two networks ("Scores"; include/kocr.h: kocr_set_scores).

The reference returns none.  They are numbers it computes on the way and drops: the component maximum ``getBoxes`` compares
with ``detection_threshold``, and fc_12's softmax that the CTC decoder reduces to an arg-max."""
import collections
import math

import numpy as np

Score = collections.namedtuple("Score", ["detection", "word", "log_word", "characters"])
Score.__doc__ = """One word's scores.

detection: the maximum of the detector's text map over the box's connected component (float; ``None`` where no detector
    ran, as in ``Recognizer.recognize``).
word: ``exp(log_word)``, the probability the recogniser gives the returned text.
log_word: the log of the summed probability of every CTC alignment that collapses to the returned text (float).
characters: float32 array, one value per decoded label: the peak probability of that label over the frames that emitted it.
"""


def assemble(labels, log_word, char_scores, detection=None):
    """Rows of the recogniser's scores -> a list of ``Score``; ``labels``: the decoded label rows (-1 padded), ``detection``:
    one value per row or None."""
    lengths = (np.asarray(labels) >= 0).sum(axis=1) if len(labels) else []
    out = []
    for i, n in enumerate(lengths):
        lw = float(log_word[i])
        out.append(Score(None if detection is None else float(detection[i]), math.exp(lw), lw,
                         np.array(char_scores[i, :n], dtype=np.float32)))
    return out


def parameters(fn):
    """The parameter names of a (possibly duck-typed) stage's method; none where its signature cannot be read"""
    import inspect

    try:
        return inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return {}


def need(stage, obj, method):
    """The bound ``method`` of a (possibly duck-typed) stage if it takes ``return_scores``, else TypeError naming the stage."""
    fn = getattr(obj, method)
    if "return_scores" not in parameters(fn):
        raise TypeError(f"return_scores=True: the {stage} ({type(obj).__name__}.{method}) cannot give scores "
                        "(it takes no return_scores argument)")
    return fn
