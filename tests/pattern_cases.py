"""The frozen (case, pattern) pairs of the pattern tests: tests/decode_cases.py's chosen logits, each decoded under regular
expressions that sit where pattern_viterbi_kernel can go wrong.  Shared by tests/test_patterns_cpu.py (which shows with the
float64 statement alone that every pair compared on the GPU is decidable, or an exact tie that only the tie rule resolves) and
tests/test_patterns_gpu.py.  Plain numpy, nothing read from a file.

37 classes are the digits and the lower-case letters; 96 add the capitals, the punctuation and the space.  Discards 0, 2 and
40: 50, 48 and 10 decoded frames.  The patterns (`PATTERNS`): one state (``.*``, ``\\d*``, ``[a-z]*``); 2 to 13 states (a
plate, a date, the shape of the saturated crops' word); ``.{11}`` / ``.{12}``, whose 396 / 432 nodes cross the workgroup's
256 lanes; and ``.{0,40}`` at 96 classes, 41 states and 3841 nodes, whose back-pointers leave LDS.

An entry: ``case`` (decode_cases' dict), ``pattern`` (a name of PATTERNS[classes]), ``kind``:
  margin  the statement's decision margin exceeds its bound (pattern_statement.decidable): labels must equal
  tie     an exact tie between twin columns: the stated rule and the opposite rule give different texts of equal log_path,
          and the next distinct alignment value (pattern_statement.next_value) lies further below than the bound
  nofit   no accepted text fits the frames: the row is -1 / -inf
What decides the kind: `saturated+30` crops are decidable only under patterns their text satisfies -- a contradicting pattern
pushes the choice onto the 1e-7 floor, where float32 sees exact ties (``.{11}`` on the 12-letter word: margin 8e-6 against a
bound of 1.5e-3); the `saturated+8` crop is decidable under contradicting patterns as well; the twins are ties wherever the
pattern allows two of them and decidable where it allows one."""
import functools
import string

import numpy as np

from keras_ocr_amd import patterns as kp
from tests import decode_cases as dc
from tests import pattern_statement as ps

ALPHABETS = {37: string.digits + string.ascii_lowercase,
             96: string.digits + string.ascii_lowercase + string.ascii_uppercase + string.punctuation + " "}
CONFIGS = [(37, 2), (37, 0), (96, 2), (96, 40)]

# the saturated "word" crops spell h44n9u1cz8l3 (decode_cases.WORD), h44 at 10 frames
WORD_SHAPE = r"[a-z]\d{2}[a-z]\d[a-z]\d[a-z]{2}\d[a-z]\d"
PATTERNS = {
    37: {"any": r".*", "digits": r"\d*", "letters": r"[a-z]*", "letters+": r"[a-z]+", "plate": r"[a-z]{2}\d{2}[a-z]{3}",
         "code": r"\d{2}[a-z]\d{2}", "shape": WORD_SHAPE, "eleven": r".{11}", "twelve": r".{12}", "h..3": r"h.*3",
         "empty-or-digits": r"(\d{4})?"},
    96: {"any": r".*", "digits": r"\d*", "letters+": r"[a-z]+", "date": r"\d{2}/\d{2}/\d{4}", "shape": WORD_SHAPE,
         "upto40": r".{0,40}", "eleven": r".{11}", "short": r"[a-z]\d{2}", "caps": r"[A-Z]{2}\d+"},
}

SAT = "saturated+30 word C={} d={}"
BLANK = "saturated+30 all-blank C={} d={}"
SOFT = "saturated+8 word C=37 d=2"
TWINS = {(37, 2): "twins 3->7 3->20 x3 C=37 d=2 seed=101", (37, 0): "twins 3->7 3->20 x3 C=37 d=0 seed=112",
         (96, 2): "twins 3->7 3->20 3->67 x3 C=96 d=2 seed=115", (96, 40): "twins 3->7 3->20 3->67 x5 C=96 d=40 seed=108"}

# (case name, pattern name, kind)
ENTRIES = [
    # 37 classes, 48 frames
    (SAT.format(37, 2), "any", "margin"), (SAT.format(37, 2), "shape", "margin"), (SAT.format(37, 2), "twelve", "margin"),
    (SAT.format(37, 2), "h..3", "margin"), (BLANK.format(37, 2), "empty-or-digits", "margin"), (BLANK.format(37, 2), "any", "margin"),
    (SOFT, "any", "margin"), (SOFT, "letters", "margin"), (SOFT, "digits", "margin"), (SOFT, "eleven", "margin"),
    (SOFT, "plate", "margin"), (SOFT, "code", "margin"),
    (TWINS[(37, 2)], "any", "tie"), (TWINS[(37, 2)], "digits", "tie"), (TWINS[(37, 2)], "letters+", "margin"),
    # 37 classes, 50 frames
    (SAT.format(37, 0), "any", "margin"), (SAT.format(37, 0), "shape", "margin"), (SAT.format(37, 0), "twelve", "margin"),
    (TWINS[(37, 0)], "digits", "tie"), (TWINS[(37, 0)], "eleven", "tie"), (TWINS[(37, 0)], "letters+", "margin"),
    # 96 classes, 48 frames
    (SAT.format(96, 2), "any", "margin"), (SAT.format(96, 2), "shape", "margin"), (SAT.format(96, 2), "upto40", "margin"),
    (TWINS[(96, 2)], "digits", "tie"), (TWINS[(96, 2)], "letters+", "margin"), (TWINS[(96, 2)], "caps", "tie"),
    (TWINS[(96, 2)], "date", "tie"), (TWINS[(96, 2)], "upto40", "tie"),
    # 96 classes, 10 frames
    (SAT.format(96, 40), "short", "margin"), (SAT.format(96, 40), "upto40", "margin"), (SAT.format(96, 40), "eleven", "nofit"),
    (TWINS[(96, 40)], "date", "tie"), (TWINS[(96, 40)], "upto40", "tie"), (TWINS[(96, 40)], "digits", "tie"), (TWINS[(96, 40)], "letters+", "margin"),
]


@functools.lru_cache(maxsize=None)
def compiled(classes):
    """the patterns of one class count: keras_ocr_amd.patterns.Patterns"""
    return kp.Patterns(ALPHABETS[classes], PATTERNS[classes])


def dfa(classes, pattern):
    pats = compiled(classes)
    i = pats.names.index(pattern)
    return pats.delta[i], pats.accept[i]


def twin_classes(case):
    """class -> representative for the columns a twins case copies (None for the other families)"""
    if case["family"] != "twins":
        return None
    lg = case["logits"]
    same = {}
    for c in range(lg.shape[1] - 1):
        for r in range(c):
            if np.array_equal(lg[:, r], lg[:, c]):
                same[c] = r
                break
    return same


@functools.lru_cache(maxsize=None)
def pairs():
    out = []
    for name, pattern, kind in ENTRIES:
        case = dc.by_name(name)
        assert pattern in PATTERNS[case["classes"]], (name, pattern)
        out.append(dict(case=case, pattern=pattern, kind=kind, name=f"{name} | {pattern}"))
    assert len({p["name"] for p in out}) == len(out)
    return tuple(out)


def of_config(classes, discard):
    return [p for p in pairs() if (p["case"]["classes"], p["case"]["discard"]) == (classes, discard)]


def by_name(name):
    return next(p for p in pairs() if p["name"] == name)


# ---- the statement on a pair, computed once and shared ---------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def decode(name, last=False):
    """pattern_statement.viterbi of a pair: (log_path, labels or None)"""
    p = by_name(name)
    d, a = dfa(p["case"]["classes"], p["pattern"])
    return ps.viterbi(dc.log_q(p["case"]["name"]), d, a, last)


@functools.lru_cache(maxsize=None)
def margin(name):
    """log_path - runner_up of a pair, the twins' tie classes counted as one text"""
    p = by_name(name)
    value, labels = decode(name)
    return value - ps.runner_up(dc.log_q(p["case"]["name"]), dfa(p["case"]["classes"], p["pattern"]), labels, twin_classes(p["case"]))
