"""The frozen (case, character set) pairs of the character-set tests: tests/decode_cases.py's chosen logits, each decoded under
sets that sit where the masked kernels can go wrong (csrc/crnn_kernels.hip: the MASKED instantiations).  Shared by
tests/test_charset_statement_cpu.py (which shows with the float64 statement alone that every pair compared on the GPU is
decidable) and tests/test_charsets_gpu.py.  Plain numpy, every seed fixed.

37 classes are one lane stripe and two mask words; 96 make a lane own c and c + 64 and cross the 32-bit mask words twice.
Both with the default discard (48 frames) and with another one (50 frames at 37 classes; 10 frames at 96, where the wide
beam is searched).

The kinds of set (`build`):
  all     every class: the statement is the unconstrained one, the kernels take the masked path with an all-ones mask
  one     exactly one class: E = 1 at every beam width
  high    96 classes only: classes >= 64 alone -- the first two mask words hold nothing, every lane's first class is masked
  word    the classes of the crop's spelled word (saturated family), filled up with others (16: E = B at width 16): the decode is the word
  miss    classes that are the raw arg-max of NO decoded frame: every non-blank frame's winner is masked
  twin    3 and its twin 7 (bit-equal columns) with others: where they top the allowed classes the maximum is an exact tie
|A| is 1, 3 and 10 against decode_cases.BEAM_PAIRS, so that E = |A| < B and E = B < |A| both occur.

An entry: ``case`` (decode_cases' dict), ``set`` (sorted tuple of classes), ``kind``, ``beam`` (the (beam_width, top_paths)
pairs), ``judge`` ("margin" / "lead" as in decode_cases), ``lexicon`` (whether the best TOP_WORDS lexicon indices are
compared: decidable by the statement; values are compared on every entry).  The seeds of the filled-up sets were chosen with the
statement alone, by scanning consecutive seeds from 0 for sets that are decidable at their beam widths."""
import functools

import numpy as np

from tests import decode_cases as dc

CONFIGS = [(37, 2), (37, 0), (96, 2), (96, 40)]
SAT = "saturated+30 word C={} d={}"
TWINS = {(37, 2): "twins 3->7 3->20 x3 C=37 d=2 seed=101", (37, 0): "twins 3->7 3->20 x3 C=37 d=0 seed=112",
         (96, 2): "twins 3->7 3->20 3->67 x3 C=96 d=2 seed=115", (96, 40): "twins 3->7 3->20 3->67 x5 C=96 d=40 seed=108"}
NARROW, WIDE = dc.NARROW, dc.WIDE


def build(case, kind, size, seed):
    """the sorted tuple of classes of one set"""
    C, d = case["classes"], case["discard"]
    rng = np.random.default_rng(1000 + seed)
    raw = case["logits"][d:].argmax(-1)

    def fill(base, pool):
        base = sorted(set(base))
        pool = [c for c in pool if c not in base]
        more = rng.choice(pool, size - len(base), replace=False) if size and size > len(base) else []
        return tuple(sorted(base + [int(c) for c in more]))

    if kind == "all":
        return tuple(range(C - 1))
    if kind == "one":
        return (int(next(c for c in raw if c != C - 1)),)
    if kind == "high":
        return fill([], range(64, C - 1)) if size else tuple(range(64, C - 1))
    if kind == "word":
        return fill([int(c) for c in case["path"] if c != C - 1], range(C - 1))
    if kind == "miss":
        return fill([], [c for c in range(C - 1) if c not in set(raw.tolist())])
    if kind == "twin":
        return fill([3, 7], [c for c in range(C - 1) if c not in (3, 7, 20, 67)])
    raise ValueError(kind)


# (case name, kind, |A| or None, seed, beam pairs, judge, lexicon indices compared)
def _entries():
    out = []
    for C, d in CONFIGS:
        sat, twin = SAT.format(C, d), TWINS[(C, d)]
        wide = d == 40
        pairs = WIDE if wide else NARROW
        out += [(sat, "all", None, 0, pairs, "lead", not wide),
                (twin, "all", None, 0, list(dc.by_name(twin)["beam"]), "margin", False),
                (sat, "one", 1, 0, dc.BEAM_PAIRS, "lead", True),
                (sat, "word", None, 0, pairs, "lead", True),
                (sat, "word", 16, SEEDS[(C, d, "word16")], dc.BEAM_PAIRS if wide else NARROW, "lead", True),
                (sat, "miss", 3, SEEDS[(C, d, "miss3")], dc.BEAM_PAIRS if wide else NARROW, "lead", False),
                (sat, "miss", 10, SEEDS[(C, d, "miss10")], pairs, "lead", False),
                (twin, "twin", 3, SEEDS[(C, d, "twin3")], dc.BEAM_PAIRS if wide else NARROW, "margin", False),
                (twin, "twin", 10, SEEDS[(C, d, "twin10")], pairs, "margin", False)]
        if C == 96:
            out += [(sat, "high", None, 0, pairs, "lead", False),
                    (sat, "high", 10, SEEDS[(C, d, "high10")], pairs, "lead", False)]
    return out


# the scanned seeds (module docstring): the first seed from 0 at which the entry is decidable at every one of its beam pairs
SEEDS = {
    (37, 2, "word16"): 0, (37, 2, "miss3"): 0, (37, 2, "miss10"): 0, (37, 2, "twin3"): 26, (37, 2, "twin10"): 1,
    (37, 0, "word16"): 0, (37, 0, "miss3"): 0, (37, 0, "miss10"): 0, (37, 0, "twin3"): 0, (37, 0, "twin10"): 0,
    (96, 2, "word16"): 0, (96, 2, "miss3"): 0, (96, 2, "miss10"): 0, (96, 2, "twin3"): 0, (96, 2, "twin10"): 1, (96, 2, "high10"): 0,
    (96, 40, "word16"): 2, (96, 40, "miss3"): 0, (96, 40, "miss10"): 0, (96, 40, "twin3"): 0, (96, 40, "twin10"): 0, (96, 40, "high10"): 0,
}


@functools.lru_cache(maxsize=None)
def pairs():
    out = []
    for name, kind, size, seed, beam, judge, lexicon in _entries():
        case = dc.by_name(name)
        allowed = build(case, kind, size, seed)
        assert allowed and (size is None or len(allowed) == size), (name, kind, size, allowed)
        out.append(dict(case=case, set=allowed, kind=kind, beam=[tuple(p) for p in beam], judge=judge, lexicon=lexicon,
                        name=f"{name} | {kind}{'' if size is None else size}"))
    assert len({p["name"] for p in out}) == len(out)
    return tuple(out)


def of_config(classes, discard):
    return [p for p in pairs() if (p["case"]["classes"], p["case"]["discard"]) == (classes, discard)]


def table(entries, classes):
    """the entries' sets as kocr_set_charsets takes them: (S, classes - 1) uint8"""
    allowed = np.zeros((len(entries), classes - 1), np.uint8)
    for s, p in enumerate(entries):
        allowed[s, list(p["set"])] = 1
    return allowed


# ---- the statement on an entry, computed once and shared ---------------------------------------------------------------------

def by_name(name):
    return next(p for p in pairs() if p["name"] == name)


@functools.lru_cache(maxsize=None)
def beam(name, beam_width, top_paths, larger_class_first=False, larger_row_first=False):
    from tests import charset_statement as st

    p = by_name(name)
    return st.beam(dc.decoded(p["case"]), p["set"], beam_width, top_paths, larger_class_first, larger_row_first)


@functools.lru_cache(maxsize=None)
def lexicon_values(name):
    from tests import charset_statement as st

    p = by_name(name)
    labels, lengths = dc.rows(dc.lexicon(p["case"]["classes"]))
    return st.lexicon_values(dc.decoded(p["case"]), p["set"], labels, lengths)
