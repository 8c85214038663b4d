"""Logits chosen to sit where the CTC kernels behind fc_12 can go wrong (csrc/crnn_kernels.hip: ctc_kernel, ctc_scores_kernel,
ctc_beam_kernel, ctc_loss_kernel<true>, the three lexicon kernels), shared by tests/test_decode_cases_cpu.py (which shows with
the float64 statements alone that every case is decidable and exercises the rule it is there for) and
tests/test_decode_edges_gpu.py (which holds the kernels to the statements through kocr_crnn_decode_logits).  Plain numpy,
every seed fixed, nothing read from a file.

A case is a dict: ``name``; ``family``; ``classes`` / ``discard`` -- the recogniser it is decoded under (C classes, blank
C - 1, rows discard .. 49 of the 50 frames decoded: To = 50 - discard); ``logits`` (50, C) float32, read-only; ``path`` -- the
class the construction puts on top of each decoded frame, where there is one; ``beam`` -- the (beam_width, top_paths) pairs it
is searched with; ``judge`` -- "margin": every row must equal the statement's, the tie-aware decision margin
(beam_statement.beam_search_ties) exceeds bound(To); "lead": row 0 alone, the lead margin exceeds it (saturated crops: their
lower rows are near-ties of floor-level candidates, margins around 1e-12 of the bound at every width); ``ties`` -- whether it
is there for a tie rule (then it meets an exact tie and the opposite rule gives another answer); ``same_as`` -- the case whose
results it must reproduce bit for bit (the shifted crops).

The families ("Chosen logits"):
  saturated   N(0, 1) noise plus 30 (or 8) on one class per frame: what a trained recogniser gives.  In float32 the softmax
              of a wrong class underflows against 1e-7 and q sits on the floor.
  floor       frames whose losers lie 40, 90 and 200 below the winner (at 90 float32's softmax is subnormal, at 200 expf is
              exactly 0), on a grid of 2^-10; and the same crop with +1e4 / -1e4 added to every logit of some frames, which is
              exactly representable on that grid: the results must be the same bits.
  twins       soft logits (N(0, 1) times a scale) with one column copied bit for bit into others: prefixes / words that differ
              by swapping the twins have equal values in float64 and, by the symmetry of the arithmetic, on the GPU; only the
              tie rule separates them.  3 -> 7 and 3 -> 20 sit on different lanes, 3 -> 67 (96 classes) on the same lane,
              blank -> 5 makes a letter the blank's twin.
  flat        frames with all C logits equal: every arg-max is a tie.
  soft        plain soft logits at 4 classes and 3 frames, small enough to enumerate all 4^3 alignments.
The twins' seeds were chosen with the statements alone, by scanning consecutive seeds for crops that are decidable at the
widths they are used with, meet an exact tie and change under the opposite rule."""
import functools

import numpy as np

F32 = np.float32
T = 50
GATE = 1e-6  # tests/test_ctc_loss_gpu.py
MAX_WORD = 32  # KOCR_LEXICON_MAX_WORD
BEAM_PAIRS = [(4, 1), (4, 3), (16, 3), (64, 3), (64, 64)]
NARROW = [(4, 1), (4, 3), (16, 3)]


def bound(frames):
    """twice the gate of one CTC total: a decision compares two (tests/test_beam_gpu.py's margin_bound)"""
    return 2 * GATE * frames


def _frozen(a):
    a = np.ascontiguousarray(a, F32)
    a.flags.writeable = False
    return a


def spell(word, frames, blank, rng):
    """a frame path that collapses to `word`: runs of 1 - 4 frames per letter, 0 - 2 blanks between (at least one between equal
    letters), shrunk until it fits, blanks behind"""
    runs = [int(r) for r in rng.integers(1, 5, len(word))]
    gaps = [int(g) for g in rng.integers(0, 3, len(word))]  # gaps[i]: blanks before letter i
    need = [1 if i and word[i] == word[i - 1] else 0 for i in range(len(word))]
    gaps = [max(g, n) for g, n in zip(gaps, need)]
    while sum(runs) + sum(gaps) > frames:
        i = int(np.argmax(runs))
        j = int(np.argmax([g - n for g, n in zip(gaps, need)]))
        if runs[i] > 1:
            runs[i] -= 1
        elif gaps[j] > need[j]:
            gaps[j] -= 1
        else:
            raise ValueError("the word does not fit")
    path = []
    for c, r, g in zip(word, runs, gaps):
        path += [blank] * g + [int(c)] * r
    return path + [blank] * (frames - len(path))


def saturated(classes, discard, path, boost, seed):
    """noise everywhere; `boost` on path[t] in decoded frame t, and on class 0 in the discarded frames (a kernel that read
    them would decode another row)"""
    rng = np.random.default_rng(seed)
    lg = rng.normal(0, 1, (T, classes)).astype(F32)
    lg[:discard, 0] += F32(boost)
    lg[np.arange(discard, T), path] += F32(boost)
    return lg


def floor(classes, discard, seed):
    """grid noise in [-1, 1]; the losers of frame t are moved (40, 90, 200)[t % 3] down"""
    rng = np.random.default_rng(seed)
    lg = (rng.integers(-1024, 1025, (T, classes)) / 1024.0).astype(F32)
    path = spell([int(c) for c in rng.integers(0, classes - 1, 9)], T - discard, classes - 1, rng)
    win = np.array([0] * discard + path)
    depth = np.array([40.0, 90.0, 200.0], F32)[np.arange(T) % 3]
    lg -= depth[:, None]
    lg[np.arange(T), win] += depth
    return lg, path


def twins(classes, seed, scale, copies):
    rng = np.random.default_rng(seed)
    lg = (rng.normal(0, 1, (T, classes)) * scale).astype(F32)
    for src, dst in copies:
        lg[:, dst] = lg[:, src]
    return lg


FIVE = (3, 7, 20, 25, 30)


def straddle(classes, seed, scale, every=6):
    """five twins 3 = 7 = 20 = 25 = 30 whose shared logit is, in every `every`-th frame, 1 above every other class: at beam
    width 4 the pruning keeps E = 4 classes, so its cut runs THROUGH the five and its tie rule (the smaller class) picks the
    four that are extended -- 30 is dropped; under the opposite rule 3 is, and the best path spells another twin"""
    lg = twins(classes, seed, scale, [(3, c) for c in FIVE[1:]])
    others = [c for c in range(classes) if c not in FIVE]
    for t in range(1, T, every):
        lg[t, list(FIVE)] = lg[t, others].max() + F32(1)
    return lg


def _case(name, family, classes, discard, logits, path=None, beam=(), judge="margin", ties=False, same_as=None):
    logits = _frozen(logits)
    assert logits.shape == (T, classes)
    return dict(name=name, family=family, classes=classes, discard=discard, logits=logits, path=path, beam=list(beam), judge=judge,
                ties=ties, same_as=same_as)


# the word of the saturated "word" crops and of the saturated lexicon: 12 letters, a double letter inside
WORD = [17, 4, 4, 23, 9, 30, 1, 12, 35, 8, 21, 3]


def _saturated_set(classes, discard, beam, seed, boosts=(30,), wide=()):
    """the saturated crops of one recogniser; those named in `wide` are searched at beam width 64 as well"""
    To, blank = T - discard, classes - 1
    rng = np.random.default_rng(seed)
    word = [c % blank for c in WORD][:max(1, min(12, To // 3))]
    paths = {
        "word": spell(word, To, blank, rng),
        "double": spell([1 % blank, 1 % blank, 0, 0, 2 % blank, 2 % blank], To, blank, rng) if To >= 12 else spell([0, 0], To, blank, rng),
        "one-letter": [2 % blank] * To,
        "all-blank": [blank] * To,
        "full-width": [t % blank for t in range(To)],  # another non-blank class in every frame: To labels, S = 2 To + 1 states
    }
    out = []
    for boost in boosts:
        for i, (what, path) in enumerate(paths.items()):
            if boost != 30 and what not in ("word", "full-width"):
                continue
            pairs = list(beam) + ([p for p in BEAM_PAIRS if p not in beam] if f"{what}+{boost}" in wide else [])
            out.append(_case(f"saturated+{boost} {what} C={classes} d={discard}", "saturated", classes, discard,
                             saturated(classes, discard, path, boost, seed * 100 + boost + i), path, pairs, judge="lead"))
    return out


# twins: (classes, discard, seed, scale, copies, beam pairs) -- see the module docstring for how the seeds were found: of 24 - 30
# consecutive seeds from 100 the scan kept about half at beam width 4, a quarter at 16 and one in six at 64 (scale 5 there: a
# larger scale widens the margins); at 96 classes and 48 frames no seed of 16 was decidable at width 64 (scales 5 and 8), so
# the wide beam meets 96 classes on 10 frames (discard 40), 65 classes (E = 64 = C - 1: nothing is pruned) likewise
WIDE = [(64, 3), (64, 64)]
THREE, FOUR = [(3, 7), (3, 20)], [(3, 7), (3, 20), (3, 67)]
TWINS = [
    (37, 2, 101, 3, THREE, NARROW),
    (37, 2, 106, 3, THREE, [(4, 1), (4, 3)]),
    (37, 2, 110, 3, THREE, NARROW),
    (37, 2, 123, 3, THREE, NARROW),
    (37, 2, 106, 5, THREE, WIDE),
    (37, 2, 111, 5, THREE, WIDE),
    (37, 0, 112, 3, THREE, NARROW),
    (37, 0, 110, 3, THREE, NARROW),
    (64, 2, 109, 3, THREE, NARROW),
    (64, 2, 110, 3, THREE, NARROW),
    (65, 2, 110, 3, THREE, NARROW),
    (65, 2, 107, 3, THREE, NARROW),
    (65, 40, 103, 5, THREE, WIDE),
    (96, 2, 115, 3, FOUR, [(4, 1), (4, 3)]),
    (96, 2, 123, 3, FOUR, [(4, 1), (4, 3)]),
    (96, 2, 114, 3, FOUR, NARROW),
    (96, 2, 133, 3, FOUR, [(16, 3)]),
    (96, 40, 108, 5, FOUR, WIDE),
    (96, 40, 101, 5, FOUR, WIDE),
]
# straddle: (classes, discard, seed, scale); beam width 4
STRADDLE = [(37, 2, 102, 3), (37, 2, 107, 3), (96, 2, 110, 3), (96, 2, 111, 3)]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # 37 classes, the default discard: every family
    out += _saturated_set(37, 2, NARROW, 1, boosts=(30, 8), wide=("word+30", "full-width+30", "word+8"))
    lg, path = floor(37, 2, 2)
    out.append(_case("floor C=37 d=2", "floor", 37, 2, lg, path, BEAM_PAIRS, judge="lead"))
    shifted = lg.copy()
    shifted[5:T:4] += F32(1e4)
    shifted[7:T:4] -= F32(1e4)
    shifted[0] += F32(1e4)  # a discarded frame
    out.append(_case("floor shifted C=37 d=2", "floor", 37, 2, shifted, path, NARROW, judge="lead", same_as="floor C=37 d=2"))
    # other discards: the full-width label at 50 frames (S = 101), 45 frames
    out += _saturated_set(37, 0, NARROW, 3)
    out += _saturated_set(37, 5, NARROW, 4)
    lg, path = floor(37, 5, 5)
    out.append(_case("floor C=37 d=5", "floor", 37, 5, lg, path, NARROW, judge="lead"))
    # the blank on lane 63, on lane 0's second class, and two classes per lane
    for classes, seed in ((64, 6), (65, 7), (96, 8), (4, 9)):
        out += _saturated_set(classes, 2, NARROW, seed, boosts=(30, 8) if classes == 4 else (30,))
    # the wide beam on 10 frames: E = 64 = C - 1 at 65 classes (nothing pruned), 64 of 95 at 96
    for classes, seed in ((65, 12), (96, 13)):
        out += [c for c in _saturated_set(classes, 40, WIDE, seed) if " word " in c["name"] or " full-width " in c["name"]]
    # flat frames: greedy, scores, loss and lexicon values (a beam search of them is one tie after another, by symmetry and
    # not: no decidable case)
    for classes in (37, 64, 65, 96, 4):
        out.append(_case(f"flat C={classes} d=2", "flat", classes, 2, np.full((T, classes), 0.5, F32), ties=True))
        mixed = saturated(classes, 2, spell([c % (classes - 1) for c in WORD[:6]], T - 2, classes - 1, np.random.default_rng(10)), 30, 11)
        mixed[3:T:3] = F32(-1.25)
        out.append(_case(f"flat and saturated C={classes} d=2", "flat", classes, 2, mixed, ties=True))
    for classes, discard, seed, scale, copies, beam in TWINS:
        tag = " ".join(f"{a}->{b}" for a, b in copies)
        out.append(_case(f"twins {tag} x{scale} C={classes} d={discard} seed={seed}", "twins", classes, discard,
                         twins(classes, seed, scale, copies), None, beam, ties=True))
    for classes, discard, seed, scale in STRADDLE:
        out.append(_case(f"twins straddle x{scale} C={classes} d={discard} seed={seed}", "twins", classes, discard,
                         straddle(classes, seed, scale), None, [(4, 1), (4, 3)], ties=True))
    # the blank's column copied into a letter: no beam tie (a blank is no letter), but every arg-max of the two is one
    out.append(_case("twins 36->5 x3 C=37 d=2 seed=100", "twins", 37, 2, twins(37, 100, 3, [(36, 5)]), None, [], ties=True))
    # 4 classes, 3 frames: everything can be enumerated
    for seed in (0, 1, 2):
        out.append(_case(f"soft C=4 d=47 seed={seed}", "soft", 4, 47, twins(4, 20 + seed, 2.0, []), None, [(64, 64), (4, 3)]))
    out.append(_case("twins 0->1 x2 C=4 d=47 seed=23", "twins", 4, 47, twins(4, 23, 2.0, [(0, 1)]), None, [(64, 64)], ties=True))
    out.append(_case("saturated+30 C=4 d=47", "saturated", 4, 47, saturated(4, 47, [1, 3, 1], 30, 24), [1, 3, 1], [(64, 64)], judge="lead"))
    names = [c["name"] for c in out]
    assert len(names) == len(set(names))
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def configs():
    """the (classes, discard) pairs of the cases, in first-use order"""
    return list(dict.fromkeys((c["classes"], c["discard"]) for c in cases()))


def of_config(classes, discard, family=None):
    return [c for c in cases() if (c["classes"], c["discard"]) == (classes, discard) and family in (None, c["family"])]


# ---- what the statements take ---------------------------------------------------------------------------------------------

def decoded(case):
    """the decoded frames of a case as float64 logits (To, C)"""
    return case["logits"][case["discard"]:].astype(np.float64)


def softmax(lg):
    e = np.exp(lg - lg.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def greedy(lg, last=False):
    """the collapsed arg-max path of logits (To, C), -1 padded: first maximum (last: the OPPOSITE rule, the last one)"""
    lg = np.asarray(lg)
    To, C = lg.shape
    best = C - 1 - lg[:, ::-1].argmax(-1) if last else lg.argmax(-1)
    row, prev = [], -1
    for c in best:
        if c != prev and c != C - 1:
            row.append(int(c))
        prev = c
    return np.array(row + [-1] * (To - len(row)), np.int64)


# ---- lexicons ---------------------------------------------------------------------------------------------------------------

def _far(word, distance, blank, rng):
    """`word` with `distance` letters replaced by other classes"""
    out = list(word)
    for i in rng.choice(len(word), distance, replace=False):
        out[i] = int((out[i] + 1 + rng.integers(0, blank - 1)) % blank)
    return out


def saturated_lexicon(classes, longest=MAX_WORD):
    """for the saturated crops of (classes, discard 2): the word itself, words 1, 3, 6 and 12 letters away, a one-letter
    word, a word of `longest` letters that fits and (longest permitting) words that cannot fit 48 frames"""
    blank = classes - 1
    rng = np.random.default_rng(31)
    word = [c % blank for c in WORD][:min(12, longest)]
    words = [word] + [_far(word, d, blank, rng) for d in (1, 3, 6, 12) if d <= len(word)]
    words += [[word[0]], [2 % blank], [(3 * i) % blank if blank > 3 else i % blank for i in range(longest)]]
    words += [[1 % blank, 1 % blank, 0, 0, 2 % blank, 2 % blank][:longest]]
    if longest >= 26:
        words += [[7 % blank] * longest, [5 % blank, 5 % blank] * 13]  # 63 resp. 51 frames
    return words


def rows(words):
    """labels (V, width) int32 -1 padded, lengths (V,) int32"""
    width = max(len(w) for w in words)
    labels = np.full((len(words), width), -1, np.int32)
    for i, w in enumerate(words):
        labels[i, :len(w)] = w
    return labels, np.array([len(w) for w in words], np.int32)


def twin_words(rng, n, blank, a, b, longest=8):
    """n random words that hold `a`, each followed by its twin (every a <-> b swapped): pairs of equal value under a -> b twins"""
    words = []
    while len(words) < 2 * n:
        w = [int(c) for c in rng.integers(0, blank, int(rng.integers(1, longest + 1)))]
        w[int(rng.integers(0, len(w)))] = a
        swap = [b if c == a else a if c == b else c for c in w]
        if w not in words and swap not in words and w != swap:
            words += [swap, w] if len(words) % 4 else [w, swap]
    return words


# ---- the statements on a case, computed once and shared by the tests that need them --------------------------------------

@functools.lru_cache(maxsize=None)
def log_q(name):
    from tests import ctc_statement as cs

    return cs.log_q(softmax(decoded(by_name(name)))[None])[0]


@functools.lru_cache(maxsize=None)
def _frames(name, beam_width, larger_class_first, larger_row_first):
    from tests import beam_statement as bs

    return bs.beam_frames(log_q(name), beam_width, decoded(by_name(name)), larger_class_first, larger_row_first)


@functools.lru_cache(maxsize=None)
def beam(name, beam_width, top_paths, larger_class_first=False, larger_row_first=False):
    """beam_statement.beam_search_ties of a case (the logits rank the classes, as on the GPU): labels, log_prob, stats"""
    from tests import beam_statement as bs

    final, stats = _frames(name, beam_width, larger_class_first, larger_row_first)
    return bs.beam_paths(log_q(name), final, top_paths, stats, larger_row_first)


# ---- the lexicon of a recogniser's cases ------------------------------------------------------------------------------------
TOP_WORDS = 3


@functools.lru_cache(maxsize=None)
def lexicon(classes):
    """one word list per class count: saturated_lexicon, then (8 classes or more) pairs of twin words under 3 -> 7 and, at 96
    classes, under 3 -> 67"""
    words = saturated_lexicon(classes)
    if classes > 8:
        words += twin_words(np.random.default_rng(32), 6, classes - 1, 3, 7)
    if classes > 68:
        words += [w for w in twin_words(np.random.default_rng(33), 6, classes - 1, 3, 67) if w not in words]
    return tuple(tuple(w) for w in words)


@functools.lru_cache(maxsize=None)
def lexicon_values(name):
    """lexicon_statement.values of a case under its recogniser's lexicon: (V,) float64"""
    from tests import lexicon_statement as ls

    labels, lengths = rows(lexicon(by_name(name)["classes"]))
    return ls.values(log_q(name)[None], labels, lengths)[0]


# The cases whose best words are compared index by index: those the float64 statement alone finds decidable
# (lexicon_statement.top_words_ties: margin above bound(To)) under lexicon(classes).  Values are compared on every case.
# The saturated ones at TOP_WORDS: on the others (a double letter, all blank, the floor) the runners-up are words of equal
# length whose values differ only at floor level, margins of 1e-5 of the bound and less.
LEXICON_TOP = tuple(f"saturated+{boost} {what} C={classes} d={discard}" for boost, what, classes, discard in [
    (30, "word", 37, 2), (30, "one-letter", 37, 2), (30, "full-width", 37, 2), (8, "word", 37, 2), (8, "full-width", 37, 2),
    (30, "word", 37, 0), (30, "one-letter", 37, 0), (30, "full-width", 37, 0),
    (30, "word", 37, 5), (30, "one-letter", 37, 5), (30, "full-width", 37, 5),
    (30, "word", 64, 2), (30, "word", 65, 2), (30, "one-letter", 65, 2), (30, "word", 96, 2),
    (30, "word", 4, 2), (30, "double", 4, 2), (30, "one-letter", 4, 2), (30, "all-blank", 4, 2), (30, "full-width", 4, 2),
    (8, "word", 4, 2), (8, "full-width", 4, 2)])
# The twins with EVERY word returned (top_words = 64, more than the lexicon holds): each pair of twin words is an exact tie
# that only the rule (the smaller index) orders, and the opposite rule orders the other way.
ALL_WORDS = 64


def lexicon_index_cases():
    """[(case, top_words)]"""
    out = [(by_name(n), TOP_WORDS) for n in LEXICON_TOP]
    out += [(c, ALL_WORDS) for c in cases() if c["family"] == "twins" and c["discard"] <= 5 and c["beam"]]
    return out
