"""Patterns on the CPU ("Patterns: the statement and its status"): the host compiler
(keras_ocr_amd/patterns.py) against ``re.fullmatch``, the float64 statement (tests/pattern_statement.py) against the enumeration
of every alignment, and the frozen (case, pattern) pairs of tests/pattern_cases.py -- each shown decidable by the margin rule,
an exact tie that only the tie rule resolves, or without a fit -- before tests/test_patterns_gpu.py compares them on the GPU."""
import itertools
import re

import numpy as np
import pytest

from keras_ocr_amd import patterns as kp
from tests import charset_statement as chs
from tests import ctc_statement as cs
from tests import decode_cases as dc
from tests import lexicon_statement as ls
from tests import pattern_cases as pc
from tests import pattern_statement as ps

# every construct of the syntax, over three or four characters
SMALL = [
    ("ab1", r"a*"), ("ab1", r"(a|b)+1?"), ("ab1", r"[ab]{2}\d"), ("ab1", r"a{1,3}b{2,}"), ("ab1", r".*"), ("ab1", r"(?:ab|1)*"),
    ("ab1", r"[^a]+"), ("ab1", r"a?b?1?"), ("ab1", r"\d{2}|a.b"), ("ab1", r"[a-b1]*a"), ("ab1", r"(a|b|)(1|)"), ("ab1", r"((a))(?:(b)|1){0,2}"),
    ("a.-1", r"a\.1?"), ("a.-1", r"[.\-]+a"), ("a.-1", r"[a-]\d*"), ("a.-1", r"[^.\d]{2}"), ("a.-1", r".\.."), ("a.-1", r"[]a]*|-{3}"),
    ("a*+1", r"\**a\+"), ("a*+1", r"[*+]{1,2}1{0}a"),
]


def _texts(alphabet, longest):
    for n in range(longest + 1):
        yield from itertools.product(range(len(alphabet)), repeat=n)


@pytest.mark.parametrize("alphabet, regex", [(a, r) for a, r in SMALL if "]a]" not in r], ids=lambda v: v)
def test_compiler_accepts_what_fullmatch_accepts(alphabet, regex):
    pats = kp.Patterns(alphabet, {"p": regex})
    for text in _texts(alphabet, 5):
        want = re.fullmatch(regex, "".join(alphabet[c] for c in text)) is not None
        assert pats.accepts(0, text) == want, (regex, text)
    delta, accept = pats.delta[0], pats.accept[0]
    assert delta.dtype == np.int32 and delta.shape[1] == len(alphabet) and accept.shape == (len(delta),)
    # trimmed and breadth-first: every state is first reached from a smaller one, and some accepting state exists
    seen = 1
    for s in range(len(delta)):
        for t in delta[s]:
            assert t <= seen
            seen += t == seen
    assert seen == len(delta) and accept.any()


def test_tables_are_canonical():
    for alphabet, spellings in [("ab1", [r"(a|b)*", r"[ab]*", r"(a*b*)*", r"(?:[ab]+)?", r"[^1]*"]),
                                ("ab1", [r"aa*", r"a+", r"a{1,}", r"a|aa+"]),
                                ("ab1", [r"\d|a", r"[a1]", r"1|a", r"[^b]"]),
                                (pc.ALPHABETS[37], [r"\d{2}", r"[0-9][0-9]", r"\d\d", r"[0-9]{2,2}"])]:
        tables = [kp.compile_pattern("p", r, alphabet) for r in spellings]
        for d, a in tables[1:]:
            assert np.array_equal(d, tables[0][0]) and np.array_equal(a, tables[0][1]), spellings


def test_typical_patterns_are_small():
    for regex, classes, states, nodes in [(r"\d{2}/\d{2}", 96, 6, 41), (r"[a-z]{2}\d{2}[a-z]{3}", 37, 8, 150), (r"[a-z0-9]*", 37, 1, 36),
                                          (r".{0,40}", 96, 41, 3800), (r".{11}", 37, 12, 396)]:
        d, _ = kp.compile_pattern("p", regex, pc.ALPHABETS[classes])
        assert (len(d), kp.label_nodes(d)) == (states, nodes), regex


REFUSED = [
    (r"^a", r"pattern 'p': the anchor '\^' is not supported.*position 0"), (r"a$", r"anchor '\$'.*position 1"),
    (r"(a)\1", r"escape \\1 is not supported.*position 3"), (r"a\b", r"escape \\b.*position 1"), (r"\w+", r"escape \\w.*position 0"),
    (r"(?=a)b", r"group extension other than \(\?: \).*position 0"), (r"(?i)a", r"group extension.*position 0"),
    (r"(?P<x>a)", r"group extension"), (r"a*?", r"quantifier behind a quantifier.*position 2"), (r"a++", r"quantifier behind a quantifier"),
    (r"a{2}?", r"quantifier behind a quantifier"), (r"*a", r"nothing to repeat at position 0"), (r"a|+", r"nothing to repeat at position 2"),
    (r"(a", r"'\(' that is never closed at position 0"), (r"a)", r"unbalanced '\)' at position 1"), (r"[ab", r"'\[' that is never closed"),
    (r"a{,2}", r"'\{' that does not open"), (r"a{2,1}", r"n < m"), (r"a{5000}", r"repetition count above 4096"), (r"[b-a]", r"bad character range b-a"),
    (r"a\\", None), ("a\\", r"backslash at the end at position 1"),
]


@pytest.mark.parametrize("regex, message", REFUSED, ids=[r for r, _ in REFUSED])
def test_refusals_name_the_pattern_and_the_position(regex, message):
    if message is None:  # an escaped backslash is a literal the alphabet cannot spell
        message = r"cannot spell the character '\\\\'"
    with pytest.raises(ValueError, match=message):
        kp.Patterns("ab1", {"p": regex})


def test_refusals_of_the_alphabet_the_caps_and_the_mapping():
    with pytest.raises(ValueError, match=r"pattern 'date': the alphabet cannot spell the character '/' \(position 5"):
        kp.Patterns(pc.ALPHABETS[37], {"date": r"\d{2}/\d{2}"})
    with pytest.raises(ValueError, match="cannot spell the character 'A'"):
        kp.Patterns(pc.ALPHABETS[37], {"p": r"[A]b"})
    assert kp.Patterns(pc.ALPHABETS[37], {"p": r"Ab"}, lowercase=True).accepts(0, [10, 11])
    with pytest.raises(ValueError, match="pattern 'none' matches no text over the alphabet: its language is empty"):
        kp.Patterns("ab1", {"none": r"[^ab1]"})
    with pytest.raises(ValueError, match="language is empty"):
        kp.Patterns("ab1", {"none": r"a[^ab1]b|[^ab1]+"})
    # the caps, from both sides
    assert len(kp.compile_pattern("p", r"a{255}", "ab1")[0]) == kp.MAX_STATES == 256
    with pytest.raises(ValueError, match=r"pattern 'p' has 257 states: at most 256"):
        kp.compile_pattern("p", r"a{256}", "ab1")
    wide = "".join(chr(0x100 + i) for i in range(128))
    assert kp.label_nodes(kp.compile_pattern("p", r".{32}", wide)[0]) == kp.MAX_NODES == 4096
    with pytest.raises(ValueError, match=r"pattern 'p' has 4224 label nodes: at most 4096"):
        kp.compile_pattern("p", r".{33}", wide)
    assert len(kp.Patterns("ab1", {str(i): "a" for i in range(64)})) == kp.MAX_PATTERNS == 64
    with pytest.raises(ValueError, match="65 patterns: there must be between 1 and 64"):
        kp.Patterns("ab1", {str(i): "a" for i in range(65)})
    with pytest.raises(ValueError, match="0 patterns"):
        kp.Patterns("ab1", {})
    with pytest.raises(ValueError, match="mapping name -> regular expression"):
        kp.Patterns("ab1", [r"a"])
    with pytest.raises(ValueError, match="names are strings"):
        kp.Patterns("ab1", {1: r"a"})
    with pytest.raises(ValueError, match="must be a string"):
        kp.Patterns("ab1", {"p": 7})
    names = ["date", "amount"]
    assert kp.index_of(names, "amount") == 1 and kp.index_of(names, None) is None
    with pytest.raises(ValueError, match=r"unknown pattern 'iban'.*date"):
        kp.index_of(names, "iban")
    uniform, flat = kp.per_box(names, [["date", None], "amount", []], [np.zeros((2, 4, 2)), np.zeros((3, 4, 2)), []])
    assert uniform is None and flat.tolist() == [0, -1, 1, 1, 1]
    assert kp.per_box(names, "date", [[]]) == (0, None)
    with pytest.raises(ValueError, match="image 0 has 1 entries for 2 boxes"):
        kp.per_box(names, [["date"]], [np.zeros((2, 4, 2))])
    tables = kp.Patterns("ab1", {"x": r"a*", "y": r"ab"}).tables()
    assert tables[0].shape == (4, 3) and tables[1].tolist() == [1, 0, 0, 1] and tables[2].tolist() == [1, 3]


# ---- the statement -----------------------------------------------------------------------------------------------------------

def _soft(rng, frames, classes=4):
    return cs.log_q(dc.softmax(rng.normal(0, 2, (frames, classes)))[None])[0]


ENUMERATED = [r"a*", r"(a|b)+1?", r"[ab]{2}\d", r".*", r"a?b?1?", r"aa", r"(ab)*", r"[^a]+|a"]


@pytest.mark.parametrize("regex", ENUMERATED)
def test_statement_equals_the_enumeration(regex):
    """all 4^T alignments (T <= 5) whose collapse re.fullmatch accepts: the best value, a text that reaches it, and the best
    value of the other texts, to 1e-12"""
    alphabet = "ab1"
    dfa = kp.compile_pattern("p", regex, alphabet)
    rng = np.random.default_rng(len(regex))
    for trial in range(20):
        frames = 1 + trial % 5
        lq = _soft(rng, frames)
        best, total = {}, {}
        for path in itertools.product(range(4), repeat=frames):
            text = tuple(cs.collapse(path, 3))
            if re.fullmatch(regex, "".join(alphabet[c] for c in text)) is not None:
                v = sum(lq[t, c] for t, c in enumerate(path))
                best[text] = max(best.get(text, -np.inf), v)
                total[text] = total.get(text, 0.0) + np.exp(v)
        value, labels = ps.viterbi(lq, *dfa)
        if not best:
            assert (value, labels) == (-np.inf, None)
            continue
        assert abs(value - max(best.values())) < 1e-12 and abs(best[tuple(labels)] - value) < 1e-12
        others = [v for text, v in best.items() if text != tuple(labels)]
        assert abs(ps.runner_up(lq, dfa, labels) - max(others)) < 1e-12 if others else ps.runner_up(lq, dfa, labels) == -np.inf
        opposite, _ = ps.viterbi(lq, *dfa, last=True)
        assert opposite == value
        assert abs(ps.log_prob(lq, labels) - np.log(total[tuple(labels)])) < 1e-9  # every alignment of that text


def _text(row):
    return [int(c) for c in row if c >= 0]


def test_statement_reduces_to_the_decodes_it_generalises():
    case = dc.by_name(pc.SOFT)
    lg, lq = dc.decoded(case), dc.log_q(pc.SOFT)
    alphabet = pc.ALPHABETS[37]
    greedy = _text(dc.greedy(lg))
    # .* is the greedy decode; [set]* the greedy decode under that set; a pattern the greedy text matches returns it
    assert ps.viterbi(lq, *kp.compile_pattern("p", r".*", alphabet))[1] == greedy
    for regex, allowed in [(r"\d*", range(10)), (r"[a-z]*", range(10, 36)), (r"[a-f0-3]*", list(range(4)) + list(range(10, 16)))]:
        want = _text(chs.greedy(lg, allowed))
        assert ps.viterbi(lq, *kp.compile_pattern("p", regex, alphabet))[1] == want, regex
    text = "".join(alphabet[c] for c in greedy)
    shape = "".join(r"\d" if ch.isdigit() else "[a-z]" for ch in text)
    for regex in (shape, re.escape(text[:3]) + ".*", ".{%d}" % len(greedy)):
        value, labels = ps.viterbi(lq, *kp.compile_pattern("p", regex, alphabet))
        assert labels == greedy and value == ps.viterbi(lq, *kp.compile_pattern("p", r".*", alphabet))[0], regex
    # a literal word returns that word, log_prob == lexicon_statement.values
    for word in ("h44n9u1cz8l3", "word", "a"):
        row = [alphabet.index(ch) for ch in word]
        value, labels = ps.viterbi(lq, *kp.compile_pattern("p", word, alphabet))
        assert labels == row
        want = ls.values(lq[None], np.array([row], np.int32), np.array([len(row)], np.int32))[0, 0]
        assert abs(ps.log_prob(lq, labels) - want) < 1e-9 and value <= ps.log_prob(lq, labels) + 1e-12


def test_statement_without_a_fit_and_with_the_empty_text():
    rng = np.random.default_rng(5)
    aa = kp.compile_pattern("p", r"aa", "ab1")
    assert ps.viterbi(_soft(rng, 2), *aa) == (-np.inf, None)  # a, blank, a needs three frames
    assert ps.viterbi(_soft(rng, 3), *aa)[1] == [0, 0]
    assert ps.margin(_soft(rng, 2), aa) == (-np.inf, None, None) and not ps.decidable(_soft(rng, 2), aa)
    blank = dc.by_name(pc.BLANK.format(37, 2))
    lq = dc.log_q(blank["name"])
    for regex in (r"(\d{4})?", r".*", r"a*|b"):
        value, labels = ps.viterbi(lq, *kp.compile_pattern("p", regex, pc.ALPHABETS[37]))
        assert labels == [] and abs(value - lq[:, -1].sum()) < 1e-12
        assert abs(ps.log_prob(lq, []) - value) < 1e-12  # the empty text has one alignment


# ---- the frozen pairs ----------------------------------------------------------------------------------------------------------

def test_pairs_cover_what_the_kernel_can_get_wrong():
    assert {(p["case"]["classes"], p["case"]["discard"]) for p in pc.pairs()} == set(pc.CONFIGS)
    sizes = {}
    for classes in (37, 96):
        pats = pc.compiled(classes)
        for name, d in zip(pats.names, pats.delta):
            sizes[(classes, name)] = (len(d), len(d) + kp.label_nodes(d))
    used = {sizes[(p["case"]["classes"], p["pattern"])] for p in pc.pairs()}
    assert any(s == 1 for s, _ in used) and any(6 <= s <= 13 for s, _ in used)
    assert any(n < 256 for _, n in used) and any(256 < n < 1024 for _, n in used)  # across the workgroup's lanes
    assert sizes[(96, "upto40")] == (41, 3841) and sizes[(96, "upto40")] in used
    assert 2 * 48 * 3841 > 64 * 1024  # its back-pointers cannot lie in LDS
    kinds = [p["kind"] for p in pc.pairs()]
    assert kinds.count("tie") >= 6 and kinds.count("nofit") >= 1 and kinds.count("margin") >= 15


@pytest.mark.parametrize("name", [p["name"] for p in pc.pairs()])
def test_every_pair_is_decidable_a_tie_or_without_a_fit(name):
    p = pc.by_name(name)
    frames = dc.T - p["case"]["discard"]
    value, labels = pc.decode(name)
    if p["kind"] == "nofit":
        assert (value, labels) == (-np.inf, None)
        return
    assert labels is not None and np.isfinite(value)
    pats = pc.compiled(p["case"]["classes"])
    assert pats.accepts(pats.names.index(p["pattern"]), labels)
    assert re.fullmatch(pc.PATTERNS[p["case"]["classes"]][p["pattern"]], "".join(pats.alphabet[c] for c in labels))
    if p["kind"] == "margin":
        assert pc.margin(name) > ps.bound(frames, value), (name, pc.margin(name), ps.bound(frames, value))
        assert pc.decode(name, True)[1] == labels
    else:
        other_value, other = pc.decode(name, True)
        assert other_value == value and other != labels, name
        lq = dc.log_q(p["case"]["name"])
        gap = value - ps.next_value(lq, *pc.dfa(p["case"]["classes"], p["pattern"]))
        assert gap > ps.bound(frames, value), (name, gap)


def test_saturated_crops_are_decidable_only_under_patterns_their_text_satisfies():
    """why the frozen pairs pair them so: a contradicting pattern pushes the choice onto the 1e-7 floor"""
    name = pc.SAT.format(37, 2)
    lq = dc.log_q(name)
    value, labels, margin = ps.margin(lq, pc.dfa(37, "eleven"))
    assert len(labels) == 11 and 0 <= margin < 1e-4 < ps.bound(48, value)
