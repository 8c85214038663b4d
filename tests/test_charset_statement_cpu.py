"""The character-set statement (tests/charset_statement.py; DESIGN.md section 4, "Character sets") by itself, and the frozen
(case, set) pairs of tests/charset_cases.py: that every comparison tests/test_charsets_gpu.py makes on them is decidable.  No
GPU."""
import numpy as np
import pytest

from tests import beam_statement as bs
from tests import charset_cases as cc
from tests import charset_statement as st
from tests import ctc_statement as cs
from tests import decode_cases as dc
from tests import lexicon_statement as ls
from tests import scores_statement as ss

PAIRS = cc.pairs()
ALL = [p for p in PAIRS if p["kind"] == "all"]


def _ids(p):
    return p["name"]


def test_the_frozen_list_covers_what_it_names():
    """both class counts, two discards each; every kind of set; |A| in {1, 3, 10} with E = |A| < B and E = B < |A|"""
    assert {(p["case"]["classes"], p["case"]["discard"]) for p in PAIRS} == set(cc.CONFIGS)
    assert {c for c, _ in cc.CONFIGS} == {37, 96} and all(len({d for c, d in cc.CONFIGS if c == n}) == 2 for n in (37, 96))
    for cfg in cc.CONFIGS:
        kinds = {p["kind"] for p in cc.of_config(*cfg)}
        assert kinds >= {"all", "one", "word", "miss", "twin"} and (cfg[0] != 96 or "high" in kinds)
        sizes = {len(p["set"]) for p in cc.of_config(*cfg)}
        assert sizes >= {1, 3, 10, 16, cfg[0] - 1}
    below = [(len(p["set"]), b) for p in PAIRS for b, _ in p["beam"] if len(p["set"]) < b]
    above = [(len(p["set"]), b) for p in PAIRS for b, _ in p["beam"] if len(p["set"]) > b]
    assert {n for n, _ in below} >= {1, 3, 10} and {n for n, _ in above} >= {10}
    assert {b for p in PAIRS for b, _ in p["beam"]} == {b for b, _ in dc.BEAM_PAIRS}
    for p in PAIRS:
        C, d = p["case"]["classes"], p["case"]["discard"]
        raw = p["case"]["logits"][d:].argmax(-1)
        assert st.check_set(p["set"], C) == list(p["set"])
        if p["kind"] == "high":
            assert min(p["set"]) >= 64
        if p["kind"] == "word":
            assert set(p["case"]["path"]) - {C - 1} <= set(p["set"])
        if p["kind"] == "miss":  # the raw arg-max of every non-blank frame is masked
            assert (raw != C - 1).any() and not set(raw[raw != C - 1].tolist()) & set(p["set"])
        if p["kind"] == "twin":  # ... and here the allowed maximum is an exact tie of 3 and 7 in some frame
            m = st.masked(dc.decoded(p["case"]), p["set"])
            assert ((m[:, 3] == m.max(-1)) & (m[:, 7] == m.max(-1))).any()


@pytest.mark.parametrize("p", ALL, ids=_ids)
def test_all_classes_allowed_is_the_unconstrained_statement(p):
    """exactly: the same float64 numbers, not nearly the same"""
    case, lg = p["case"], dc.decoded(p["case"])
    assert np.array_equal(st.masked(lg, p["set"]), lg) and np.array_equal(st.masked(lg, None), lg)
    assert np.array_equal(st.probs(lg, p["set"]), dc.softmax(lg))
    assert np.array_equal(st.log_q(lg, p["set"]), dc.log_q(case["name"]))
    assert np.array_equal(st.greedy(lg, p["set"]), dc.greedy(lg))
    assert st.log_word(lg, p["set"]) == float(ss.log_word(dc.softmax(lg)[None])[0])
    assert np.array_equal(cc.lexicon_values(p["name"]), dc.lexicon_values(case["name"]))
    for pair in p["beam"]:
        got, want = cc.beam(p["name"], *pair), dc.beam(case["name"], *pair)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


@pytest.mark.parametrize("p", PAIRS, ids=_ids)
def test_labels_lie_in_the_set_and_masked_classes_are_zero(p):
    lg, C = dc.decoded(p["case"]), p["case"]["classes"]
    A = set(p["set"])
    outside = [c for c in range(C - 1) if c not in A]
    assert (st.probs(lg, p["set"])[:, outside] == 0).all()
    assert np.isfinite(st.log_q(lg, p["set"])).all()  # ... but q keeps the floor: summed over all C classes
    row = st.greedy(lg, p["set"])
    assert set(row[row >= 0].tolist()) <= A
    for pair in p["beam"]:
        labels, log_prob, _ = cc.beam(p["name"], *pair)
        assert set(labels[labels >= 0].tolist()) <= A
        assert np.isfinite(log_prob[0])
        # every row's value is the masked crop's CTC log-probability of that row
        n = int(np.isfinite(log_prob).sum())
        lq = st.log_q(lg, p["set"])
        want = -cs.ctc_loss_logq(np.broadcast_to(lq, (n,) + lq.shape), labels[:n], (labels[:n] >= 0).sum(-1), [len(lg)] * n)
        assert np.array_equal(log_prob[:n], want)
    # a word that uses a masked character keeps a finite value: it is not removed
    words = dc.lexicon(C)
    values = cc.lexicon_values(p["name"])
    fits = np.array([ls.frames_needed(w) <= len(lg) for w in words])
    assert np.array_equal(np.isfinite(values), fits)
    if outside:
        assert any(fits[v] and set(w) - A for v, w in enumerate(words))


@pytest.mark.parametrize("allowed", [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)], ids=str)
@pytest.mark.parametrize("name", [c["name"] for c in dc.of_config(4, 47)])
def test_tiny_crops_equal_the_enumeration_restricted_to_the_set(name, allowed):
    """4 classes, 3 frames: the sum over all 4^3 alignments of the masked q.  The word log-probability is the enumeration's value
    of the decode; the beam at width 64 (nothing is pruned) returns exactly the labellings over A, in the enumeration's order"""
    case = dc.by_name(name)
    lg = dc.decoded(case)
    every = bs.all_labellings(st.probs(lg, allowed))
    within = [(v, lab) for v, lab in every if set(lab) <= set(allowed)]
    assert len(within) < len(every) or len(allowed) == 3
    decode = tuple(int(c) for c in st.greedy(lg, allowed) if c >= 0)
    assert st.log_word(lg, allowed) == pytest.approx(dict((lab, v) for v, lab in every)[decode], rel=1e-12, abs=1e-12)
    labels, log_prob, stats = st.beam(lg, allowed, 64, 64)
    rows = [tuple(int(c) for c in r if c >= 0) for r in labels[:len(within)]]
    assert np.allclose(log_prob[:len(within)], [v for v, _ in within], rtol=1e-12, atol=1e-12)
    assert (labels[len(within):] == -1).all() and (log_prob[len(within):] == -np.inf).all()
    if stats["margin"] > 1e-9 and not stats["ties"]:
        assert rows == [lab for _, lab in within]
    else:
        assert sorted(rows) == sorted(lab for _, lab in within)
    assert rows[0] == max(within, key=lambda r: (r[0], [-x for x in bs.row_key(r[1], 3)]))[1] or stats["ties"]


@pytest.mark.parametrize("p", PAIRS, ids=_ids)
def test_every_frozen_pair_is_decidable(p):
    """The condition under which tests/test_charsets_gpu.py compares rows and indices with the statement: the decision margin
    (tie-aware: an exact tie is judged by the tie rule, on both sides) exceeds decode_cases.bound, the bound the unconstrained
    decode tests use; the saturated crops are judged by their lead margin, as there.  Nothing on the GPU is skipped for it."""
    frames = dc.T - p["case"]["discard"]
    for pair in p["beam"]:
        stats = cc.beam(p["name"], *pair)[2]
        print(f"\n{p['name']} {pair}: margin {stats['margin']:.3g}, lead {stats['lead']:.3g}, ties {stats['ties']}; bound {dc.bound(frames):.3g}")
        assert stats["lead" if p["judge"] == "lead" else "margin"] > dc.bound(frames), (p["name"], pair, stats)
    if p["lexicon"]:
        _, _, margin, _ = ls.top_words_ties(cc.lexicon_values(p["name"])[None], dc.TOP_WORDS)
        assert margin[0] > dc.bound(frames), (p["name"], margin)


def test_the_twin_sets_hang_on_the_tie_rule():
    """every `twin` entry meets exact ties in its search, and at some width the opposite rule gives another answer"""
    for p in (q for q in PAIRS if q["kind"] == "twin"):
        assert all(cc.beam(p["name"], *pair)[2]["ties"] > 0 for pair in p["beam"]), p["name"]
        lg = dc.decoded(p["case"])
        assert not np.array_equal(st.greedy(lg, p["set"]), st.greedy(lg, p["set"], last=True)), p["name"]


def test_set_validation():
    with pytest.raises(ValueError, match="at least one"):
        st.check_set([], 37)
    with pytest.raises(ValueError, match="36"):
        st.check_set([36], 37)
    with pytest.raises(ValueError, match="-1"):
        st.check_set([-1, 3], 37)
    assert st.check_set([5, 3, 3], 37) == [3, 5]


def test_python_layer_validates_without_a_gpu():
    import keras_ocr_amd as k
    from keras_ocr_amd import charsets, pipeline

    alphabet = k.recognition.DEFAULT_ALPHABET
    names, allowed = charsets.table({"digits": "0123456789", "hex": "0123456789abcdef"}, alphabet)
    assert names == ["digits", "hex"] and allowed.shape == (2, 36) and allowed.dtype == np.uint8
    assert allowed[0].tolist() == [1] * 10 + [0] * 26 and allowed[1].sum() == 16
    assert np.array_equal(charsets.table({"x": "ABC"}, alphabet, lowercase=True)[1][0], charsets.table({"x": "abc"}, alphabet)[1][0])
    assert np.array_equal(charsets.table({"x": ["a", "b"]}, alphabet)[1][0], charsets.table({"x": "ab"}, alphabet)[1][0])
    with pytest.raises(ValueError, match="'A'.*outside the alphabet"):
        charsets.table({"upper": "ABC"}, alphabet)
    with pytest.raises(ValueError, match="'codes'.*'-'"):
        charsets.table({"digits": "012", "codes": "a-z"}, alphabet)
    with pytest.raises(ValueError, match="'none' is empty"):
        charsets.table({"none": ""}, alphabet)
    with pytest.raises(ValueError, match="257 character sets"):
        charsets.table({str(i): "0" for i in range(257)}, alphabet)
    with pytest.raises(ValueError, match="0 character sets"):
        charsets.table({}, alphabet)
    with pytest.raises(ValueError, match="mapping"):
        charsets.table(["0123"], alphabet)
    assert len(charsets.table({str(i): "0" for i in range(256)}, alphabet)[0]) == 256
    assert charsets.index_of(names, None) is None and charsets.index_of(names, "hex") == 1
    with pytest.raises(ValueError, match=r"unknown character set 'letters'.*\['digits', 'hex'\]"):
        charsets.index_of(names, "letters")
    with pytest.raises(ValueError, match=r"unknown character set 'digits'.*\[\]"):
        charsets.index_of(None, "digits")
    boxes = [np.zeros((2, 4, 2)), np.zeros((0, 4, 2)), np.zeros((1, 4, 2))]
    assert charsets.per_box(names, "hex", boxes) == (1, None)
    assert charsets.per_box(names, None, boxes) == (None, None)
    uniform, flat = charsets.per_box(names, [["digits", None], [], ["hex"]], boxes)
    assert uniform is None and flat.dtype == np.int32 and flat.tolist() == [0, -1, 1]
    assert charsets.per_box(names, ["digits", None, "hex"], boxes)[1].tolist() == [0, 0, 1]
    with pytest.raises(ValueError, match="2 per-image lists for 3"):
        charsets.per_box(names, [["digits", None], []], boxes)
    with pytest.raises(ValueError, match="image 0 has 1 entries for 2 boxes"):
        charsets.per_box(names, [["digits"], [], ["hex"]], boxes)
    with pytest.raises(ValueError, match="unknown character set 'nope'"):
        charsets.per_box(names, [["digits", "nope"], [], ["hex"]], boxes)

    # a recogniser without a loaded table refuses charset= before anything runs; so does the pipeline
    rec = k.recognition.Recognizer.__new__(k.recognition.Recognizer)
    rec.alphabet, rec.charsets, rec.lexicon, rec._ctx = alphabet, None, None, None  # pylint: disable=protected-access
    with pytest.raises(ValueError, match="set_charsets"):
        rec.recognize(np.zeros((31, 200, 3), np.uint8), charset="digits")
    with pytest.raises(ValueError, match="set_charsets"):
        rec.recognize_from_boxes([np.zeros((8, 8, 3), np.uint8)], [np.zeros((1, 4, 2), np.float32)], charset="digits")
    with pytest.raises(ValueError, match="set_charsets"):
        rec.recognize_from_boxes([np.zeros((8, 8, 3), np.uint8)], [np.zeros((1, 4, 2), np.float32)], charset=[["digits"]])

    class Foreign:
        alphabet = "abc"

        def recognize_from_boxes(self, images, box_groups):
            raise AssertionError("refused before it is called")

    class Det:
        def detect(self, images, **kw):
            return [np.zeros((1, 4, 2), np.float32) for _ in images]

    page = [np.zeros((8, 8, 3), np.uint8)]
    pipe = pipeline.Pipeline(detector=Det(), recognizer=Foreign())
    for method in (pipe.recognize, pipe.recognize_with_scores, pipe.recognize_lines, pipe.recognize_raw, pipe.recognize_tiled):
        with pytest.raises(TypeError, match="charset"):
            method(page, recognition_kwargs={"charset": "digits"})
    pipe = pipeline.Pipeline(detector=Det(), recognizer=rec)
    rec._ctx = object()  # pylint: disable=protected-access
    with pytest.raises(ValueError, match="set_charsets"):
        pipe.recognize(page, recognition_kwargs={"charset": "digits"})
    with pytest.raises(ValueError, match="one name for every box"):
        pipe.recognize(page, recognition_kwargs={"charset": ["digits"]})
