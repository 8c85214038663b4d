"""tests/decode_cases.py judged by the float64 statements alone, without a GPU: every committed beam and lexicon case is
decidable, every tie case meets an exact tie and gives another answer under the opposite rule, and at 4 classes and 3 frames
the search equals the enumeration of all alignments.  This is what keeps tests/test_decode_edges_gpu.py from passing vacuously:
a case that were not decidable could not be held to the statement, and a tie case whose answer did not hang on the rule would
not test it.

The rule of decidability is the one tests/test_beam_gpu.py and tests/test_lexicon_gpu.py apply: margin above 2 * GATE * To,
GATE = 1e-6 (tests/test_ctc_loss_gpu.py), To the frames after the discard -- with the tie-aware margins
(beam_statement.beam_search_ties, lexicon_statement.top_words_ties), in which a gap between two values that compare equal in
float64 is an exact tie and no margin.  Saturated and floor crops are judged by their lead margin and compared in row 0 only:
their lower rows are near-ties of floor-level candidates."""
import numpy as np
import pytest

from tests import beam_statement as bs
from tests import decode_cases as dc
from tests import lexicon_statement as ls

BEAM_CASES = [c for c in dc.cases() if c["beam"]]


def _id(c):
    return c["name"].replace(" ", "_")


def test_the_constructions_are_what_they_say():
    for c in dc.cases():
        lg, d, C = c["logits"], c["discard"], c["classes"]
        assert lg.dtype == np.float32 and lg.shape == (dc.T, C) and not lg.flags.writeable
        if c["path"] is not None:
            assert lg[d:].argmax(-1).tolist() == list(c["path"]), c["name"]
        if c["family"] == "saturated" and d:
            assert (lg[:d].argmax(-1) == 0).all()  # the discarded frames would decode another row
        if c["family"] == "floor":
            srt = np.sort(lg.astype(np.float64), -1)
            gap = srt[:, -1] - srt[:, -2]
            assert (np.round(lg.astype(np.float64) * 1024) == lg.astype(np.float64) * 1024).all()  # on the grid of 2^-10
            for depth, rows in zip((40, 90, 200), (gap[0::3], gap[1::3], gap[2::3])):
                assert (np.abs(rows - depth) <= 2).all()
            assert np.exp(np.float32(-198)) == 0 and 0 < np.exp(np.float32(-88)) < 2.0 ** -126  # exactly 0, and subnormal
        if c["same_as"]:
            shift = lg.astype(np.float64) - dc.by_name(c["same_as"])["logits"].astype(np.float64)
            assert set(np.unique(shift)) == {-1e4, 0.0, 1e4} and (shift == shift[:, :1]).all()  # exact, whole frames
            assert (shift[d:] != 0).any() and (shift[:d] != 0).any()
    full = dc.by_name("saturated+30 full-width C=37 d=0")
    row = dc.greedy(full["logits"])
    assert (row >= 0).all() and len(row) == 50 and 2 * len(row) + 1 > 64  # no -1 in the label row; more states than lanes
    assert {(c["classes"]) for c in dc.cases()} == {37, 64, 65, 96, 4} and {c["discard"] for c in dc.cases()} >= {0, 2, 5, 47}
    for copies, classes in ((dc.THREE, 37), (dc.FOUR, 96)):
        lg = dc.twins(classes, 1, 3, copies)
        assert all(np.array_equal(lg[:, a].view(np.uint32), lg[:, b].view(np.uint32)) for a, b in copies)
    assert 3 % 64 == 67 % 64 and len({3 % 64, 7 % 64, 20 % 64}) == 3  # the same lane; different lanes


@pytest.mark.parametrize("case", BEAM_CASES, ids=_id)
def test_beam_cases_are_decidable(case):
    frames = dc.T - case["discard"]
    for beam_width, top_paths in case["beam"]:
        labels, log_prob, stats = dc.beam(case["name"], beam_width, top_paths)
        what = f"{case['name']} B={beam_width} K={top_paths}: {stats}"
        assert np.isfinite(log_prob[0]), what
        if case["judge"] == "lead":
            assert stats["lead"] > dc.bound(frames), what
            assert np.array_equal(labels[0], dc.greedy(dc.decoded(case))), what  # a peaked crop's best reading is its arg-max path
        else:
            assert stats["margin"] > dc.bound(frames), what
        if case["ties"]:
            assert stats["ties"] > 0, what
        if case["same_as"]:
            assert np.array_equal(labels[0], dc.beam(case["same_as"], beam_width, top_paths)[0][0])


def test_saturated_lower_rows_are_not_decidable():
    """why the saturated crops are held to row 0: at top_paths 3 their full margin is far below the bound"""
    worst = max(dc.beam(c["name"], 4, 3)[2]["margin"] / dc.bound(dc.T - c["discard"])
                for c in dc.of_config(37, 2, "saturated") if "+30" in c["name"])
    assert worst < 1e-3


def _flips(case):
    """which opposite rules change a tie case's answer"""
    hit = set()
    lg = dc.decoded(case)
    if not np.array_equal(dc.greedy(lg), dc.greedy(lg, last=True)):
        hit.add("greedy")
    for beam_width, top_paths in case["beam"]:
        rows = dc.beam(case["name"], beam_width, top_paths)[0]
        if not np.array_equal(rows, dc.beam(case["name"], beam_width, top_paths, True, False)[0]):
            hit.add("class")
        if not np.array_equal(rows, dc.beam(case["name"], beam_width, top_paths, False, True)[0]):
            hit.add("row")
    return hit


def test_every_tie_case_hangs_on_its_rule():
    """the opposite rule -- the larger class first in the pruning, the larger row first in the beam, the larger index first in
    the lexicon, the last arg-max in the greedy decode -- gives another answer on every tie case, and each direction is hit"""
    seen = set()
    for case in dc.cases():
        if not case["ties"]:
            continue
        hit = _flips(case)
        for beam_width, top_paths in case["beam"]:  # ... at every width it is searched with
            rows = dc.beam(case["name"], beam_width, top_paths)[0]
            other = [dc.beam(case["name"], beam_width, top_paths, *f)[0] for f in ((True, False), (False, True))]
            assert any(not np.array_equal(rows, o) for o in other), (case["name"], beam_width, top_paths)
        assert hit, case["name"]
        seen |= hit
    for case, k in dc.lexicon_index_cases():
        if not case["ties"]:
            continue
        value = dc.lexicon_values(case["name"])[None]
        index, _, _, ties = ls.top_words_ties(value, k)
        assert ties[0] > 0, case["name"]
        assert not np.array_equal(index, ls.top_words_ties(value, k, larger_index_first=True)[0]), case["name"]
        seen.add("index")
    assert seen == {"greedy", "class", "row", "index"}
    straddle = [c for c in dc.cases() if "straddle" in c["name"]]
    assert straddle and all("class" in _flips(c) for c in straddle)
    assert "greedy" in _flips(dc.by_name("twins 36->5 x3 C=37 d=2 seed=100"))


def test_lexicon_cases_are_decidable():
    assert len(dc.lexicon_index_cases()) >= 30
    for case, k in dc.lexicon_index_cases():
        words = dc.lexicon(case["classes"])
        value = dc.lexicon_values(case["name"])[None]
        index, log_prob, margin, ties = ls.top_words_ties(value, k)
        assert margin[0] > dc.bound(dc.T - case["discard"]), (case["name"], margin[0])
        plain = ls.top_words(value, k)
        assert np.array_equal(plain[0], index) and np.array_equal(plain[1], log_prob)  # the variant changes the margin only
        if not ties[0]:
            assert plain[2][0] == margin[0]
        if case["family"] == "saturated" and " word " in case["name"]:
            assert index[0, 0] == 0 and list(words[0]) == [c for c in dc.greedy(dc.decoded(case)) if c >= 0]
        if k > len(words):
            feasible = int(np.isfinite(value).sum())
            assert (index[0, :feasible] >= 0).all() and (index[0, feasible:] == -1).all()


def test_the_lexicons_hold_what_the_issue_lists():
    for classes in (37, 64, 65, 96):
        words = dc.lexicon(classes)
        word = list(words[0])
        assert len(word) == 12 and len(set(words)) == len(words) <= 64
        distance = [sum(a != b for a, b in zip(word, w)) for w in words[1:5]]
        assert distance == [1, 3, 6, 12] and all(len(w) == 12 for w in words[1:5])
        assert min(len(w) for w in words) == 1 and max(len(w) for w in words) == dc.MAX_WORD
        needs = [ls.frames_needed(w) for w in words]
        assert sum(n > 50 for n in needs) == 2 and dc.MAX_WORD in needs  # two cannot fit; a 32-letter word that does
        value = dc.lexicon_values(f"saturated+30 word C={classes} d=2")
        assert np.array_equal(np.isfinite(value), np.array(needs) <= 48)
        lower = -np.sort(-value[:5])
        assert np.array_equal(lower, value[:5]) and value[0] - value[3] > 6 * 10  # six letters off: e^-60 and less
    a, b = dc.lexicon(37)[-2:]
    assert [7 if c == 3 else 3 if c == 7 else c for c in a] == list(b)


def test_tie_aware_margins_on_a_hand_case():
    """two identical columns, two frames (tests/test_beam_statement_cpu.py's tie case): the plain margin is 0, the tie-aware
    one is not, ties are counted, and the opposite row rule turns the order of the twins"""
    from tests import ctc_statement as cs

    lq = cs.log_q(np.array([[[0.3, 0.3, 0.4]] * 2]))[0]
    labels, log_prob, stats = bs.beam_search_ties(lq, 16, 16)
    plain = bs.beam_search(lq, 16, 16)
    assert np.array_equal(labels, plain[0]) and np.array_equal(log_prob, plain[1]) and plain[2] == 0.0 == stats["plain"]
    assert stats["ties"] > 0 and stats["margin"] > 1e-3 and stats["lead"] == 0.0  # (0) and (1) lead together
    rows = [tuple(int(c) for c in r if c >= 0) for r in labels[:5]]
    assert rows.index((0,)) < rows.index((1,)) and rows.index((0, 1)) < rows.index((1, 0))
    other = bs.beam_search_ties(lq, 16, 16, larger_row_first=True)[0]
    rows = [tuple(int(c) for c in r if c >= 0) for r in other[:5]]
    assert rows.index((0,)) > rows.index((1,)) and rows.index((0, 1)) > rows.index((1, 0))
    # beam width 1 keeps one class: the smaller of the twins, under the opposite rule the larger
    assert bs.beam_search_ties(lq[:, [0, 1, 2]], 1, 1)[0][0, 0] in (0, -1)
    y = np.array([[0.45, 0.45, 0.1]] * 2)
    lq = cs.log_q(y[None])[0]
    assert bs.beam_search_ties(lq, 1, 1)[0][0, 0] == 0 and bs.beam_search_ties(lq, 1, 1, larger_class_first=True)[0][0, 0] == 1
    value = np.array([[-1.0, -2.0, -2.0, -2.0 - 1e-13, -9.0]])
    index, _, margin, ties = ls.top_words_ties(value, 2)
    assert index.tolist() == [[0, 1]] and ties[0] == 1 and 0 < margin[0] < 1e-12  # the value just behind the tie counts
    assert ls.top_words_ties(value, 2, larger_index_first=True)[0].tolist() == [[0, 2]]
    assert ls.top_words(value, 2)[2][0] == 0.0


@pytest.mark.parametrize("case", dc.of_config(4, 47), ids=_id)
def test_three_frames_of_four_classes_equal_the_enumeration(case):
    """beam width 64 holds every labelling of 3 frames: rows and values are those of the sum over all 4^3 alignments"""
    every = bs.all_labellings(dc.softmax(dc.decoded(case)))
    assert len(every) <= 64
    labels, log_prob, stats = dc.beam(case["name"], 64, 64)
    rows = [tuple(int(c) for c in r if c >= 0) for r in labels[:len(every)]]
    assert rows == [lab for _, lab in every]
    assert np.abs(log_prob[:len(every)] - np.array([v for v, _ in every])).max() <= 1e-12
    assert (labels[len(every):] == -1).all() and (log_prob[len(every):] == -np.inf).all()
