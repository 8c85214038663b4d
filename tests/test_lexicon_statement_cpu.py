"""The lexicon statement (tests/lexicon_statement.py) pinned without a GPU, and the host-side Lexicon class.

The statement's values are pinned by exhaustive enumeration (ctc_statement.brute_force over all C**T alignments), for every
word up to length 3 -- repeats and words without an alignment included."""
import itertools

import numpy as np
import pytest

from tests import ctc_statement as cs
from tests import lexicon_statement as ls


def _rows(rng, T, C, peaked=False):
    y = rng.gamma(0.3 if peaked else 0.7, size=(T, C)) + (1e-9 if peaked else 0.0)
    return y / y.sum(-1, keepdims=True)


def _every_word(C, longest=3):
    words = [w for n in range(1, longest + 1) for w in itertools.product(range(C - 1), repeat=n)]
    labels = np.full((len(words), longest), -1, np.int64)
    for v, w in enumerate(words):
        labels[v, :len(w)] = w
    return words, labels, np.array([len(w) for w in words])


@pytest.mark.parametrize("T, C, seed", [(1, 2, 0), (2, 3, 1), (3, 2, 2), (3, 4, 3), (4, 3, 4), (5, 3, 5), (5, 4, 6), (4, 4, 7)])
def test_values_equal_exhaustive_enumeration(T, C, seed):
    y = _rows(np.random.default_rng(seed), T, C, peaked=seed % 2 == 0)
    words, labels, lengths = _every_word(C)
    value = ls.values(cs.log_q(y[None]), labels, lengths)
    assert value.shape == (1, len(words))
    saw_infeasible = False
    for v, w in enumerate(words):
        want = -cs.brute_force(y, w, T)
        if ls.frames_needed(w) > T:
            saw_infeasible = True
            assert want == -np.inf and value[0, v] == -np.inf, w
        else:
            assert np.isfinite(want) and abs(value[0, v] - want) <= 1e-12, w
    assert saw_infeasible == (T < 5)  # (0, 0, 0) needs five frames
    # the words of every length partition part of the alignments: their probabilities sum to at most one
    assert np.exp(value[0][np.isfinite(value[0])]).sum() <= 1 + 1e-12


def test_frames_needed():
    assert ls.frames_needed([3]) == 1 and ls.frames_needed([3, 3]) == 3 and ls.frames_needed([1, 2, 2, 2, 1]) == 7
    assert ls.frames_needed([5] * 32) == 63  # a 32-letter word of one character does not fit the recogniser's 48 frames


def test_order_ties_tail_and_margin():
    value = np.array([[-3.0, -1.0, -1.0, -np.inf, -2.0],
                      [-np.inf, -np.inf, -5.0, -np.inf, -np.inf],
                      [-100.0, -300.0, -200.0, -400.0, -500.0]])
    index, log_prob, margin = ls.top_words(value, 3)
    assert index.tolist() == [[1, 2, 4], [2, -1, -1], [0, 2, 1]]  # equal values: the smaller index first; -inf never returned
    assert log_prob.tolist() == [[-1.0, -1.0, -2.0], [-5.0, -np.inf, -np.inf], [-100.0, -200.0, -300.0]]
    assert margin[0] == 0.0  # the tie
    assert margin[1] == np.inf  # one finite value followed by -inf: an infinite gap, nothing to resolve
    assert margin[2] == 100.0 / 400.0  # gaps of 100 among ranks 1 .. 4, over |value at rank 4|
    index, log_prob, margin = ls.top_words(value[:1], 7)  # more than V
    assert index.tolist() == [[1, 2, 4, 0, -1, -1, -1]] and margin[0] == 0.0
    one = ls.top_words(np.array([[-2.5]]), 1)
    assert one[0].tolist() == [[0]] and one[2][0] == np.inf


def test_greedy_decode_is_not_ranked_below_a_word_less_probable_than_its_path():
    """value(greedy word) >= log P(the arg-max path), since that path is one of its alignments: so no word whose value is
    below the path's own probability may precede the greedy decode"""
    rng = np.random.default_rng(5)
    T, C = 12, 6
    for trial in range(20):
        y = _rows(rng, T, C, peaked=trial % 2 == 0)
        lq = cs.log_q(y[None])
        greedy = cs.collapse(y.argmax(-1), C - 1)
        if not greedy:
            continue
        path = lq[0, np.arange(T), y.argmax(-1)].sum()
        words = [tuple(greedy)] + [tuple(rng.integers(0, C - 1, rng.integers(1, 7))) for _ in range(60)]
        labels = np.full((len(words), 12), -1, np.int64)
        for v, w in enumerate(words):
            labels[v, :len(w)] = w
        value = ls.values(lq, labels, [len(w) for w in words])
        assert value[0, 0] >= path - 1e-12
        index, _, _ = ls.top_words(value, len(words))
        rank = index[0].tolist().index(0)
        assert all(value[0, v] >= path - 1e-12 for v in index[0, :rank])


# ---- keras_ocr_amd.lexicon: the host side -------------------------------------------------------------------------------------

def test_lexicon_encodes_and_merges_duplicates():
    from keras_ocr_amd import lexicon

    alphabet = "0123456789abcdefghijklmnopqrstuvwxyz"
    lex = lexicon.Lexicon(["Hello", "world", "hello", "a", "WORLD", "z9"], alphabet, lowercase=True)
    assert lex.words == ["hello", "world", "a", "z9"] and len(lex) == 4 and lex.classes == 37
    assert lex.labels.dtype == np.int32 and lex.lengths.dtype == np.int32
    assert lex.labels.shape == (4, 5) and lex.lengths.tolist() == [5, 5, 1, 2]
    assert lex.labels[0].tolist() == [alphabet.index(c) for c in "hello"]
    assert lex.labels[2].tolist() == [10, -1, -1, -1, -1] and lex.labels[3].tolist() == [35, 9, -1, -1, -1]
    # without lower-casing "hello" and "Hello" differ -- and the capital is outside this alphabet
    with pytest.raises(ValueError, match="Hello"):
        lexicon.Lexicon(["hello", "Hello"], alphabet)
    cased = lexicon.Lexicon(["ab", "AB", "ab"], "abAB")
    assert cased.words == ["ab", "AB"] and cased.labels.tolist() == [[0, 1], [2, 3]]
    longest = lexicon.Lexicon(["a" * 32], alphabet)
    assert longest.lengths.tolist() == [32] and lexicon.MAX_WORD == 32
    assert len(lexicon.Lexicon([], alphabet)) == 0


def test_lexicon_refusals_name_the_word():
    from keras_ocr_amd import lexicon

    alphabet = "abc"
    with pytest.raises(ValueError, match="empty"):
        lexicon.Lexicon(["ab", ""], alphabet)
    with pytest.raises(ValueError, match="'abd'.*'d'"):
        lexicon.Lexicon(["ab", "abd"], alphabet)
    with pytest.raises(ValueError, match="a{33}.*33 characters"):
        lexicon.Lexicon(["a" * 33], alphabet)
    with pytest.raises(ValueError, match="not a string"):
        lexicon.Lexicon(["ab", 7], alphabet)
    with pytest.raises(ValueError, match="list of words"):
        lexicon.Lexicon("abc", alphabet)
    assert lexicon.top_arg(1) == 1 and lexicon.top_arg(64) == 64
    for bad in (0, 65, -2):
        with pytest.raises(ValueError, match="lexicon_top"):
            lexicon.top_arg(bad)


def test_python_layer_refuses_without_a_gpu():
    import keras_ocr_amd
    from keras_ocr_amd import pipeline

    assert pipeline.lexicon_of(None) is None and pipeline.lexicon_of({"batch_size": 4}) is None
    assert pipeline.lexicon_of({"lexicon_top": 3, "verbose": 0}) == 3
    with pytest.raises(ValueError, match="lexicon_top"):
        pipeline.lexicon_of({"lexicon_top": 0})
    with pytest.raises(ValueError, match="beam_width"):
        pipeline.lexicon_of({"lexicon_top": 3, "beam_width": 8})
    sharded = keras_ocr_amd.dist.ShardedPipeline(pipeline=None)
    with pytest.raises(NotImplementedError, match="lexicon"):
        sharded.recognize([np.zeros((8, 8, 3), np.uint8)], recognition_kwargs={"lexicon_top": 3})

    class Rec:
        alphabet = "abc"
        lexicon = None

    pipe = pipeline.Pipeline(detector=object(), recognizer=Rec())
    with pytest.raises(ValueError, match="loaded lexicon"):
        pipe.recognize([np.zeros((8, 8, 3), np.uint8)], recognition_kwargs={"lexicon_top": 2})


def test_assemble_turns_lexicon_rows_into_matches():
    from keras_ocr_amd import lexicon as lexicon_module, pipeline

    class Rec:
        alphabet = "abc"
        lexicon = lexicon_module.Lexicon(["ab", "c", "cab"], "abc")

    pipe = pipeline.Pipeline(detector=object(), recognizer=Rec())
    boxes = [np.zeros((2, 4, 2), np.float32), np.zeros((0, 4, 2), np.float32)]
    labels = np.array([[0, 1, -1], [2, -1, -1]], np.int32)
    rows = (np.array([[0, 2], [1, -1]], np.int32), np.array([[-0.5, -1.5], [-0.25, -np.inf]], np.float32))
    out = pipe.assemble(boxes, labels, None, None, rows)
    assert [m for m, _ in out[0]] == [[("ab", -0.5), ("cab", -1.5)], [("c", -0.25)]] and out[1] == []
    assert [t for t, _ in pipe.assemble(boxes, labels)[0]] == ["ab", "c"]
