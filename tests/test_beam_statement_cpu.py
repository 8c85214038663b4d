"""The beam-search statement (tests/beam_statement.py) pinned without a GPU, and the Python layer's argument checks.

TensorFlow's ctc_beam_search_decoder cannot be executed here, so the statement is pinned by exhaustive enumeration: with a
beam wide enough to hold every reachable prefix nothing is ever pruned, and its top paths must be the most probable
labellings of ctc_statement.brute_force's sum over all C**T alignments."""
import numpy as np
import pytest

from tests import beam_statement as bs
from tests import ctc_statement as cs


def _rows(rng, T, C, peaked=False):
    y = rng.gamma(0.3 if peaked else 0.7, size=(T, C)) + (1e-9 if peaked else 0.0)
    return y / y.sum(-1, keepdims=True)


@pytest.mark.parametrize("T, C, seed", [(1, 2, 0), (3, 2, 1), (4, 3, 2), (5, 4, 3), (6, 3, 4), (6, 4, 5), (6, 4, 6)])
def test_wide_beam_equals_exhaustive_enumeration(T, C, seed):
    y = _rows(np.random.default_rng(seed), T, C, peaked=seed % 2 == 0)
    every = bs.all_labellings(y)
    K = min(5, len(every))
    labels, log_prob, margin = bs.beam_search(cs.log_q(y[None])[0], beam_width=len(every), top_paths=K)
    assert [tuple(int(c) for c in row if c >= 0) for row in labels] == [lab for _, lab in every[:K]]
    assert np.abs(log_prob - np.array([v for v, _ in every[:K]])).max() <= 1e-12
    assert (np.diff(log_prob) <= 0).all() and margin >= 0
    # every labelling, not only the best: nothing was pruned
    labels, log_prob, _ = bs.beam_search(cs.log_q(y[None])[0], beam_width=len(every) + 3, top_paths=len(every) + 3)
    assert np.isfinite(log_prob).sum() == len(every) and (labels[len(every):] == -1).all()
    assert abs(np.exp(log_prob[:len(every)]).sum() - 1.0) <= 1e-12  # the labellings partition the alignments


def test_tie_rule_and_padding():
    """two classes with identical columns: equal totals; the smaller class first, a longer row before its own prefix"""
    y = np.array([[0.3, 0.3, 0.4]] * 2)
    labels, log_prob, margin = bs.beam_search(cs.log_q(y[None])[0], beam_width=16, top_paths=16)
    assert margin == 0.0
    rows = [tuple(int(c) for c in r if c >= 0) for r, v in zip(labels, log_prob) if v > -np.inf]
    assert len(rows) == len(set(rows)) == 5  # (), (0), (1), (0, 1), (1, 0); a doubled label needs a blank between: T >= 3
    assert rows.index((0,)) < rows.index((1,)) and rows.index((0, 1)) < rows.index((1, 0))
    assert bs.row_key((3, 5), 4) < bs.row_key((3,), 4) < bs.row_key((4,), 4)
    # fewer prefixes than top_paths: -1 rows with -inf behind
    assert (labels[5:] == -1).all() and (log_prob[5:] == -np.inf).all()


def test_pruning_is_part_of_the_statement():
    """beam_width 1 keeps one extension class and one prefix per frame: not the arg-max collapse, and not the best labelling"""
    rng = np.random.default_rng(11)
    differs = 0
    for _ in range(20):
        y = _rows(rng, 6, 4)
        lq = cs.log_q(y[None])[0]
        narrow = bs.beam_search(lq, 1, 1)
        wide = bs.beam_search(lq, 200, 1)
        assert narrow[1][0] <= wide[1][0] + 1e-12
        differs += not np.array_equal(narrow[0], wide[0])
    assert differs > 0


# Seeds on which the best beam path (B = 8 and 16) is at least as probable as the greedy decode.  This is no theorem for a
# finite beam -- the greedy labelling can be pruned on the way -- so the assertion is kept for seeds where it holds in float64,
# which is what this test checks; every seed of range(24) does.
GREEDY_SEEDS = list(range(24))


@pytest.mark.parametrize("beam_width", [8, 16])
def test_best_path_is_no_worse_than_greedy(beam_width):
    for seed in GREEDY_SEEDS:
        rng = np.random.default_rng(1000 + seed)
        T, C = 24, 12
        y = _rows(rng, T, C, peaked=seed % 3 == 0)
        lq = cs.log_q(y[None])
        greedy = cs.collapse(y.argmax(-1), C - 1)
        row = np.array([greedy + [-1] * (T - len(greedy))])
        g = -cs.ctc_loss_logq(lq, row, [len(greedy)], [T])[0]
        _, log_prob, _ = bs.beam_search(lq[0], beam_width, 1)
        assert log_prob[0] >= g - 1e-12, seed


def test_python_layer_validates_without_a_gpu():
    import keras_ocr_amd
    from keras_ocr_amd import _lib, pipeline

    assert _lib.beam_args(16, 3) == (16, 3) and _lib.beam_args(64) == (64, 1) and _lib.beam_args(1, 1) == (1, 1)
    for beam_width, top_paths, name in [(0, 1, "beam_width"), (65, 1, "beam_width"), (-3, 1, "beam_width"),
                                        (4, 5, "top_paths"), (4, 0, "top_paths")]:
        with pytest.raises(ValueError, match=name):
            _lib.beam_args(beam_width, top_paths)
        with pytest.raises(ValueError, match=name):
            pipeline.beam_of({"beam_width": beam_width, "top_paths": top_paths, "batch_size": 4})
    assert pipeline.beam_of(None) is None and pipeline.beam_of({"batch_size": 4, "verbose": 0}) is None
    assert pipeline.beam_of({"beam_width": 8}) == (8, 1)
    sharded = keras_ocr_amd.dist.ShardedPipeline(pipeline=None)
    with pytest.raises(NotImplementedError, match="beam"):
        sharded.recognize([np.zeros((8, 8, 3), np.uint8)], recognition_kwargs={"beam_width": 8})


def test_assemble_turns_beam_rows_into_alternatives():
    from keras_ocr_amd import pipeline

    class Rec:
        alphabet = "abc"

    pipe = pipeline.Pipeline(detector=object(), recognizer=Rec())
    boxes = [np.zeros((2, 4, 2), np.float32), np.zeros((0, 4, 2), np.float32)]
    labels = np.array([[0, 1, -1], [2, -1, -1]], np.int32)
    beam_labels = np.array([[[0, 1, -1], [0, -1, -1]], [[2, -1, -1], [-1, -1, -1]]], np.int32)
    beam_log_prob = np.array([[-0.5, -1.5], [-0.25, -np.inf]], np.float32)
    out = pipe.assemble(boxes, labels, None, (beam_labels, beam_log_prob))
    assert [alt for alt, _ in out[0]] == [[("ab", -0.5), ("a", -1.5)], [("c", -0.25)]] and out[1] == []
    assert [t for t, _ in pipe.assemble(boxes, labels)[0]] == ["ab", "c"]
