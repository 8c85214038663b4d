"""The scores statement (tests/scores_statement.py) against brute force and its own invariants; no GPU."""
import numpy as np
import pytest

from tests import ctc_statement as cs
from tests import scores_statement as ss
from tests import synth


def _rows(rng, M, T, C, peaked):
    if peaked:
        y = rng.gamma(0.2, size=(M, T, C)) * 1e-6
        y[np.arange(M)[:, None], np.arange(T)[None, :], rng.integers(0, C, (M, T))] += 1.0
    else:
        y = rng.gamma(0.5, size=(M, T, C))
    return (y / y.sum(-1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("T,C", [(1, 2), (2, 3), (3, 4), (4, 4), (5, 3), (5, 4)])
@pytest.mark.parametrize("peaked", [False, True])
def test_log_word_is_the_brute_force_sum_over_paths(T, C, peaked):
    rng = np.random.default_rng(100 * T + 10 * C + peaked)
    y = _rows(rng, 6, T, C, peaked)
    assert ss.no_ties(y)
    got = ss.log_word(y)
    for m in range(len(y)):
        want = ss.brute_force_log_word(y[m])
        assert abs(got[m] - want) <= 1e-12 * max(1.0, abs(want)), (m, got[m], want)


def test_all_blank_decode_is_the_all_blank_path():
    y = np.full((2, 4, 3), 0.1, np.float32)
    y[..., 2] = 0.8  # the blank wins every frame
    rows, L = ss.greedy_decode(y)
    assert np.all(rows == -1) and np.all(L == 0)
    assert np.allclose(ss.log_word(y), cs.log_q(y)[..., 2].sum(-1), rtol=0, atol=1e-12)
    assert np.all(ss.char_scores(y) == 0)


@pytest.mark.parametrize("peaked", [False, True])
@pytest.mark.parametrize("C", [4, 37, 1000])
def test_log_word_is_at_least_the_greedy_path(peaked, C):
    rng = np.random.default_rng(C + peaked)
    y = _rows(rng, 24, 48, C, peaked)
    lw = ss.log_word(y)
    assert np.all(np.isfinite(lw)) and np.all(lw <= 1e-12)
    assert np.all(lw >= ss.greedy_path_log_prob(y) - 1e-9)


def test_character_scores_by_hand():
    #            a     a     blank  a     b     b
    path = [0, 0, 2, 0, 1, 1]
    peak = [0.5, 0.7, 0.9, 0.6, 0.8, 0.55]
    y = np.zeros((1, 6, 3), np.float32)
    for t, (c, p) in enumerate(zip(path, peak)):
        y[0, t] = (1 - p) / 2
        y[0, t, c] = p
    rows, L = ss.greedy_decode(y)
    assert list(rows[0]) == [0, 0, 1, -1, -1, -1] and L[0] == 3
    assert np.array_equal(ss.char_scores(y)[0], np.array([0.7, 0.6, 0.8, 0, 0, 0], np.float32))
    assert ss.greedy_runs(y[0]) == [(0, 0, 2), (0, 3, 4), (1, 4, 6)]
    assert cs.collapse(path, 2) == [0, 0, 1]


def test_detection_scores_are_the_component_maxima():
    from oracle import postproc

    y = synth.heatmap_batch()
    boxes, debug = postproc.get_boxes(y, return_debug=True)
    scores = ss.detection_scores(y, debug)
    assert [len(s) for s in scores] == [len(b) for b in boxes] and sum(len(s) for s in scores) >= 6
    for img, s in zip(y, scores):
        assert s.dtype == np.float32 and np.all(s >= np.float32(0.7))
        # every score is a value of the text map, and no component's maximum exceeds the map's
        assert np.all(np.isin(s, img[..., 0])) and np.all(s <= img[..., 0].max())
    # a second component-wise restatement: the maximum over the pixels with that label, one component at a time
    from scipy import ndimage
    fg = (y[0, ..., 0] > np.float32(0.4)) | (y[0, ..., 1] > np.float32(0.4))
    lab, _ = ndimage.label(fg, structure=np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]]))
    want = ndimage.maximum(y[0, ..., 0], lab, [d["component"] for d in debug[0]])
    assert np.array_equal(scores[0], np.asarray(want, np.float32))


def test_sharded_pipeline_refuses_scores():
    import keras_ocr_amd

    sharded = keras_ocr_amd.dist.ShardedPipeline(pipeline=None)
    with pytest.raises(NotImplementedError, match="scores"):
        sharded.recognize([np.zeros((8, 8, 3), np.uint8)], return_scores=True)
    with pytest.raises(NotImplementedError, match="scores"):
        sharded.recognize_device(0, 1, 8, 8, return_scores=True)


def test_score_tuple_and_duck_typed_stage_refusal():
    from keras_ocr_amd import scores

    labels = np.array([[3, 4, -1, -1], [-1, -1, -1, -1]])
    out = scores.assemble(labels, np.array([-0.5, -2.0], np.float32), np.array([[.9, .8, 0, 0], [0, 0, 0, 0]], np.float32), [0.75, 0.9])
    assert out[0]._fields == ("detection", "word", "log_word", "characters")
    assert out[0].detection == 0.75 and out[0].log_word == -0.5 and out[0].word == np.exp(-0.5)
    assert out[0].characters.dtype == np.float32 and list(out[0].characters) == [np.float32(.9), np.float32(.8)]
    assert len(out[1].characters) == 0 and isinstance(out[1].word, float)

    class Plain:
        def detect(self, images, **kwargs):
            return []

    with pytest.raises(TypeError, match="detector"):
        scores.need("detector", Plain(), "detect")
