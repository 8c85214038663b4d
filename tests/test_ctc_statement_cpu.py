"""The CTC loss statement (tests/ctc_statement.py) against brute-force enumeration and against
torch.nn.functional.ctc_loss, and Recognizer.get_batch_generator's batches (recognition.batch_generator) against the
reference text (recognition.py:406-465).  No GPU."""
import itertools

import numpy as np
import pytest

from tests import ctc_statement as cs


def _dirichlet(rng, shape, alpha=1.0):
    y = rng.gamma(alpha, size=shape)
    return (y / y.sum(-1, keepdims=True)).astype(np.float32)


def test_statement_equals_brute_force_enumeration():
    rng = np.random.default_rng(0)
    n = n_inf = 0
    for T in range(1, 6):
        for C in range(2, 5):
            if C ** T > 1024:
                continue
            y = _dirichlet(rng, (T, C), alpha=0.7)
            labels = []
            for L in range(0, T + 1):
                labels += [list(l) for l in itertools.product(range(C - 1), repeat=L)][:6]
            for lab in labels:
                for Tm in range(max(1, len(lab)), T + 1):
                    want = cs.brute_force(y[:Tm], lab, Tm)
                    row = np.full((1, max(1, T)), -1)
                    row[0, :len(lab)] = lab
                    got = cs.ctc_loss(y[np.newaxis], row, [len(lab)], [Tm])[0]
                    if np.isinf(want):
                        assert np.isinf(got) and got > 0, (T, C, lab, Tm)
                        n_inf += 1
                    else:
                        assert abs(got - want) <= 1e-12 * abs(want) + 1e-300, (T, C, lab, Tm, got, want)
                    n += 1
    assert n > 300 and n_inf > 10


def test_infeasible_repeats_are_inf_and_the_rest_finite():
    y = _dirichlet(np.random.default_rng(1), (1, 4, 3))
    got = cs.ctc_loss(np.repeat(y, 3, 0), [[0, 0, -1], [0, 1, -1], [0, 0, 0]], [2, 2, 3], [2, 2, 4])
    assert np.isinf(got[0]) and np.isfinite(got[1]) and np.isinf(got[2])
    assert np.isfinite(cs.ctc_loss(np.repeat(y, 1, 0), [[0, 0]], [2], [3]))[0]


@pytest.mark.parametrize("C", [37, 1000])
def test_statement_equals_torch_ctc_loss(C):
    import torch

    rng = np.random.default_rng(C)
    M, T = 64, 48
    y = _dirichlet(rng, (M, T, C), alpha=0.3)
    Tm = rng.integers(1, T + 1, M)
    L = np.array([rng.integers(0, t + 1) for t in Tm])
    L[:4] = Tm[:4]  # full-length labels
    labels = np.full((M, T), -1)
    for m in range(M):
        labels[m, :L[m]] = rng.integers(0, min(C - 1, 3 if m % 3 == 0 else C - 1), L[m])  # every third sample: many repeats
    want = cs.ctc_loss(y, labels, L, Tm)
    lq = torch.from_numpy(cs.log_q(y)).permute(1, 0, 2)
    tgt = torch.from_numpy(np.concatenate([labels[m, :L[m]] for m in range(M)]).astype(np.int64))
    ref = torch.nn.functional.ctc_loss(lq, tgt, torch.from_numpy(Tm), torch.from_numpy(L), blank=C - 1, reduction="none",
                                       zero_infinity=False).numpy()
    fin = np.isfinite(ref)
    assert np.array_equal(fin, np.isfinite(want))
    assert fin.sum() > M // 2
    assert np.all(np.abs(want[fin] - ref[fin]) <= 1e-9 * np.maximum(1.0, np.abs(ref[fin])))


# ---- Recognizer.get_batch_generator ---------------------------------------------------------------------------------------
ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyz"


def _samples(sentences, seed=0, weights=False):
    rng = np.random.default_rng(seed)
    for i, s in enumerate(sentences):
        img = rng.integers(0, 256, (31, 200, 3), dtype=np.uint8)
        yield (img, s, float(i) + 0.5) if weights else (img, s)


def test_batch_generator_shapes_labels_and_gray_rule():
    from keras_ocr_amd import recognition
    from oracle import tools as otools

    sentences = ["abc", " hello ", "x1y2", "z" * 48, "a b", "q", "7", "mm", "last"]
    src = list(_samples(sentences))
    gen = recognition.batch_generator(iter(src), ALPHABET + " ", 48, batch_size=4)
    (images, labels, input_length, label_length), y = next(gen)
    assert images.shape == (4, 31, 200, 1) and images.dtype == np.float32
    for i in range(4):
        want = otools.rgb2gray_u8(src[i][0]).astype(np.float32) / 255
        assert np.array_equal(images[i, ..., 0], want)
    assert labels.shape == (4, 48) and labels.dtype.kind == "i"
    strip = [s.strip() for s in sentences[:4]]
    for i, s in enumerate(strip):
        assert list(labels[i, :len(s)]) == [(ALPHABET + " ").index(c) for c in s]
        assert np.all(labels[i, len(s):] == -1)
    assert np.array_equal(label_length, np.array([[len(s)] for s in strip]))
    assert input_length.shape == (4, 1) and np.all(input_length == 48)
    assert y.shape == (4, 1) and np.all(y == 0)
    # the reference's zip(image_generator, range(batch_size)) draws one more sample and drops it
    (images2, labels2, _, label_length2), _ = next(gen)
    assert label_length2[0, 0] == len(sentences[5])
    assert np.array_equal(images2[0, ..., 0], otools.rgb2gray_u8(src[5][0]).astype(np.float32) / 255)


def test_batch_generator_sample_weights():
    from keras_ocr_amd import recognition

    out = next(recognition.batch_generator(_samples(["ab", "cd", "ef"], weights=True), ALPHABET, 48, batch_size=3))
    assert len(out) == 3
    assert np.array_equal(out[2], [0.5, 1.5, 2.5])


def test_batch_generator_lowercase():
    from keras_ocr_amd import recognition

    (_, labels, _, _), _ = next(recognition.batch_generator(_samples(["AbC"]), ALPHABET, 48, batch_size=1, lowercase=True))
    assert list(labels[0, :3]) == [10, 11, 12]
    with pytest.raises(AssertionError, match="illegal character: A"):
        next(recognition.batch_generator(_samples(["AbC"]), ALPHABET, 48, batch_size=1))


@pytest.mark.parametrize("sentence, match", [
    ("ab#", "illegal character"),
    ("   ", "zero length"),
    ("a" * 49, "longer than this model"),
    ("a  b", "multiple sequential spaces"),
])
def test_batch_generator_assertions(sentence, match):
    from keras_ocr_amd import recognition

    with pytest.raises(AssertionError, match=match):
        next(recognition.batch_generator(_samples(["ok", sentence]), ALPHABET + " ", 48, batch_size=2))


def test_host_label_conversion():
    from keras_ocr_amd import recognition

    labels, il, ll = recognition._ctc_host_inputs(  # pylint: disable=protected-access
        np.array([[1.0, 2.0, np.nan], [3.0, -1.0, -1.0]]), np.array([[5.0], [4.0]]), np.array([[2.0], [1.0]]), 2)
    assert labels.dtype == np.int32 and labels.tolist() == [[1, 2, -1], [3, -1, -1]]
    assert il.tolist() == [5, 4] and ll.tolist() == [2, 1]
    with pytest.raises(ValueError, match="integers"):
        recognition._ctc_host_inputs(np.array([[1.5]]), [[1]], [[1]], 1)  # pylint: disable=protected-access
    with pytest.raises(ValueError, match="integers"):
        recognition._ctc_host_inputs(np.array([[1]]), [[1.5]], [[1]], 1)  # pylint: disable=protected-access
