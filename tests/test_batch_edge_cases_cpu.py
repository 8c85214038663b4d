"""The inputs of tests/test_batch_edge_gpu.py (tests/batch_edge_cases.py) are what that test needs them to be: the cut is the
library's, no two crops, boxes or words are equal, the boxes are legal for the warp, and the two conditions it asserts on its
reference see what they are meant to see."""
import numpy as np
import pytest

from tests import batch_edge_cases as bc

CLASSES, LW = 37, 48


@pytest.mark.parametrize("m", [0, 1, 1023, 1024, 1025, 2048, 2049, 2055])
def test_pieces_cover_the_crops_once_cut_at_multiples_of_the_batch(m):
    cut = bc.pieces(m)
    assert [i for a, b in cut for i in range(a, b)] == list(range(m))
    assert all(0 < b - a <= bc.BATCH and a % bc.BATCH == 0 for a, b in cut)
    assert len(cut) == -(-m // bc.BATCH)
    assert all(b % bc.BATCH == 0 for _, b in cut[:-1])


def test_batch_is_the_library_s():
    import os
    import re

    abi = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "keras_ocr_amd", "csrc", "abi.h")
    with open(abi, encoding="utf-8") as f:
        assert int(re.search(r"constexpr int CRNN_BATCH = (\d+);", f.read()).group(1)) == bc.BATCH


def test_no_two_crops_are_equal():
    x = bc.crops(2055)
    assert x.shape == (2055, 31, 200) and x.dtype == np.float32
    assert x.min() >= 0 and x.max() <= 1
    assert bc.distinct_rows(x)
    assert np.array_equal(bc.crops(1025), x[:1025])  # the long call's crops are the short call's, continued
    with pytest.raises(ValueError):
        x[0, 0, 0] = 0  # shared among the tests: read-only


@pytest.mark.parametrize("counts", [(600, 425), (1030, 1025), (0, 3)])
def test_boxes_are_distinct_inside_the_image_and_at_least_8_px_wide_and_high(counts):
    h, w = 64, 256
    groups = bc.boxes(counts, h, w)
    assert [len(g) for g in groups] == list(counts)
    flat = np.concatenate(groups)
    assert flat.dtype == np.float32 and flat.shape == (sum(counts), 4, 2)
    assert bc.distinct_rows(flat)
    assert flat[..., 0].min() >= 0 and flat[..., 0].max() <= w - 1 and flat[..., 1].min() >= 0 and flat[..., 1].max() <= h - 1
    sides = np.linalg.norm(flat - np.roll(flat, -1, axis=1), axis=-1)
    assert sides.min() >= 8 - 1e-3  # float32 corners of a rectangle with sides >= 8
    turned = np.abs(flat[:, 0, 1] - flat[:, 1, 1]) > 1e-3
    assert turned.sum() in (len(flat) // 2, len(flat) // 2 - 1)  # rotated and axis-aligned in turn, per image
    assert np.array_equal(bc.boxes(counts, h, w)[0], groups[0])  # seeded


def test_pages_differ_and_no_8_x_8_window_is_of_one_colour():
    a, b = bc.page(64, 256, 31), bc.page(64, 256, 32)
    assert a.shape == (64, 256, 3) and a.dtype == np.uint8 and not np.array_equal(a, b)
    assert np.array_equal(a, bc.page(64, 256, 31))
    gray = a.astype(np.int32).sum(-1)
    windows = np.lib.stride_tricks.sliding_window_view(gray, (8, 8))
    assert (windows.max((-1, -2)) > windows.min((-1, -2))).all()


def test_lexicon_words_are_legal_and_distinct():
    labels, lengths = bc.lexicon(CLASSES)
    assert labels.shape == (bc.LEXICON_WORDS, bc.LONGEST_WORD) and labels.dtype == np.int32 and lengths.dtype == np.int32
    assert lengths.min() == 1 and lengths.max() == bc.LONGEST_WORD
    words = [tuple(row[:n]) for row, n in zip(labels.tolist(), lengths)]
    assert len(set(words)) == len(words)
    for row, n in zip(labels, lengths):
        assert (row[:n] >= 0).all() and (row[:n] <= CLASSES - 2).all() and (row[n:] == -1).all()


def test_ctc_inputs_differ_from_crop_to_crop_and_have_alignments():
    labels, ll, il = bc.ctc_inputs(1025, LW, CLASSES)
    assert labels.shape == (1025, 8) and ll.shape == il.shape == (1025,)
    assert labels.min() >= 0 and labels.max() <= CLASSES - 2
    assert ll.min() == 1 and ll.max() == 8 and il.min() == LW // 2 and il.max() == LW
    rows = np.concatenate([np.where(np.arange(8) < ll[:, None], labels, -1), ll[:, None], il[:, None]], 1)
    assert bc.neighbour_share(rows) == 1.0
    assert (2 * ll - 1 <= il).all()  # labels plus a blank between any two


def test_the_conditions_on_the_reference_see_repeated_rows():
    a = np.arange(2 * 1030, dtype=np.float32).reshape(1030, 2)
    assert bc.distinct_rows(a) and bc.neighbour_share(a) == 1.0
    b = a.copy()
    b[1029] = b[5]  # 1029 - 1024
    assert not bc.distinct_rows(b) and bc.neighbour_share(b) == 1029 / 1030
    b[7] = b[8]
    assert bc.neighbour_share(b) == 1027 / 1030
    nan = np.full((3, 1), np.nan, np.float32)
    assert not bc.distinct_rows(nan)  # byte strings: equal NaNs are equal rows
    assert not bc.distinct_rows(np.array([0.0, 1.0, 0.0], np.float32))  # a vector's rows are its entries
    assert bc.distinct_rows(np.array([0.0, -0.0], np.float32))
    assert bc.neighbour_share(np.zeros((4, 3), np.int32)) == 0.0
