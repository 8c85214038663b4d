"""The statement of the character boxes (tests/chars_statement.py) on words whose answer is known: constructed from Gaussian
blobs, and hand-made profiles whose samples fall on pixel centres.  No GPU."""
import numpy as np
import pytest

from tests import chars_cases as cc
from tests import chars_statement as cs


def test_constructed_words_give_their_characters():
    """200 words of 1 - 8 blobs, pitch 5 - 12, height 1 - 1.8 pitches, within 0.3 rad: the constructed number of characters
    for every one of them (no word may be left out), every cut strictly between the two neighbouring centres"""
    words = cc.constructed_words()
    assert len(words) == 200 and {n for _, _, n, _ in words} == set(range(1, 9))
    wrong = []
    for k, (text_map, quad, n, pitch) in enumerate(words):
        got = cs.word_chars(text_map, quad)
        if len(got["peaks"]) != n:
            wrong.append((k, n, len(got["peaks"])))
            continue
        assert got["boxes"].shape == (n, 4, 2) and got["scores"].shape == (n,)
        assert (got["scores"] >= np.float32(0.4)).all() and (got["scores"] <= 1).all()
        length = n * pitch + 4.0  # the quad is the word grown by 2 pixels: centre k lies 2 + (k + 0.5) pitch along it
        for j, cut in enumerate(got["bounds"][1:-1]):
            at = cut / got["n_cols"] * length
            assert 2 + (j + 0.5) * pitch < at < 2 + (j + 1.5) * pitch, (k, j, at, pitch)
        for j, peak in enumerate(got["peaks"]):
            assert got["bounds"][j] <= peak < got["bounds"][j + 1]
    assert not wrong, wrong


@pytest.mark.parametrize("case", cc.hand_made(), ids=lambda c: c[0])
def test_hand_made(case):
    _, text_map, quad, rule, bounds, peaks = case
    got = cs.word_chars(text_map, quad, **rule)
    assert got["bounds"] == bounds and got["peaks"] == peaks
    assert len(got["boxes"]) == len(got["scores"]) == len(peaks)
    if got["n_rows"] == 1 and got["n_cols"] == 8:
        # the samples fall on pixel centres: the profile is the map's row, the scores are its float32 values
        x0 = int(quad[0, 0] / 2 + 0.5)
        row = [float(text_map[2, x0 + i]) if 0 <= x0 + i < text_map.shape[1] else 0.0 for i in range(8)]
        assert got["profile"] == row
        assert got["scores"].tolist() == [np.float32(row[p]) for p in peaks]
    # the characters tile the trimmed part of the word: left to right, full height, in detector-input pixels
    for k in range(len(peaks)):
        left, right = quad[0, 0] + 2 * bounds[k], quad[0, 0] + 2 * bounds[k + 1]
        assert got["boxes"][k].tolist() == [[left, quad[0, 1]], [right, quad[0, 1]], [right, quad[3, 1]], [left, quad[3, 1]]]


def test_a_word_wider_than_512_pixels_is_sampled_coarsely():
    text_map, quad, n = cc.wide_word()
    got = cs.word_chars(text_map, quad)
    assert (quad[1, 0] - quad[0, 0]) / 2 > 1000 and got["n_cols"] == cs.MAX_COLS == 512
    assert len(got["peaks"]) == n


def test_a_word_taller_than_32_pixels():
    text_map, quad, n = cc.tall_word()
    got = cs.word_chars(text_map, quad)
    assert (quad[3, 1] - quad[0, 1]) / 2 > 40 and got["n_rows"] == cs.MAX_ROWS == 32
    assert len(got["peaks"]) == n


def test_the_batch_holds_what_its_generator_guarantees():
    heat, pages, inside = cc.batch()
    assert [len(p) for p in pages] == list(cc.BATCH_WORDS) and 0 in cc.BATCH_WORDS and inside >= 15
    counts, quads, scores = cs.char_batch(heat, pages)
    assert counts.sum() >= inside and len(quads) == len(scores) == counts.sum()
    assert counts.max() >= 2
    # some quads reach outside the map
    flat = np.concatenate([p.reshape(-1, 2) for p in pages if len(p)]) / 2
    assert (flat < 0).any() and (flat[:, 0] > heat.shape[2]).any()


def test_the_many_words_batch_holds_what_its_generator_guarantees():
    """1069 words in five blocks of 256: a block without characters between blocks with, ragged counts elsewhere, and one
    word with as many characters as a word can have, in a block with characters before it"""
    heat, pages, fullest = cc.many_words_batch()
    assert [len(p) for p in pages] == list(cc.MANY_WORDS) == [0, 255, 256, 257, 1, 0, 300]
    assert heat.shape[:2] == (7, 48) and heat.shape[2] >= 3 + 512 and heat.dtype == np.float32
    counts, quads, scores = cs.char_batch(heat, pages, **cc.EXACT_RULE)
    assert len(counts) == 1069 and len(quads) == len(scores) == counts.sum()
    # the dead block: words 512 .. 767 are block 2 of a pack kernel that takes 256 words a block
    assert cc.DEAD_WORDS == (512, 768) and (counts[512:768] == 0).all()
    assert counts[:512].sum() > 0 and counts[768:].sum() > 0 and counts[:256].sum() > 0 and counts[256:512].sum() > 0 and counts[1024:].sum() > 0
    dead = np.concatenate(pages[3][1:257]).reshape(-1, 4, 2).astype(np.float64)
    zero_width = (dead[:, 0] == dead[:, 1]).all(axis=1)
    zero_height = (dead[:, 0] == dead[:, 3]).all(axis=1)
    off_the_map = ((dead[..., 0] / 2 < -1).all(axis=1) | (dead[..., 1] / 2 < -1).all(axis=1)) & ~zero_width & ~zero_height
    assert min(zero_width.sum(), zero_height.sum(), off_the_map.sum()) >= 40 and (zero_width | zero_height | off_the_map).all()
    # the two shares, outside the dead block
    live = np.concatenate([counts[:512], counts[768:]])
    assert (live == 0).mean() >= 0.1 and (live >= 3).mean() >= 0.1
    # the fullest word: the first of the last page, so in block 3 behind characters of earlier blocks
    assert fullest == sum(cc.MANY_WORDS[:-1]) == 769 and fullest // 256 == 3 and fullest % 256 > 0
    assert counts[fullest] == 256 == cs.MAX_COLS // 2
    got = cs.word_chars(heat[6, :, :, 0], pages[6][0], **cc.EXACT_RULE)
    assert got["n_cols"] == 512 and got["n_rows"] == 1 and got["profile"] == [float(np.float32(v)) for v in cc.FULLEST_VALUES]
    assert got["peaks"] == list(range(0, 512, 2)) and got["bounds"] == [0] + list(range(1, 511, 2)) + [511]


@pytest.mark.parametrize("rule, name", [
    ({"peak_threshold": 0.0}, "peak_threshold"), ({"peak_threshold": -1.0}, "peak_threshold"),
    ({"peak_threshold": float("inf")}, "peak_threshold"), ({"peak_threshold": float("nan")}, "peak_threshold"),
    ({"valley_ratio": -0.1}, "valley_ratio"), ({"valley_ratio": 1.5}, "valley_ratio"), ({"valley_ratio": float("nan")}, "valley_ratio"),
    ({"extent_threshold": -0.1}, "extent_threshold"), ({"extent_threshold": 0.5}, "extent_threshold"),
    ({"extent_threshold": float("nan")}, "extent_threshold"), ({"peak_threshold": 0.1}, "extent_threshold"),
])
def test_parameters_out_of_range_are_refused(rule, name):
    with pytest.raises(ValueError, match=name):
        cs.check_rule(**rule)
    text_map, quad = cc.exact_word([0.0, 0.3, 0.7, 0.3, 0.0, 0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match=name):
        cs.word_chars(text_map, quad, **rule)


def test_parameters_at_the_ends_of_their_ranges_are_accepted():
    for rule in ({"valley_ratio": 0.0}, {"valley_ratio": 1.0}, {"extent_threshold": 0.0}, {"extent_threshold": 0.4},
                 {"peak_threshold": 1e-300, "extent_threshold": 0.0}):
        assert cs.check_rule(**rule) == tuple(float({**cs.DEFAULTS, **rule}[k]) for k in ("peak_threshold", "valley_ratio", "extent_threshold"))


def test_the_product_states_the_same_defaults():
    from keras_ocr_amd import _lib, layout

    assert _lib.CHAR_RULE_DEFAULTS == cs.DEFAULTS
    assert _lib.char_rule(True) == cs.DEFAULTS and _lib.char_rule(None) is None and _lib.char_rule(False) is None
    assert _lib.char_rule({"valley_ratio": 1}) == {**cs.DEFAULTS, "valley_ratio": 1.0}
    with pytest.raises(TypeError, match="max_gap"):
        _lib.char_rule({"max_gap": 1.0})
    assert layout.Characters._fields == ("boxes", "scores")
