"""Inputs for the tests across the recogniser's batch edge (tests/test_batch_edge_gpu.py): pure numpy, seeded, no GPU.

The recogniser runs at most BATCH = 1024 crops at once (CRNN_BATCH, csrc/abi.h); every entry point offsets its output pointers
by hand for the batch that starts at crop s.  The statement those tests hold the library to: for crops x[0:M] cut at every
multiple of 1024, f(x) is the concatenation of f(piece) over the pieces, bit for bit, for every output.  That comparison sees
a displaced row only where neighbouring rows differ, so the inputs here are made to differ from crop to crop: `distinct_rows`
and `neighbour_share` are the two conditions the GPU test asserts on its reference."""
import functools

import numpy as np

from tests import synth

BATCH = 1024  # CRNN_BATCH of csrc/abi.h
CROP_SEED = 7000
LEXICON_WORDS = 200
LONGEST_WORD = 8


def pieces(m):
    """[0, m) cut at every multiple of BATCH: a list of (start, stop)"""
    return [(s, min(s + BATCH, m)) for s in range(0, m, BATCH)]


@functools.lru_cache(maxsize=None)
def crops(m, seed=CROP_SEED):
    """m distinct crops (m, 31, 200) float32 in [0, 1], as tests/test_crnn_gpu.py builds its own; crops(a) is the head of
    crops(b) for a <= b.  Shared among the tests and read-only."""
    x = np.zeros((m, 31, 200), np.float32)
    for i in range(m):
        x[i] = synth.text_page(31, 200, 3, seed=seed + i)[..., 0] / np.float32(255)
    x.flags.writeable = False
    return x


def page(h, w, seed):
    """a synth.text_page (h, w, 3) uint8 whose white is replaced by a seeded texture of 4 x 4 blocks: no box of 8 x 8 pixels
    cuts a blank crop, so no two boxes of `boxes` cut the same one"""
    img = synth.text_page(h, w, (h * w) // 1000, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    texture = np.kron(rng.integers(130, 256, (-(-h // 4), -(-w // 4), 3), dtype=np.uint8), np.ones((4, 4, 1), np.uint8))[:h, :w]
    white = (img == 255).all(-1)
    img[white] = texture[white]
    return img


def boxes(counts, h, w, seed=11, longest=200, tallest=40):
    """per image a (n, 4, 2) float32 array of n distinct quads inside an h x w image: axis-aligned rectangles and rectangles
    rotated by up to 0.2 rad in turn, sides from 8 px to `longest` x `tallest` (close to the crop's own 200 x 31, so that a
    crop keeps the page's structure and the recogniser reads something else in every one), every corner inside
    [0, w - 1] x [0, h - 1]"""
    rng = np.random.default_rng(seed)
    groups = []
    for n in counts:
        seen, quads = set(), []
        while len(quads) < n:
            bw, bh = rng.uniform(8, min(longest, w - 2)), rng.uniform(8, min(tallest, h - 2))
            cx, cy = rng.uniform(0, w - 1), rng.uniform(0, h - 1)
            th = rng.uniform(-0.2, 0.2) if len(quads) % 2 else 0.0
            c, s = np.cos(th), np.sin(th)
            q = np.array([(cx + x * c - y * s, cy + x * s + y * c)
                          for x, y in ((-bw / 2, -bh / 2), (bw / 2, -bh / 2), (bw / 2, bh / 2), (-bw / 2, bh / 2))], np.float32)
            if q[:, 0].min() < 0 or q[:, 0].max() > w - 1 or q[:, 1].min() < 0 or q[:, 1].max() > h - 1:
                continue
            if q.tobytes() in seen:
                continue
            seen.add(q.tobytes())
            quads.append(q)
        groups.append(np.asarray(quads, np.float32).reshape(-1, 4, 2))
    return groups


def lexicon(classes, n_words=LEXICON_WORDS, seed=5):
    """n_words distinct words of 1 .. LONGEST_WORD labels in [0, classes - 2]: labels (V, LONGEST_WORD) int32, -1 padded, and
    lengths (V,) int32"""
    rng = np.random.default_rng(seed)
    seen, words = set(), []
    while len(words) < n_words:
        word = tuple(int(c) for c in rng.integers(0, classes - 1, int(rng.integers(1, LONGEST_WORD + 1))))
        if word not in seen:
            seen.add(word)
            words.append(word)
    labels = np.full((n_words, LONGEST_WORD), -1, np.int32)
    for i, word in enumerate(words):
        labels[i, :len(word)] = word
    return labels, np.array([len(word) for word in words], np.int32)


def ctc_inputs(m, lw, classes, seed=8):
    """labels (m, 8) int32 in [0, classes - 2], label lengths (m,) in [1, 8] and input lengths (m,) in [lw // 2, lw]: every
    crop has its own row and lengths, and every row has an alignment (a row of 8 labels needs at most 15 frames)"""
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, classes - 1, (m, 8)).astype(np.int32)
    label_lengths = rng.integers(1, 9, m).astype(np.int32)
    input_lengths = rng.integers(lw // 2, lw + 1, m).astype(np.int32)
    return labels, label_lengths, input_lengths


def _row_bytes(a):
    a = np.ascontiguousarray(a)
    return [row.tobytes() for row in a.reshape(len(a), -1)]


def distinct_rows(a):
    """whether the rows of `a` (first axis) are pairwise different as byte strings"""
    rows = _row_bytes(a)
    return len(set(rows)) == len(rows)


def neighbour_share(a):
    """the share of rows k of `a` that differ, as byte strings, from each of the rows k - 1, k + 1 and k - BATCH that exist"""
    rows = _row_bytes(a)
    m = len(rows)
    good = sum(all(rows[k] != rows[j] for j in (k - 1, k + 1, k - BATCH) if 0 <= j < m) for k in range(m))
    return good / m if m else 1.0
