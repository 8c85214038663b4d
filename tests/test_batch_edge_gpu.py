"""Every recogniser entry point across the 1024-crop batch edge (CRNN_BATCH, csrc/abi.h).

The statement: for an entry point f and crops x[0:M] cut at every multiple of 1024 (tests/batch_edge_cases.pieces), f(x) equals
the concatenation of f(piece) over the pieces BIT FOR BIT, for every output.  Each piece is one batch with s = 0 and the nb of
the corresponding batch of the long call: the same launches, dispatch, cell grid and lexicon chunking on the same data, so
any difference is an addressing or workspace fault of the batch loop (api.cpp, RecStage::run in abi.h) and no tolerance
applies.  A tail piece is never compared with the same crops inside a larger batch: other kernels run there.  M = 1025 leaves
a tail of one crop (the 8-wide cell grid, conv_mfma for the 1x1 layers) behind a full batch on the same workspace; M = 2055
makes three batches, s = 2048 and a tail of 7.

The piece calls are the library's own, on paths that tests/test_crnn_gpu.py, test_crnn_layers_gpu.py, test_beam_gpu.py,
test_lexicon_gpu.py, test_scores_gpu.py and test_ctc_loss_gpu.py tie to independent references at M <= 1024; one anchor is
direct: the first 8 crops' probabilities of the M = 2055 call against oracle.crnn within test_crnn_gpu.PROB_TOL.

A displaced row shows only where rows differ.  So the REFERENCE (the concatenated pieces) of every comparison must have M
pairwise different rows, as byte strings, in every float output, and in every integer output the row of crop k must differ
from those of crops k - 1, k + 1 and k - 1024 for at least half of the crops (`_conditions`).  That is a condition on the
inputs of tests/batch_edge_cases.py, not on the library.  Measured shares (pytest -s prints them):
  crops of batch_edge_cases.crops, M = 1025: every float output (probs, log_word, char_scores, beam log_prob, lexicon log_prob
    and values, loss, feats) 1025 of 1025 rows different; labels 1.000, beam labels 1.000, lexicon index 0.975;
  the same, M = 2055: 2055 of 2055; labels 0.996;
  crops warped from batch_edge_cases.boxes, counts (600, 425): floats 1025 of 1025; labels 0.870, beam labels 0.992, lexicon
    index 0.684; counts (1030, 1025): floats 2055 of 2055; labels 0.868, beam labels 0.992, lexicon index 0.655.
On the CPU, oracle.crnn on crops(2055) alone gives labels 0.996 and no empty decode (an empty decode's char_scores row is all
zero, so two of them would be equal rows).
"""
import ctypes

import numpy as np
import pytest

from tests import batch_edge_cases as bc
from tests.test_crnn_gpu import PROB_TOL

pytestmark = pytest.mark.gpu

BEAM = (4, 2)
TOP_WORDS = 3
PAGE_H, PAGE_W = 64, 256


@pytest.fixture(scope="module")
def rec(ctx, crnn_weights):
    """the default build with the lexicon of batch_edge_cases loaded; every switch off again afterwards"""
    ctx.crnn_set_rnn_steps_to_discard(2)
    ctx.load_crnn(crnn_weights)
    assert ctx.crnn_classes() == 37 and ctx.crnn_label_width() == 48
    ctx.set_lexicon(*bc.lexicon(ctx.crnn_classes()))
    assert ctx.lexicon_size() == bc.LEXICON_WORDS
    yield ctx
    _switches_off(ctx)
    ctx.set_lexicon_scratch(0)
    ctx.set_lexicon(None)


def _switches_off(c):
    c.set_scores(False)
    c.set_beam(0)
    c.set_lexicon_match(0)
    assert (c.get_scores(), c.get_beam(), c.get_lexicon_match()) == (False, (0, 1), 0)


def _tuple(out):
    return out if isinstance(out, tuple) else (out,)


def _bits(a):
    """floats through their bit patterns, so that -inf rows and NaNs count"""
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_same(got, want, what, names):
    got, want = _tuple(got), _tuple(want)
    assert len(got) == len(want) == len(names), what
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name}: {g.dtype} {g.shape} for {w.dtype} {w.shape}"
        assert g.dtype in (np.float32, np.int32), f"{what}: {name}"
        if not np.array_equal(_bits(g), _bits(w)):
            m = len(w)
            rows = np.flatnonzero((_bits(g).reshape(m, -1) != _bits(w).reshape(m, -1)).any(1))
            raise AssertionError(f"{what}: {name}: {len(rows)} of {m} rows differ from the pieces', the first at crop {rows[0]}, the last at crop {rows[-1]}")


def _conditions(want, what, names):
    """the comparison can see a displaced row: the condition of the module docstring on the reference"""
    for w, name in zip(_tuple(want), names):
        if w.dtype == np.float32:
            distinct = len({row.tobytes() for row in w.reshape(len(w), -1)})
            print(f"\n{what}: {name}: {distinct} of {len(w)} rows pairwise different")
            assert bc.distinct_rows(w), f"{what}: {name}: only {distinct} different rows among {len(w)}: choose other inputs"
        else:
            share = bc.neighbour_share(w)
            print(f"\n{what}: {name}: {share:.3f} of the rows differ from rows k - 1, k + 1 and k - 1024")
            assert share >= 0.5, f"{what}: {name}: choose other inputs"


def _by_pieces(call, m, *per_crop):
    """call(x[a:b] for x in per_crop) on every piece, the outputs concatenated"""
    parts = [_tuple(call(*[x[a:b] for x in per_crop])) for a, b in bc.pieces(m)]
    return tuple(np.concatenate(column) for column in zip(*parts))


def _check(call, m, names, what, *more):
    x = bc.crops(m)
    got = call(x, *more)
    want = _by_pieces(call, m, x, *more)
    what = f"{what} M={m}"
    _conditions(want, what, names)
    _assert_same(got, want, what, names)
    return _tuple(got)


@pytest.mark.parametrize("m", [1025, 2055])
def test_forward_with_probs(rec, crnn_weights, m):
    labels, probs = _check(lambda x: rec.crnn_forward(x, return_probs=True), m, ("labels", "probs"), "crnn_forward(return_probs=True)")
    assert probs.shape == (m, 48, 37)
    if m == 2055:
        # the anchor: crops 0 .. 7 lie in a first batch of 1024 crops, the conv_ds configuration that
        # tests/test_crnn_gpu.py::test_probs_and_labels_match_oracle holds to the oracle at m = 40
        from oracle import crnn as ocrnn

        want = ocrnn.crnn_forward(crnn_weights, np.array(bc.crops(8))[..., None])
        err = float(np.abs(probs[:8] - want).max())
        print(f"\ncrops 0 .. 7 of M=2055: max abs prob error {err:.2e} against the oracle")
        assert err <= PROB_TOL, f"max abs prob error {err}"


def test_forward_labels_only(rec):
    _check(rec.crnn_forward, 1025, ("labels",), "crnn_forward(return_probs=False)")


@pytest.mark.parametrize("m", [1025, 2055])
def test_forward_scores(rec, m):
    _check(lambda x: rec.crnn_forward_scores(x, return_probs=True), m, ("labels", "log_word", "char_scores", "probs"),
           "crnn_forward_scores(return_probs=True)")


def test_beam(rec):
    labels, log_prob = _check(lambda x: rec.crnn_beam(x, *BEAM), 1025, ("labels", "log_prob"), f"crnn_beam{BEAM}")
    assert labels.shape == (1025, BEAM[1], 48) and log_prob.shape == (1025, BEAM[1])


@pytest.mark.parametrize("chunk", [0, 3], ids=["default_scratch", "chunks_of_3"])
def test_lexicon(rec, chunk):
    """chunks of 3 crops: the chunk loop (lexicon_run) inside the batch loop, 342 chunks in the first batch and one of 1 crop
    in the second"""
    v = rec.lexicon_size()
    try:
        rec.set_lexicon_scratch(chunk * 4 * v + 8 if chunk else 0)
        index, log_prob, values = _check(lambda x: rec.crnn_lexicon(x, TOP_WORDS, return_values=True), 1025,
                                         ("index", "log_prob", "values"), f"crnn_lexicon(top_words={TOP_WORDS}), chunk {chunk}")
    finally:
        rec.set_lexicon_scratch(0)
    assert index.shape == log_prob.shape == (1025, TOP_WORDS) and values.shape == (1025, v)
    assert index.min() >= 0 and np.isfinite(values).all()  # every word of 1 .. 8 labels has an alignment in 48 frames


def test_ctc_loss(rec):
    """a label row or a length taken from another crop changes the loss"""
    m = 1025
    per_crop = bc.ctc_inputs(m, rec.crnn_label_width(), rec.crnn_classes())
    (loss,) = _check(rec.crnn_ctc_loss, m, ("loss",), "crnn_ctc_loss", *per_crop)
    assert np.isfinite(loss).all()
    # the label rows matter: crop k with the row and lengths of crop k - 1 gives another loss, the tail crop's included
    rolled = rec.crnn_ctc_loss(bc.crops(m)[-3:], *[a[-4:-1] for a in per_crop])
    assert (rolled != loss[-3:]).all()


def test_features(rec):
    (feats,) = _check(rec.crnn_features, 1025, ("feats",), "crnn_features")
    assert feats.shape == (1025, 50, 256)


# ---- RecStage: kocr_recognize_boxes with every switch on --------------------------------------------------------------
STAGE_NAMES = ("labels", "log_word", "char_scores", "beam labels", "beam log_prob", "lexicon index", "lexicon log_prob")


def _pages():
    return np.stack([bc.page(PAGE_H, PAGE_W, 31), bc.page(PAGE_H, PAGE_W, 32)])


def _switches_on(c):
    c.set_scores(True)
    c.set_beam(*BEAM)
    c.set_lexicon_match(TOP_WORDS)


_STAGE_REFERENCE = {}


def _stage_reference(c, counts):
    """what tests/test_lexicon_gpu.py::test_pipeline_equals_the_stages composes at small M: the crops of the context's warp
    entry point on the same boxes, then crnn_forward_scores, crnn_beam and crnn_lexicon on the pieces.  Computed once."""
    if counts not in _STAGE_REFERENCE:
        groups = bc.boxes(counts, PAGE_H, PAGE_W)
        crops = c.warp_crops(_pages(), groups)
        m = sum(counts)
        assert crops.shape == (m, 31, 200) and bc.distinct_rows(crops)
        want = _by_pieces(lambda x: c.crnn_forward_scores(x) + c.crnn_beam(x, *BEAM) + c.crnn_lexicon(x, TOP_WORDS), m, crops)
        _conditions(want, f"recognize_boxes{counts} reference", STAGE_NAMES)
        _STAGE_REFERENCE[counts] = want
    return _STAGE_REFERENCE[counts]


@pytest.mark.parametrize("counts", [(600, 425), (1030, 1025)], ids=["M=1025", "M=2055"])
def test_recognize_boxes_with_every_switch_on(rec, counts):
    """the image index changes inside the first batch (600 / 1030 boxes on the first image)"""
    want = _stage_reference(rec, counts)
    groups = bc.boxes(counts, PAGE_H, PAGE_W)
    try:
        _switches_on(rec)
        labels = rec.recognize_boxes(_pages(), groups)
        got = (labels,) + rec.recognition_scores() + rec.recognition_beams() + rec.recognition_lexicon()
    finally:
        _switches_off(rec)
    _assert_same(got, want, f"recognize_boxes{counts}", STAGE_NAMES)


def _raw_fetch(c, name, buffers, max_crops, n_sizes):
    sizes = [ctypes.c_int32(-1) for _ in range(n_sizes)]
    fn = getattr(c._lib, name)  # pylint: disable=protected-access
    rc = fn(c._h, *[b.ctypes.data for b in buffers], max_crops, *[ctypes.byref(s) for s in sizes])  # pylint: disable=protected-access
    return rc, [s.value for s in sizes]


def test_raw_getters_past_one_batch(rec):
    """kocr_recognition_scores / _beams / _lexicon at M = 1025: too small a buffer is refused with the size reported and
    nothing written; the right size brings the bits, twice; the plain call afterwards returns the same labels"""
    from keras_ocr_amd._lib import KOCR_ECAPACITY, KOCR_OK

    counts, m, lw, k = (600, 425), 1025, 48, BEAM[1]
    want = _stage_reference(rec, counts)
    groups = bc.boxes(counts, PAGE_H, PAGE_W)
    getters = {
        "kocr_recognition_scores": (slice(1, 3), [m, lw]),
        "kocr_recognition_beams": (slice(3, 5), [m, lw, k]),
        "kocr_recognition_lexicon": (slice(5, 7), [m, TOP_WORDS]),
    }
    try:
        _switches_on(rec)
        labels = rec.recognize_boxes(_pages(), groups)
        for name, (part, sizes) in getters.items():
            rows = want[part]
            sentinel = [np.full_like(w, 0x5A5A5A5A if w.dtype == np.int32 else np.float32(-7.25)) for w in rows]
            small = [s[:m - 1].copy() for s in sentinel]
            rc, reported = _raw_fetch(rec, name, small, m - 1, len(sizes))
            assert rc == KOCR_ECAPACITY and reported == sizes, f"{name} with max_crops = {m - 1}: {rc}, {reported}"
            assert all(np.array_equal(_bits(a), _bits(s[:m - 1])) for a, s in zip(small, sentinel)), f"{name} wrote into a refused buffer"
            for again in range(2):
                full = [s.copy() for s in sentinel]
                rc, reported = _raw_fetch(rec, name, full, m, len(sizes))
                assert rc == KOCR_OK and reported == sizes, f"{name} with max_crops = {m}: {rc}, {reported}"
                _assert_same(tuple(full), rows, f"{name}, fetch {again + 1}", STAGE_NAMES[part])
    finally:
        _switches_off(rec)
    _assert_same(labels, want[0], "recognize_boxes before the fetches", ("labels",))
    _assert_same(rec.recognize_boxes(_pages(), groups), want[0], "the plain recognize_boxes after the fetches", ("labels",))
