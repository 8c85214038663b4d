"""CPU suite: the float64 statement of evaluation on the device (tests/evaluation_statement.py) against the host path
keras_ocr_amd/evaluation.py, and the surface the feature adds."""
import inspect
import os
import subprocess
import warnings

import numpy as np
import pytest

from tests import evaluation_cases as ec
from tests import evaluation_statement as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = [(0, 0), (100, 0), (100, 100), (0, 100)]


def test_reference_values():
    """the reference's own values (its tests/test_evaluation.py:4-10) and the two of tests/test_evaluation_cpu.py"""
    assert es.iou(SQUARE, [(50, 50), (100, 50), (100, 100), (50, 100)]) == 0.25
    assert es.iou(SQUARE, [(100, 100), (200, 100), (200, 200), (100, 200)]) == 0.0
    assert es.iou(es.as_quad([(0, 0), (10, 10)]), [(0, 0), (10, 0), (10, 10), (0, 10)]) == 1.0
    np.testing.assert_allclose(es.iou(SQUARE, [(50, 0), (100, 50), (50, 100), (0, 50)]), 0.5, rtol=0, atol=1e-15)


def test_chevron_by_hand():
    """A chevron (0,0) (50,30) (100,0) (50,100): the triangle (0,0) (100,0) (50,100) of area 5000 without the notch
    (0,0) (50,30) (100,0) of area 1500.  At height y <= 30 it is the two strips between the outer edges x = y/2,
    x = 100 - y/2 and the notch edges x = y/0.6, x = 100 - y/0.6: width 7y/3, so the band 0 <= y <= 30 holds
    7/6 * 900 = 1050 of it.  Against the 100 x 30 rectangle: 1050 / (3500 + 3000 - 1050); against the whole square, which
    contains it: 3500 / 10000.  Every corner order and both orientations."""
    chevron = [(0, 0), (50, 30), (100, 0), (50, 100)]
    band = [(0, 0), (100, 0), (100, 30), (0, 30)]
    from keras_ocr_amd import evaluation

    for k in range(4):
        for quad in (chevron[k:] + chevron[:k], (chevron[k:] + chevron[:k])[::-1]):
            tris = es.triangulate_quad(quad, es.area2(quad))
            assert len(tris) == 2 and sum(abs(es.area2(t)) for t in tris) == 7000
            np.testing.assert_allclose(es.iou(quad, band), 1050 / 5450, rtol=0, atol=1e-14)
            np.testing.assert_allclose(es.iou(band, quad), 1050 / 5450, rtol=0, atol=1e-14)
            np.testing.assert_allclose(es.iou(quad, SQUARE), 0.35, rtol=0, atol=1e-14)
            np.testing.assert_allclose(evaluation.iou_score(quad, band), 1050 / 5450, rtol=0, atol=1e-14)


def test_degenerate_boxes():
    line = [(0, 0), (10, 5), (20, 10), (30, 15)]
    assert es.iou(line, SQUARE) == 0.0 and es.iou(SQUARE, line) == 0.0
    triangle = [(0, 0), (0, 0), (100, 0), (0, 100)]  # a repeated corner: one triangle of area 5000 inside the square
    assert len(es.triangulate_quad(triangle, es.area2(triangle))) == 1
    assert es.iou(triangle, SQUARE) == 0.5
    with pytest.raises(ValueError):
        es.as_quad([(0, 0), (1, 0), (1, 1)])


def test_statement_against_host_iou():
    """22 016 generated pairs (tests/evaluation_cases.py::quad_pairs), of which the 20 640 that are not self-intersecting
    are compared: rotated rectangles with jitter, convex quads, chevrons, touching, disjoint and identical boxes, negative
    coordinates, boxes spanning +-2^24, repeated corners, zero areas.

    Statement and host are float64 evaluations of one formula; they differ in the summation order of the shoelace sums of
    clipped polygons (np.dot) only.  Largest absolute difference measured on the CPU over these pairs: 6.9e-12 (the
    rectangles with jitter; 3.4e-15 for the boxes near 2^24, 0 for touching, disjoint, identical and zero-area boxes).  The
    gate is 100 times that, which stays below the 1e-9 that holds in any case.

    The generator's self-intersecting quads ("bowtie") are left out of this comparison altogether: the rule promises
    nothing for them beyond "the kernel gives what the statement gives" (their two lobes nearly cancel in the signed area,
    so the quotient is no IoU), and that is checked on their bits in tests/test_evaluation_gpu.py."""
    from keras_ocr_amd import evaluation

    pairs = [pair for i, pair in enumerate(ec.quad_pairs(22016, 11)) if ec.kind_of(i) != "bowtie"]
    assert len(pairs) >= 20000
    gate = min(100 * 6.9e-12, 1e-9)
    worst = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for a, b in pairs:
            worst = max(worst, abs(es.iou(a, b) - float(evaluation.iou_score(a, b))))
    print(f"statement vs host: {len(pairs)} pairs, max |difference| {worst:.3e} (gate {gate:.1e})")
    assert worst <= gate


@pytest.mark.parametrize("name", ["precision_recall", "bookkeeping", "pages", "crowded"])
def test_score_tables_against_host(name):
    from keras_ocr_amd import evaluation

    true, pred, kwargs = ec.scenarios()[name]
    ids, tables_in = ec.tables_input(true, pred, kwargs.get("translator"))
    tables = es.score_tables(iou_threshold=0.5, similarity_threshold=0.5, **tables_in)
    assert es.results_from_tables(ids, tables) == evaluation.score(true, pred, **kwargs)


def test_pages_scenario_is_rich_and_clear_of_the_threshold():
    """the generated pages exercise every list, ignored truths and both text ties, and no pair's IoU lies within 1e-6 of
    the threshold (the GPU test compares dictionaries for equality and asserts the same)"""
    from keras_ocr_amd import evaluation

    true, pred, kwargs = ec.scenario_pages()
    assert len(true) == 32 and all(len(v) == 22 for v in true.values())
    results, (precision, recall) = evaluation.score(true, pred, **kwargs)
    assert all(len(v) > 20 for v in results.values()) and 0 < precision < 1 and 0 < recall < 1
    ids, tables_in = ec.tables_input(true, pred, kwargs["translator"])
    tables = es.score_tables(iou_threshold=0.5, similarity_threshold=0.5, **tables_in)
    flat = [v for image in tables["iou"] for row in image for v in row]
    assert len(flat) > 15000 and min(abs(v - 0.5) for v in flat) > 1e-6
    assert any(3 in row for image in tables["pair_class"] for row in image)
    texts = {(t["text"], p["text"]) for i in ids for t in true[i] for p in pred[i]}
    assert ("ab", "ax") in texts and ("", "") in texts
    assert es.similarity([ord("a"), ord("b")], [ord("a"), ord("x")]) == 0.5 and es.similarity([], []) == 1.0


def test_crowded_scenario_outgrows_a_grid_and_a_block():
    """the text kernel's grid is min(pairs, words, 1024) one-wave blocks (launch_eval_text in csrc/evaluate.hip), the
    reduction runs 256 threads over an image's truths and then its predictions: the scenario lists more pairs than the grid
    has blocks, and has an image wider than 256 of either kind"""
    true, pred, kwargs = ec.scenario_crowded()
    ids, tables_in = ec.tables_input(true, pred, kwargs.get("translator"))
    assert ids == ["a", "b", "c", "d"] == list(true) == list(pred)
    tables = es.score_tables(iou_threshold=0.5, similarity_threshold=0.5, **tables_in)
    classes = [c for image in tables["pair_class"] for row in image for c in row]
    pairs = sum(len(true[i]) * len(pred[i]) for i in ids)
    words = sum(len(true[i]) + len(pred[i]) for i in ids)
    grid = min(pairs, words, 1024)
    listed = classes.count(1) + classes.count(2)
    assert len(classes) == pairs == 4600 and words == 690 and listed == 1560 + 8 > 2 * grid
    assert min(classes.count(c) for c in (1, 2)) > 500 and classes.count(3) == 42
    assert len(true["b"]) > 256 and len(pred["c"]) > 256 and not true["d"] and not pred["d"]
    # beyond the 256th truth / prediction there are both kinds of flag
    assert {0, 1} == set(tables["truth_missed"][1][256:]) == set(tables["pred_unclaimed"][2][256:])
    flat = [v for image in tables["iou"] for row in image for v in row]
    assert min(abs(v - 0.5) for v in flat) > 1e-6
    # image a: every pair overlaps, and the lengths 0, 1, 64, 65 and 256 occur on both sides
    assert all(v >= 0.5 for row in tables["iou"][0] for v in row)
    for texts in (tables_in["truth_texts"][0], tables_in["pred_texts"][0]):
        assert set(ec.CROWDED_LENGTHS) <= {len(t) for t in texts} and max(len(t) for t in texts) == es.MAX_TEXT
    lengths = [(len(t), len(p)) for ti, t in enumerate(tables_in["truth_texts"][0]) if not tables_in["truth_ignore"][0][ti]
               for p in tables_in["pred_texts"][0]]
    assert sum(1 for (a, b), (c, d) in zip(lengths, lengths[1:]) if max(a, b) > 60 and max(c, d) < 16) >= 8  # a long pair, then a short one
    # both classes where a 256-point text is involved, and ("", "") is a true positive
    row = tables["pair_class"][0][[len(t) for t in tables_in["truth_texts"][0]].index(256)]
    assert 1 in row and 2 in row
    assert tables["pair_class"][0][2][5] == 1 and tables_in["truth_texts"][0][2] == [] == tables_in["pred_texts"][0][5]


def test_levenshtein():
    from keras_ocr_amd import evaluation

    rng = np.random.default_rng(3)
    for _ in range(200):
        a = rng.integers(97, 101, int(rng.integers(0, 12))).tolist()
        b = rng.integers(97, 101, int(rng.integers(0, 12))).tolist()
        assert es.levenshtein(a, b) == evaluation._edit_distance(a, b)  # pylint: disable=protected-access
    assert es.levenshtein([1] * 256, [2] * 256) == 256 and es.levenshtein([], [5, 6]) == 2


def test_symbols_and_signatures():
    import __graft_entry__

    __graft_entry__.build()
    import keras_ocr_amd
    from keras_ocr_amd import evaluation, pipeline

    lib = keras_ocr_amd.load_library()
    assert hasattr(lib, "kocr_iou_table") and hasattr(lib, "kocr_score")
    assert lib.kocr_score.argtypes is not None and len(lib.kocr_score.argtypes) == 21 and len(lib.kocr_iou_table.argtypes) == 10
    names = subprocess.run(["nm", "-D", "--defined-only", keras_ocr_amd._lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T kocr_iou_table" in names and " T kocr_score" in names
    parameters = inspect.signature(evaluation.score).parameters
    assert list(parameters) == ["true", "pred", "iou_threshold", "similarity_threshold", "translator", "ctx", "return_results"]
    assert parameters["ctx"].default is None and parameters["return_results"].default is True
    assert list(inspect.signature(evaluation.iou_matrix).parameters) == ["boxes_a", "boxes_b", "ctx"]
    assert list(inspect.signature(pipeline.Pipeline.evaluate).parameters)[:5] == ["self", "images", "true", "detection_kwargs", "recognition_kwargs"]
    header = open(os.path.join(ROOT, "include", "kocr.h")).read()
    assert "#define KOCR_SCORE_MAX_TEXT 256" in header and es.MAX_TEXT == 256


def test_device_path_refuses_before_any_gpu_call():
    """what the device path cannot take is refused on the host: no context is touched (ctx is a sentinel here)"""
    from keras_ocr_amd import evaluation

    box = ec.sq(0, 0)
    for bad in ([(0, 0), (5, 0), (5, 5)], [(0, 0), (5, 0), (6, 3), (5, 5), (0, 5)]):
        with pytest.raises(ValueError, match=r"image 'p', prediction 1"):
            evaluation.score({"p": [{"text": "a", "vertices": box}]},
                             {"p": [{"text": "a", "vertices": box}, {"text": "b", "vertices": bad}]}, ctx=object())
    with pytest.raises(ValueError, match=r"image 'p', truth 0.*257"):
        evaluation.score({"p": [{"text": "a" * 257, "vertices": box}]}, {"p": []}, ctx=object())
    with pytest.raises(AssertionError):
        evaluation.score({"x": []}, {"y": []}, ctx=object())
    with pytest.raises(ValueError, match="beam_width"):
        from keras_ocr_amd import pipeline
        pipeline.Pipeline(detector=object(), recognizer=object()).evaluate([], [], recognition_kwargs={"beam_width": 4})
    with pytest.raises(ValueError, match="lexicon_top"):
        pipeline.Pipeline(detector=object(), recognizer=object()).evaluate([], [], recognition_kwargs={"lexicon_top": 2})
