"""GPU suite: evaluation on the device (kocr_iou_table / kocr_score) against its float64 statement
(tests/evaluation_statement.py), bit for bit, and against the host path keras_ocr_amd/evaluation.py, for equality."""
import ctypes
import warnings

import numpy as np
import pytest

from tests import evaluation_cases as ec
from tests import evaluation_statement as es

pytestmark = pytest.mark.gpu


def _bits(values):
    return np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)


def _ragged_batch(images=64, seed=5):
    """64 images of ragged sizes from the generator's quads: image i takes a run of pairs, their first quads as truths and
    a (differently long) run of second quads as predictions; every eighth image has no truths, every eighth none of the
    other kind."""
    rng = np.random.default_rng(seed)
    pairs = ec.quad_pairs(64 * 24, 23)
    truths, preds, at = [], [], 0
    for i in range(images):
        nt, npred = int(rng.integers(1, 25)), int(rng.integers(1, 25))
        run = pairs[at:at + 24]
        at += 24
        truths.append([] if i % 8 == 3 else [a for a, _ in run[:nt]])
        preds.append([] if i % 8 == 6 else [b for _, b in run[:npred]])
    return truths, preds


def _flatten(groups):
    quads = np.array([q for g in groups for q in g], dtype=np.int32).reshape(-1, 4, 2)
    return quads, np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)


def test_iou_bits_equal_the_statement(ctx):
    truths, preds = _ragged_batch()
    assert any(not t for t in truths) and any(not p for p in preds)
    tq, toff = _flatten(truths)
    pq, poff = _flatten(preds)
    got = ctx.iou_table(tq, toff, pq, poff)
    want = [es.iou(t, p) for ts, ps in zip(truths, preds) for t in ts for p in ps]
    assert len(want) == len(got) > 5000 and want.count(0.0) > 100 and sum(1 for v in want if v > 0.3) > 150
    zero = sum(1 for ts in truths for t in ts if es.area2(t) == 0) + sum(1 for ps in preds for p in ps if es.area2(p) == 0)
    assert zero > 20
    different = np.flatnonzero(_bits(got) != _bits(want))
    assert different.size == 0, (different[:5], got[different[:5]], np.array(want)[different[:5]])
    # every pair of the generator on its own: 20 480 images of one truth and one prediction
    pairs = ec.quad_pairs(20480, 11)
    tq = np.array([a for a, _ in pairs], np.int32)
    pq = np.array([b for _, b in pairs], np.int32)
    off = np.arange(len(pairs) + 1, dtype=np.int32)
    got = ctx.iou_table(tq, off, pq, off)
    want = np.array([es.iou(a, b) for a, b in pairs])
    different = np.flatnonzero(_bits(got) != _bits(want))
    assert different.size == 0, (different[:5], [ec.kind_of(int(i)) for i in different[:5]], got[different[:5]], want[different[:5]])


def test_iou_matrix_equals_iou_score(ctx):
    from keras_ocr_amd import evaluation

    boxes_a = [[(0, 0), (100, 0), (100, 100), (0, 100)], [(0, 0), (10, 10)], [(50.7, 0.2), (100.9, 50), (50, 100), (0, 50)]]
    boxes_b = [[(50, 50), (100, 50), (100, 100), (50, 100)], [(100, 100), (200, 100), (200, 200), (100, 200)],
               [(0, 0), (10, 0), (10, 10), (0, 10)], [(50, 0), (100, 50), (50, 100), (0, 50)]]
    got = evaluation.iou_matrix(boxes_a, boxes_b, ctx=ctx)
    assert got.shape == (3, 4) and got.dtype == np.float64
    assert got[0, 0] == 0.25 and got[0, 1] == 0.0 and got[1, 2] == 1.0
    want = np.array([[evaluation.iou_score(a, b) for b in boxes_b] for a in boxes_a])
    np.testing.assert_allclose(got, want, rtol=0, atol=6.9e-10)
    assert evaluation.iou_matrix([], boxes_b, ctx=ctx).shape == (0, 4)


@pytest.mark.parametrize("name", ["precision_recall", "bookkeeping", "pages", "crowded"])
def test_score_equals_the_host_path(ctx, name):
    from keras_ocr_amd import evaluation

    true, pred, kwargs = ec.scenarios()[name]
    ids, tables_in = ec.tables_input(true, pred, kwargs.get("translator"))
    tables = es.score_tables(iou_threshold=0.5, similarity_threshold=0.5, **tables_in)
    flat = [v for image in tables["iou"] for row in image for v in row]
    assert min(abs(v - 0.5) for v in flat) > 1e-6, "a pair of the scenario lies within 1e-6 of the threshold"
    want = evaluation.score(true, pred, **kwargs)
    got = evaluation.score(true, pred, ctx=ctx, **kwargs)
    assert got == want
    assert type(got[1][0]) is type(want[1][0]) and list(got[0]) == list(want[0])
    assert evaluation.score(true, pred, ctx=ctx, return_results=False, **kwargs) == (None, want[1])


def _arrays(true, pred, translator=None):
    """a scenario as Context.score_tables takes it, plus the per-image sizes"""
    ids, t = ec.tables_input(true, pred, translator)
    tq, toff = _flatten(t["truth_quads"])
    pq, poff = _flatten(t["pred_quads"])
    ignore = np.array([v for g in t["truth_ignore"] for v in g], np.uint8)
    texts = []
    for groups in (t["truth_texts"], t["pred_texts"]):
        rows = [r for g in groups for r in g]
        texts += [np.array([c for r in rows for c in r], np.int32), np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)]
    return ids, t, (tq, toff, pq, poff, ignore, *texts)


def _check_tables(ctx, true, pred, translator):
    """Context.score_tables against the statement, and every image alone against its slice of the batch"""
    ids, t, arrays = _arrays(true, pred, translator)
    tables = es.score_tables(iou_threshold=0.5, similarity_threshold=0.5, **t)
    cls, missed, unclaimed, counts, iou = ctx.score_tables(*arrays, return_iou=True)
    assert cls.tolist() == [c for image in tables["pair_class"] for row in image for c in row]
    assert missed.tolist() == [v for image in tables["truth_missed"] for v in image]
    assert unclaimed.tolist() == [v for image in tables["pred_unclaimed"] for v in image]
    assert counts.tolist() == tables["counts"]
    assert np.array_equal(_bits(iou), _bits([v for image in tables["iou"] for row in image for v in row]))
    assert np.array_equal(_bits(iou), _bits(ctx.iou_table(*arrays[:4])))
    # every image alone: the same flag bytes and IoU bits as inside the batch
    tq, toff, pq, poff = arrays[:4]
    pair_off = np.concatenate([[0], np.cumsum(np.diff(toff).astype(np.int64) * np.diff(poff))])
    for n, image_id in enumerate(ids):
        _, _, one = _arrays({image_id: true[image_id]}, {image_id: pred[image_id]}, translator)
        c1, m1, u1, k1, i1 = ctx.score_tables(*one, return_iou=True)
        assert np.array_equal(c1, cls[pair_off[n]:pair_off[n + 1]]) and np.array_equal(_bits(i1), _bits(iou[pair_off[n]:pair_off[n + 1]]))
        assert np.array_equal(m1, missed[toff[n]:toff[n + 1]]) and np.array_equal(u1, unclaimed[poff[n]:poff[n + 1]])
        assert k1.tolist() == [sum(1 for row in tables["pair_class"][n] if 1 in row), int(u1.sum()), int(m1.sum())]
    return tables


def test_tables_equal_the_statement_and_do_not_depend_on_the_batch(ctx):
    true, pred, kwargs = ec.scenario_pages()
    _check_tables(ctx, true, pred, kwargs["translator"])


def test_crowded_tables_equal_the_statement(ctx):
    """more listed pairs than eval_text_kernel has blocks (each block takes a second and a third pair, long texts before
    short ones), and images of more than 256 truths or predictions in eval_reduce_kernel"""
    true, pred, kwargs = ec.scenario_crowded()
    tables = _check_tables(ctx, true, pred, kwargs.get("translator"))
    classes = [c for image in tables["pair_class"] for row in image for c in row]
    assert classes.count(1) + classes.count(2) > min(len(classes), sum(len(true[i]) + len(pred[i]) for i in true), 1024)


def test_limits_and_errors(ctx):
    from keras_ocr_amd import evaluation

    box = ec.sq(0, 0)
    long_a, long_b = "a" * 256, "a" * 128 + "b" * 128
    true = {"p": [{"text": long_a, "vertices": box}, {"text": long_a, "vertices": ec.sq(40, 0)}]}
    pred = {"p": [{"text": long_b, "vertices": box}, {"text": "a" * 127 + "b" * 129, "vertices": ec.sq(40, 0)}]}
    # 128 of 256 code points differ: similarity exactly 0.5; 129 differ: just below
    want = evaluation.score(true, pred)
    assert [len(want[0][k]) for k in ("true_positives", "near_true_positives")] == [1, 1]
    assert evaluation.score(true, pred, ctx=ctx) == want
    with pytest.raises(ValueError, match="257"):
        evaluation.score({"p": [{"text": "a" * 257, "vertices": box}]}, {"p": [{"text": "a", "vertices": box}]}, ctx=ctx)
    for bad in ([(0, 0), (5, 0), (5, 5)], [(0, 0), (5, 0), (6, 3), (5, 5), (0, 5)]):
        with pytest.raises(ValueError, match="image 'p', truth 0"):
            evaluation.score({"p": [{"text": "a", "vertices": bad}]}, {"p": [{"text": "a", "vertices": box}]}, ctx=ctx)
    with pytest.raises(AssertionError):
        evaluation.score({"x": []}, {"y": []}, ctx=ctx)
    # the host divides by zero where nothing matches: the same exception
    for true, pred in (({}, {}), ({"a": [], "b": []}, {"a": [], "b": []})):
        with pytest.raises(ZeroDivisionError):
            evaluation.score(true, pred)
        with pytest.raises(ZeroDivisionError):
            evaluation.score(true, pred, ctx=ctx)
        with pytest.raises(ZeroDivisionError):
            evaluation.score(true, pred, ctx=ctx, return_results=False)
    only_truths = {"a": [{"text": "w", "vertices": box}]}, {"a": []}
    with pytest.raises(ZeroDivisionError):
        evaluation.score(*only_truths)
    with pytest.raises(ZeroDivisionError):
        evaluation.score(*only_truths, ctx=ctx)
    # a zero-area box in a pair warns, as the host does
    flat = {"a": [{"text": "w", "vertices": [(0, 0), (10, 0), (20, 0), (30, 0)]}, {"text": "v", "vertices": box}]}
    with pytest.warns(UserWarning, match="zero area"):
        got = evaluation.score(flat, {"a": [{"text": "v", "vertices": box}]}, ctx=ctx)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert got == evaluation.score(flat, {"a": [{"text": "v", "vertices": box}]})
    # a coordinate the exactness argument does not cover
    with pytest.raises(ValueError, match=r"image 0, prediction 1"):
        ctx.iou_table(np.array([box], np.int32), [0, 1], np.array([box, [(0, 0), (1 << 24, 0), (1 << 24, 5), (0, 5)]], np.int32), [0, 2])


def test_raw_abi_capacity_and_empty_batches(ctx):
    import keras_ocr_amd
    from keras_ocr_amd import _lib

    lib = keras_ocr_amd.load_library()
    tq = np.array([ec.sq(0, 0), ec.sq(5, 0), ec.sq(50, 50)], np.int32)
    pq = np.array([ec.sq(0, 0), ec.sq(50, 50)], np.int32)
    toff, poff = np.array([0, 2, 3], np.int32), np.array([0, 1, 2], np.int32)  # 2 x 1 + 1 x 1 = 3 pairs
    iou = np.zeros(3, np.float64)
    true_p = ctypes.c_int64(-1)
    handle = ctx._h  # pylint: disable=protected-access
    rc = lib.kocr_iou_table(handle, 2, _lib._ptr(tq), _lib._ptr(toff), _lib._ptr(pq), _lib._ptr(poff), _lib._ptr(iou), 2, ctypes.byref(true_p), 0)
    assert rc == _lib.KOCR_ECAPACITY and true_p.value == 3
    assert b"3 pairs" in lib.kocr_last_error(handle)
    true_p = ctypes.c_int64(-1)
    rc = lib.kocr_iou_table(handle, 2, _lib._ptr(tq), _lib._ptr(toff), _lib._ptr(pq), _lib._ptr(poff), _lib._ptr(iou), 3, ctypes.byref(true_p), 0)
    assert rc == 0 and true_p.value == 3 and iou.tolist() == [1.0, es.iou(ec.sq(5, 0), ec.sq(0, 0)), 1.0]
    bad = np.array([0, 2, 1], np.int32)
    assert lib.kocr_iou_table(handle, 2, _lib._ptr(tq), _lib._ptr(bad), _lib._ptr(pq), _lib._ptr(poff), _lib._ptr(iou), 3, None, 0) == _lib.KOCR_EINVAL
    assert b"truth_offsets decreases" in lib.kocr_last_error(handle)
    # N = 0, and images without pairs
    assert ctx.iou_table(np.zeros((0, 4, 2), np.int32), [0], np.zeros((0, 4, 2), np.int32), [0]).shape == (0,)
    empty = np.zeros(0, np.int32)
    cls, missed, unclaimed, counts = ctx.score_tables(np.zeros((0, 4, 2), np.int32), [0], np.zeros((0, 4, 2), np.int32), [0], [], empty, [0], empty, [0])
    assert cls.size == missed.size == unclaimed.size == 0 and counts.tolist() == [0, 0, 0]
    cls, missed, unclaimed, counts = ctx.score_tables(tq, [0, 3, 3], pq, [0, 0, 2], [0, 1, 0], empty, [0, 0, 0, 0], empty, [0, 0, 0])
    assert cls.size == 0 and missed.tolist() == [1, 0, 1] and unclaimed.tolist() == [1, 1] and counts.tolist() == [0, 2, 2]


def test_pipeline_evaluate(craft_weights, crnn_weights):
    """a small synthetic page, the detector's head calibrated as in __graft_entry__.smoke"""
    import keras_ocr_amd
    from keras_ocr_amd import evaluation
    from oracle import craft as ocraft, tools as otools

    rng = np.random.default_rng(0)
    page = np.full((64, 96, 3), 255, np.uint8)
    for _ in range(4):
        x, y = int(rng.integers(0, 60)), int(rng.integers(0, 50))
        page[y:y + 10, x:x + 30] = rng.integers(0, 120, (10, 30, 3), dtype=np.uint8)
    big = otools.resize_image(page, 2, 2048)[0][None]
    cw = keras_ocr_amd.weights.calibrate_craft_head(craft_weights, ocraft.detector_predict(craft_weights, big), text_frac=0.12, link_frac=0.05)
    context = keras_ocr_amd.Context(0)
    try:
        det = keras_ocr_amd.detection.Detector(weights=cw, ctx=context)
        rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=context)
        pipe = keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)
        plain = pipe.recognize([page, page])
        assert len(plain[0]) > 0
        # truths from the predictions: the first word as it is, the second moved away, one more that nothing predicts
        true = []
        for group in plain:
            anns = [{"text": text, "vertices": box.copy()} for text, box in group]
            if len(anns) > 1:
                anns[1]["vertices"] = anns[1]["vertices"] + 500
            anns.append({"text": "absent", "vertices": [(900, 900), (950, 920)]})
            true.append(anns)
        predictions, results, precision_recall = pipe.evaluate([page, page], true)
        assert len(predictions) == len(plain)
        for got, want in zip(predictions, plain):
            assert [t for t, _ in got] == [t for t, _ in want] and all(np.array_equal(a[1], b[1]) for a, b in zip(got, want))
        pred = {i: [{"text": text, "vertices": box} for text, box in group] for i, group in enumerate(predictions)}
        want = evaluation.score(dict(enumerate(true)), pred)
        assert (results, precision_recall) == want
        assert len(results["true_positives"]) >= 2 and len(results["false_negatives"]) >= 2
        assert pipe.evaluate([page, page], true, return_results=False)[1:] == (None, want[1])
        with pytest.raises(ValueError, match="beam_width"):
            pipe.evaluate([page], true[:1], recognition_kwargs={"beam_width": 4})
    finally:
        context.close()
