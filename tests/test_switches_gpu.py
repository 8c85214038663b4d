"""A context's switches come back after every call that overrides them: with every switch set to a non-default value, each of
``Context.get_boxes``, ``detect``, ``recognize_boxes`` and ``pipeline`` is called with every per-call extra given (as other
values) and then with none; after each call the five getters report exactly what was set, and the plain call returns the bits
it returned before.  One call fails inside the scopes (IndexError after a capacity growth)."""
import numpy as np
import pytest

from tests import postproc_cases as pc, synth

pytestmark = pytest.mark.gpu

CHAR_RULE = {"peak_threshold": 0.5, "valley_ratio": 0.75, "extent_threshold": 0.25}
SET = (True, (3, 2), 2, "opencv", (True, CHAR_RULE))
PER_CALL_RULE = {"peak_threshold": 0.375, "valley_ratio": 0.5, "extent_threshold": 0.125}


def _bits(x):
    if isinstance(x, np.ndarray):
        return x.dtype.str, x.shape, x.tobytes()
    return tuple(_bits(v) for v in x) if isinstance(x, (list, tuple)) else x


def test_switches_come_back(craft_weights, crnn_weights):
    import keras_ocr_amd
    from oracle import craft as ocraft, tools as otools

    batch = np.stack([synth.text_page(96, 128, 5, seed=21), synth.text_page(96, 128, 4, seed=23)])
    big = np.stack([otools.resize_image(p, 2, 2048)[0] for p in batch])
    weights = keras_ocr_amd.weights.calibrate_craft_head(craft_weights, ocraft.detector_predict(craft_weights, big[:1]),
                                                         text_frac=0.10, link_frac=0.04)
    ctx = keras_ocr_amd.Context(0)
    try:
        keras_ocr_amd.detection.Detector(weights=weights, ctx=ctx)
        rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=ctx)
        rec.set_lexicon(["ab", "c", "cab"])
        ctx.set_scores(True)
        ctx.set_beam(*SET[1])
        ctx.set_lexicon_match(SET[2])
        ctx.set_min_area_rect(SET[3])
        ctx.set_char_boxes(True, **CHAR_RULE)

        def switches():
            return ctx.get_scores(), ctx.get_beam(), ctx.get_lexicon_match(), ctx.get_min_area_rect(), ctx.get_char_boxes()

        assert switches() == SET
        heat = ctx.craft_forward(big)
        boxes = ctx.get_boxes(heat)
        assert max(len(b) for b in boxes) > 1
        fused = (list(batch), [96] * 2, [128] * 2, [192] * 2, [256] * 2, 192, 256)
        detection = dict(min_area_rect="exact", return_scores=True, char_boxes=PER_CALL_RULE)
        recognition = dict(return_scores=True, beam=(4, 3), lexicon_top=3)
        calls = {
            "get_boxes": (lambda **kw: ctx.get_boxes(heat, **kw), detection, 3),
            "detect": (lambda **kw: ctx.detect(big, **kw), detection, 3),
            "recognize_boxes": (lambda **kw: ctx.recognize_boxes(big, boxes, **kw), recognition, 7),
            "pipeline": (lambda **kw: ctx.pipeline(*fused, **kw), dict(detection, **recognition), 5),
        }
        for name, (call, extras, length) in calls.items():
            before = call()
            assert switches() == SET, name
            with_extras = call(**extras)
            assert switches() == SET, f"{name} with {sorted(extras)}"
            assert isinstance(with_extras, tuple) and len(with_extras) == length, name
            after = call()
            assert switches() == SET, name
            assert _bits(after) == _bits(before), f"{name}: the plain call changed after one with per-call extras"
        # a call that fails inside the scopes: the capacity growth comes first, then the empty contour list
        case = pc.case("empty_contour_among_valid")
        with pytest.raises(IndexError):
            ctx.get_boxes(case["heat"], cap=1, **detection, **case["kwargs"])
        assert switches() == SET
        assert _bits(ctx.get_boxes(heat)) == _bits(boxes)
    finally:
        ctx.close()
