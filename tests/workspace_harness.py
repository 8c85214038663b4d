"""What tests/test_workspace_gpu.py and tests/test_poison_gpu.py share: contexts per set of kernel switches with the networks a
row of tests/workspace_cases.py needs, the row's call, and results as bit patterns.  Nothing here touches a GPU until a context
is asked for."""
import functools
import os

import numpy as np
import pytest

from tests import workspace_cases as wc


# ---- contexts of this module's own: one per set of kernel switches, the networks loaded on demand ------------------------------
@functools.lru_cache(maxsize=None)
def _crnn_weights(classes, stn):
    import keras_ocr_amd

    w = dict(keras_ocr_amd.weights.synthetic_crnn_weights(4321, n_classes=classes))
    return w if stn else {k: v for k, v in w.items() if not k.startswith("stn_")}


@functools.lru_cache(maxsize=None)
def _craft_weights(kind):
    import keras_ocr_amd

    raw = keras_ocr_amd.weights.synthetic_craft_weights(1234)
    if kind == "raw":
        return raw
    if kind == "A":
        from tests import tiling_statement as ts
        return ts.fixture("A").weights
    from oracle import craft as ocraft
    return keras_ocr_amd.weights.calibrate_craft_head(raw, ocraft.detector_predict(raw, wc.page_detector_input()), text_frac=0.12,
                                                      link_frac=0.05)


class _Contexts:
    def __init__(self):
        self.made = {}

    def get(self, env):
        import keras_ocr_amd

        key = tuple(sorted(env.items()))
        if key not in self.made:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                c = keras_ocr_amd.Context(0)  # the switches are read here
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            self.made[key] = dict(ctx=c, crnn=None, craft=None)
        return self.made[key]

    def close(self):
        for state in self.made.values():
            state["ctx"].close()


def _prepare(state, r):
    """the row's networks, every switch at its default, then the row's own"""
    c = state["ctx"]
    if r["crnn"] is not None and state["crnn"] != r["crnn"]:
        classes, discard, stn = r["crnn"]
        c.crnn_set_rnn_steps_to_discard(discard)
        c.load_crnn(_crnn_weights(classes, stn))
        assert c.crnn_classes() == classes and c.crnn_label_width() == 50 - discard
        state["crnn"] = r["crnn"]
    if r["craft"] is not None and state["craft"] != r["craft"]:
        c.load_craft(_craft_weights(r["craft"]))
        state["craft"] = r["craft"]
    c.set_scores(False)
    c.set_beam(0)
    c.set_lexicon_match(0)
    c.set_lexicon_scratch(0)
    c.set_char_boxes(False)
    c.set_orientation(0)
    c.set_min_area_rect("exact")
    c.set_lexicon(None)
    c.set_patterns(None)
    c.set_charsets(None)
    for method, args in wc.setup_of(r):
        getattr(c, method)(*args)
    return c


def _bits(x):
    """anything a Context method returns as nested tuples of (dtype, shape, bytes)"""
    if hasattr(x, "render_detection"):
        x = x.render_detection()
    if isinstance(x, np.ndarray):
        return x.dtype.str, x.shape, np.ascontiguousarray(x).tobytes()
    if isinstance(x, dict):
        return tuple((k, _bits(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(_bits(v) for v in x)
    return x


def _where(a, b, path="out"):
    """the first place where two _bits trees differ"""
    if type(a) is not type(b) or (isinstance(a, tuple) and len(a) != len(b)):
        return f"{path}: {type(a).__name__} / {type(b).__name__}"
    if isinstance(a, tuple):
        for i, (x, y) in enumerate(zip(a, b)):
            if x != y:
                return _where(x, y, f"{path}[{i}]")
    if isinstance(a, bytes):
        n = next(i for i, (x, y) in enumerate(zip(a, b)) if x != y) if len(a) == len(b) else -1
        return f"{path}: first different byte {n} of {len(a)}"
    return f"{path}: {a!r} / {b!r}"


def _call(c, r):
    args, kwargs = wc.call_of(r)
    if r["raises"]:
        with pytest.raises(r["raises"][0], match=r["raises"][1]):
            getattr(c, r["method"])(*args, **kwargs)
        return ("refused",)
    return _bits(getattr(c, r["method"])(*args, **kwargs))
