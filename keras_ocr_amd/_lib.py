"""ctypes binding of libkocr.so (the C-ABI declared in include/kocr.h).

The shared library is built in-tree by ``__graft_entry__.build()`` /
``make -C keras_ocr_amd/csrc``.  There is NO CPU fallback: if the library is missing or
no HIP device is visible, the product fails loudly here.
"""
import contextlib
import ctypes
import math
import os

import numpy as np

from .extras import Extras  # pylint: disable=cyclic-import  (it reads this module's validators when called)
from .results import Results, empty_beam, empty_lexicon, empty_orientation, empty_pattern, empty_scores

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libkocr.so")

KOCR_U8, KOCR_F32 = 0, 1
# return codes (include/kocr.h)
KOCR_OK, KOCR_EINVAL, KOCR_EHIP, KOCR_ENOWEIGHTS, KOCR_ECAPACITY, KOCR_ENOMEM, KOCR_EEMPTYCONTOUR, KOCR_EZERODIV = range(0, -8, -1)
KOCR_LINES_BLOCKS = 1  # kocr_group_lines' flags: blocks instead of lines (include/kocr.h)
KOCR_LINES_DESKEW = 4  # beside KOCR_LINES_BLOCKS: the cut runs in the page's own frame
KOCR_LINES_TABLE = 16  # alone: rows, columns and spanning cells of a table's word boxes
# minAreaRect rule of getBoxes (include/kocr.h: KOCR_RECT_EXACT / KOCR_RECT_OPENCV)
MIN_AREA_RECT_RULES = {"exact": 0, "opencv": 1}

_c_float_p = ctypes.POINTER(ctypes.c_float)
_c_int_p = ctypes.POINTER(ctypes.c_int)
_c_i64_p = ctypes.POINTER(ctypes.c_int64)
_c_dbl_p = ctypes.POINTER(ctypes.c_double)

_lib = None


class KocrError(RuntimeError):
    """A libkocr call returned a non-zero code."""


def load_library():
    """Load libkocr.so (once).  Raises ImportError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C keras_ocr_amd/csrc). "
            "keras-ocr_amd has no CPU fallback.")
    # PyTorch's wheel bundles its own HIP/HSA runtime.  If libkocr (linked against the system ROCm)
    # initialises HIP first, a later `import torch` finds "No HIP GPUs" in its private runtime; the
    # other order works.  torch is only plumbing here (device buffers in bench.py, torch.distributed),
    # so when it is installed it is imported before the library is loaded.
    try:
        import torch  # noqa: F401  pylint: disable=import-outside-toplevel,unused-import
    except ImportError:  # pragma: no cover
        pass
    lib = ctypes.CDLL(LIB_PATH)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    sigs = {
        "kocr_create": (ci, [ctypes.POINTER(vp), ci]),
        "kocr_destroy": (None, [vp]),
        "kocr_last_error": (ctypes.c_char_p, [vp]),
        "kocr_set_stream": (ci, [vp, vp]),
        "kocr_synchronize": (ci, [vp]),
        "kocr_device_alloc": (ci, [vp, ctypes.POINTER(vp), ctypes.c_uint64]),
        "kocr_device_free": (ci, [vp, vp]),
        "kocr_memcpy_h2d": (ci, [vp, vp, vp, ctypes.c_uint64]),
        "kocr_memcpy_d2h": (ci, [vp, vp, vp, ctypes.c_uint64]),
        "kocr_load_craft": (ci, [vp, ci, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp), _c_i64_p, _c_int_p]),
        "kocr_load_crnn": (ci, [vp, ci, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(vp), _c_i64_p, _c_int_p]),
        "kocr_craft_forward": (ci, [vp, vp, ci, ci, ci, ci, vp, ci, ci]),
        "kocr_craft_set_taps": (ci, [vp, ci, ctypes.POINTER(ctypes.c_char_p)]),
        "kocr_craft_tap_count": (ci, [vp]),
        "kocr_craft_tap_info": (ci, [vp, ci, ctypes.c_char_p, ctypes.c_char_p, vp]),
        "kocr_craft_get_tap": (ci, [vp, ctypes.c_char_p, ci, vp, vp]),
        "kocr_crnn_set_taps": (ci, [vp, ci, ctypes.POINTER(ctypes.c_char_p)]),
        "kocr_crnn_forward": (ci, [vp, vp, ci, vp, vp, ci]),
        "kocr_crnn_forward_scores": (ci, [vp, vp, ci, vp, vp, vp, vp, ci]),
        "kocr_crnn_beam": (ci, [vp, vp, ci, ci, ci, vp, vp, ci]),
        "kocr_set_beam": (ci, [vp, ci, ci]),
        "kocr_get_beam": (ci, [vp, vp, vp]),
        "kocr_recognition_beams": (ci, [vp, vp, vp, ci, vp, vp, vp]),
        "kocr_set_lexicon": (ci, [vp, vp, ci, vp, ci]),
        "kocr_lexicon_size": (ci, [vp]),
        "kocr_crnn_lexicon": (ci, [vp, vp, ci, ci, vp, vp, vp, ci]),
        "kocr_set_lexicon_match": (ci, [vp, ci]),
        "kocr_get_lexicon_match": (ci, [vp, vp]),
        "kocr_recognition_lexicon": (ci, [vp, vp, vp, ci, vp, vp]),
        "kocr_set_lexicon_scratch": (ci, [vp, ctypes.c_uint64]),
        "kocr_set_charsets": (ci, [vp, vp, ci, ci]),
        "kocr_charset_count": (ci, [vp]),
        "kocr_set_charset": (ci, [vp, ci]),
        "kocr_get_charset": (ci, [vp, vp]),
        "kocr_recognize_boxes_charsets": (ci, [vp, vp, ci, ci, ci, vp, vp, vp, ci, vp]),
        "kocr_crnn_decode_logits_charsets": (ci, [vp, vp, ci, vp, vp, vp, vp, ci, ci, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, vp, vp]),
        "kocr_set_patterns": (ci, [vp, vp, vp, vp, ci, ci]),
        "kocr_pattern_count": (ci, [vp]),
        "kocr_set_pattern": (ci, [vp, ci]),
        "kocr_get_pattern": (ci, [vp, vp]),
        "kocr_recognition_patterns": (ci, [vp, vp, vp, vp, ci, vp]),
        "kocr_crnn_pattern": (ci, [vp, vp, ci, vp, vp, vp, vp, ci]),
        "kocr_recognize_boxes_patterns": (ci, [vp, vp, ci, ci, ci, vp, vp, vp, ci, vp]),
        "kocr_crnn_decode_logits_patterns": (ci, [vp, vp, ci, vp, vp, vp, vp]),
        "kocr_set_orientation": (ci, [vp, ci, ctypes.c_double]),
        "kocr_get_orientation": (ci, [vp, vp, vp]),
        "kocr_recognition_orientation": (ci, [vp, vp, vp, vp, ci, vp]),
        "kocr_warp_crops_turned": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, ctypes.c_double, ci, ci, vp, vp, vp]),
        "kocr_orient_select": (ci, [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "kocr_recognize_boxes_windowed": (ci, [vp, vp, ci, ci, ci, vp, vp, ctypes.c_double, ci, ci]),
        "kocr_windowed_results_shape": (ci, [vp, vp, vp]),
        "kocr_windowed_results": (ci, [vp, vp, vp, vp, vp, vp, ci, ci]),
        "kocr_window_plan": (ci, [vp, ci, vp, ctypes.c_double, ci, vp, vp, vp, ci, vp]),
        "kocr_warp_crops_windowed": (ci, [vp, vp, ci, ci, ci, vp, vp, ctypes.c_double, ci, vp, vp, vp, vp, ci, vp]),
        "kocr_ctc_stitch_decode": (ci, [vp, vp, ci, vp, ci, vp, vp, vp, vp, ci]),
        "kocr_set_scores": (ci, [vp, ci]),
        "kocr_get_scores": (ci, [vp]),
        "kocr_detection_scores": (ci, [vp, vp, ci]),
        "kocr_recognition_scores": (ci, [vp, vp, vp, ci, vp, vp]),
        "kocr_crnn_classes": (ci, [vp]),
        "kocr_crnn_label_width": (ci, [vp]),
        "kocr_crnn_set_rnn_steps_to_discard": (ci, [vp, ci]),
        "kocr_ctc_batch_cost": (ci, [vp, vp, ci, ci, ci, vp, ci, vp, vp, vp, ci]),
        "kocr_crnn_ctc_loss": (ci, [vp, vp, ci, vp, ci, vp, vp, vp, ci]),
        "kocr_crnn_features": (ci, [vp, vp, ci, vp, ci]),
        "kocr_crnn_decode_logits": (ci, [vp, vp, ci, vp, vp, vp, vp, ci, ci, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, vp]),
        "kocr_compute_maps": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, ci, vp, vp, vp, ci]),
        "kocr_heat_mse": (ci, [vp, vp, vp, ci, ci, ci, vp, ci]),
        "kocr_craft_mse": (ci, [vp, vp, ci, ci, ci, ci, vp, ci, vp, ci]),
        "kocr_iou_table": (ci, [vp, ci, vp, vp, vp, vp, vp, ctypes.c_int64, vp, ci]),
        "kocr_score": (ci, [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp, vp,
                            ctypes.c_int64, vp, ci]),
        "kocr_group_lines": (ci, [vp, ci, vp, vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, vp, vp, vp, vp,
                                  ctypes.c_int64, vp, ci]),
        "kocr_char_boxes": (ci, [vp, vp, ci, ci, ci, vp, vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, vp, vp, vp, ctypes.c_int64,
                                 vp, ci, ci]),
        "kocr_set_char_boxes": (ci, [vp, ci, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
        "kocr_get_char_boxes": (ci, [vp, vp, vp, vp, vp]),
        "kocr_detection_char_boxes": (ci, [vp, vp, vp, vp, ci, ctypes.c_int64, vp]),
        "kocr_get_boxes": (ci, [vp, vp, ci, ci, ci, ctypes.c_float, ctypes.c_float, ctypes.c_float, ci, vp, vp, ci, ci]),
        "kocr_warp_crops": (ci, [vp, vp, ci, ci, ci, vp, vp, ci, ci, vp, ci]),
        "kocr_warp_quads": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp]),
        "kocr_detect": (ci, [vp, vp, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, ctypes.c_float, ci, ci, vp, vp, ci, ci]),
        "kocr_recognize_boxes": (ci, [vp, vp, ci, ci, ci, vp, vp, vp, ci]),
        "kocr_resize_pad": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp, ci]),
        "kocr_pipeline": (ci, [vp, ci, ctypes.POINTER(vp), _c_int_p, _c_int_p, _c_int_p, _c_int_p, ci, ci,
                               ctypes.c_float, ctypes.c_float, ctypes.c_float, ci, ci, vp, vp, ci, vp, ci, vp, ci]),
        "kocr_pipeline_device_results": (ci, [vp, vp, vp, vp, vp, vp, vp]),
        "kocr_tile_plan": (ci, [vp, ci, ci, ci, ci, vp]),
        "kocr_gather_tiles": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, ci]),
        "kocr_stitch_heat": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, ci]),
        "kocr_craft_forward_tiled": (ci, [vp, vp, ci, ci, ci, ci, ci, vp, ci, ci]),
        "kocr_detect_tiled": (ci, [vp, vp, ci, ci, ci, ci, ci, ctypes.c_float, ctypes.c_float, ctypes.c_float, ci, ci, vp, vp, ci, ci]),
        "kocr_pipeline_tiled": (ci, [vp, ci, ctypes.POINTER(vp), _c_int_p, _c_int_p, _c_int_p, _c_int_p, ci, ci,
                                     ctypes.c_float, ctypes.c_float, ctypes.c_float, ci, ci, vp, vp, ci, vp, ci, vp, ci]),
        "kocr_pipeline_results": (ci, [vp, vp, ci, vp, ci]),
        "kocr_pipeline_results_shape": (ci, [vp, vp, vp]),
        "kocr_resize_pad_f32": (ci, [vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, ctypes.c_float, vp]),
        "kocr_warp_crops_f32": (ci, [vp, vp, ci, ci, ci, ci, vp, vp, ci, ci, vp]),
        "kocr_conv2d_nhwc": (ci, [vp, vp, ci, ci, ci, ci, vp, ci, ci, ci, ci, vp, vp, ci, vp, vp, vp]),
        "kocr_conv2d_cells": (ci, [vp, vp, ci, ci, ci, ci, vp, ci, vp, vp, ci, vp, vp, ci, ci, ci, vp, vp, vp]),
        "kocr_set_split_mode": (ci, [vp, ci]),
        "kocr_get_split_mode": (ci, [vp]),
        "kocr_set_schedule": (ci, [vp, ci, ci]),
        "kocr_get_schedule": (ci, [vp, _c_int_p, _c_int_p]),
        "kocr_set_min_area_rect": (ci, [vp, ci]),
        "kocr_get_min_area_rect": (ci, [vp]),
        "kocr_profile_enable": (ci, [vp, ci]),
        "kocr_profile_reset": (ci, [vp]),
        "kocr_profile_report": (ci, [vp, ci, ctypes.c_char_p, _c_i64_p, _c_dbl_p, _c_dbl_p, _c_dbl_p]),
        "kocr_range_stats_enable": (ci, [vp, ci]),
        "kocr_range_stats_report": (ci, [vp, ci, ctypes.c_char_p, _c_dbl_p]),
        "kocr_debug_arena_count": (ci, []),
        "kocr_debug_arena_name": (ctypes.c_char_p, [ci]),
        "kocr_debug_arena_stats": (ci, [vp, ci, vp, vp, vp, vp]),
        "kocr_debug_memory_stats": (ci, [vp, vp, vp, vp, vp, vp]),
        "kocr_debug_release_arenas": (ci, [vp]),
        "kocr_debug_set_arena_guards": (ci, [vp, ci]),
        "kocr_debug_check_arena_guards": (ci, [vp, vp, vp, vp]),
        "kocr_debug_set_arena_poison": (ci, [vp, ci]),
    }
    for name, (res, args) in sigs.items():
        if not hasattr(lib, name):
            continue  # entry points land incrementally; tests check the header against the .so
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _ptr(a):
    """Host numpy array / device pointer int / None -> c_void_p."""
    if a is None:
        return ctypes.c_void_p(0)
    if isinstance(a, (int, np.integer)):
        return ctypes.c_void_p(int(a))
    return ctypes.c_void_p(a.ctypes.data)


CHAR_RULE_DEFAULTS = {"peak_threshold": 0.4, "valley_ratio": 0.7, "extent_threshold": 0.2}


def char_rule(char_boxes):
    """``char_boxes=True`` or a dict of rule parameters -> the three parameters of include/kocr.h ("characters") as a dict of
    floats, None for a falsy value.  TypeError for an unknown parameter; the library checks the ranges (ValueError)."""
    if not char_boxes and not isinstance(char_boxes, dict):
        return None
    given = {} if char_boxes is True else dict(char_boxes)
    unknown = set(given) - set(CHAR_RULE_DEFAULTS)
    if unknown:
        raise TypeError(f"char_boxes: unknown rule parameter(s) {sorted(unknown)}")
    return {k: float(given.get(k, d)) for k, d in CHAR_RULE_DEFAULTS.items()}


def _char_lists(counts, quads, scores):
    """per image an array of per-word character counts + the packed quads and scores -> per image a list of one
    ``(quads (K, 4, 2), scores (K,))`` pair per word"""
    pages, at = [], 0
    for page in counts:
        words = []
        for k in np.asarray(page).tolist():
            words.append((quads[at:at + k].copy(), scores[at:at + k].copy()))
            at += k
        pages.append(words)
    return pages


def beam_args(beam_width, top_paths=1):
    """(beam_width, top_paths) as ints, or ValueError naming the argument: 1 <= beam_width <= 64, 1 <= top_paths <=
    beam_width (include/kocr.h: "Beam search"; the library checks the same)."""
    bw, k = int(beam_width), int(top_paths)
    if not 1 <= bw <= 64:
        raise ValueError(f"beam_width {bw} outside [1, 64]")
    if not 1 <= k <= bw:
        raise ValueError(f"top_paths {k} outside [1, beam_width = {bw}]")
    return bw, k


# orientation modes (include/kocr.h: KOCR_ORIENT_FLIP / KOCR_ORIENT_ANY; 0 is off)
ORIENTATION_MODES = {"flip": 1, "any": 2}


def orientation_args(orientation, tall_ratio=1.5):
    """(mode code, tall_ratio) from ``orientation`` = "flip" / "any" and ``tall_ratio``, or ValueError naming the argument:
    tall_ratio must be finite and positive (include/kocr.h: "orientation"; the library checks the same)."""
    if not isinstance(orientation, str) or orientation not in ORIENTATION_MODES:
        raise ValueError(f"orientation must be one of {sorted(ORIENTATION_MODES)}, got {orientation!r}")
    ratio = float(tall_ratio)
    if not (math.isfinite(ratio) and ratio > 0):
        raise ValueError(f"tall_ratio {tall_ratio!r} must be finite and positive")
    return ORIENTATION_MODES[orientation], ratio


def debug_process_memory():
    """{process_count, process_bytes}: the device allocations the library holds in this process, over all contexts
    (kocr_debug_memory_stats without a context; for tests).  Touches no device."""
    v = [ctypes.c_uint64(0) for _ in range(2)]
    load_library().kocr_debug_memory_stats(None, None, None, None, ctypes.byref(v[0]), ctypes.byref(v[1]))
    return {"process_count": int(v[0].value), "process_bytes": int(v[1].value)}


class Context:
    """One kocr_ctx: one HIP device, one stream, weights + workspace."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = ctypes.c_void_p()
        rc = self._lib.kocr_create(ctypes.byref(h), int(device))
        if rc != 0:
            raise KocrError(
                f"kocr_create(device={device}) failed with code {rc}: no usable HIP device. "
                "keras-ocr_amd runs only on an AMD GPU (gfx950); there is no CPU fallback.")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.kocr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # pragma: no cover
            pass

    def _check(self, rc, value_error=False):
        """rc, or the exception the reference raises where the call failed: IndexError on an empty contour list
        (detection.py:272), ZeroDivisionError on a box without width or height (tools.py:95), ValueError for a refused
        argument (KOCR_EINVAL) when ``value_error`` (the reference / TF raise one there), KocrError otherwise."""
        if rc >= 0:
            return rc
        if rc == KOCR_EEMPTYCONTOUR:
            raise IndexError("list index out of range")
        if rc == KOCR_EZERODIV:
            raise ZeroDivisionError("division by zero")
        msg = self._lib.kocr_last_error(self._h).decode("utf-8", "replace")
        if value_error and rc == KOCR_EINVAL:
            raise ValueError(msg)
        raise KocrError(f"libkocr error {rc}: {msg}")

    # -- plumbing ------------------------------------------------------------------
    def set_stream(self, stream_ptr):
        """Run this context on the caller's HIP stream (kocr_set_stream), e.g. ``torch.cuda.Stream().cuda_stream``; the
        stream it was on is synchronised first.  ``0`` / ``None`` selects the context's own non-blocking stream -- and ``0``
        is also the handle of torch's default stream, so ``set_stream(torch.cuda.current_stream().cuda_stream)`` on the
        default stream does NOT put the library there.  The context's own stream is not ordered against the legacy default
        stream: a caller working on the default stream calls ``torch.cuda.synchronize()`` before a device-pointer call and
        ``synchronize()`` after it, or uses a non-default stream."""
        self._check(self._lib.kocr_set_stream(self._h, ctypes.c_void_p(stream_ptr or 0)))

    def synchronize(self):
        self._check(self._lib.kocr_synchronize(self._h))

    def _load(self, fn, weights):
        names = sorted(weights)
        arrs = [np.ascontiguousarray(weights[k], dtype=np.float32) for k in names]
        n = len(names)
        c_names = (ctypes.c_char_p * n)(*[k.encode() for k in names])
        c_data = (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])
        shapes = np.ones((n, 4), dtype=np.int64)
        ranks = np.zeros(n, dtype=np.int32)
        for i, a in enumerate(arrs):
            if a.ndim > 4:
                raise ValueError(f"weight {names[i]} has rank {a.ndim} > 4")
            shapes[i, : a.ndim] = a.shape
            ranks[i] = a.ndim
        self._check(fn(self._h, n, c_names, c_data, shapes.ctypes.data_as(_c_i64_p),
                       ranks.ctypes.data_as(_c_int_p)))

    def load_craft(self, weights):
        self._load(self._lib.kocr_load_craft, weights)

    def load_crnn(self, weights):
        self._load(self._lib.kocr_load_crnn, weights)

    # -- inner seam #1 ---------------------------------------------------------------
    def craft_forward(self, images, micro_batch=0):
        """images: (N,H,W,3) uint8 (raw RGB) or float32 (normalised) numpy array on the host.
        Returns (N,H//2,W//2,2) float32."""
        x, dt = _detector_input(images)
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("images must have shape (N,H,W,3)")
        n, h, w, _ = x.shape
        out = np.empty((n, h // 2, w // 2, 2), dtype=np.float32)
        self._check(self._lib.kocr_craft_forward(self._h, _ptr(x), dt, n, h, w, _ptr(out), int(micro_batch), 0))
        return out

    def craft_forward_device(self, d_img, dtype, n, h, w, d_heat, micro_batch=0):
        """Device-pointer variant (asynchronous on the ctx stream)."""
        self._check(self._lib.kocr_craft_forward(self._h, _ptr(d_img), int(dtype), n, h, w, _ptr(d_heat),
                                                 int(micro_batch), 1))

    def _set_taps(self, fn, names):
        names = [n.encode() for n in names]
        arr = (ctypes.c_char_p * max(1, len(names)))(*names)
        self._check(fn(self._h, len(names), arr))

    def craft_set_taps(self, names=("*",)):
        """Record the named launches of every following craft_forward (include/kocr.h: kocr_craft_set_taps); "*" = all,
        an empty list turns taps off."""
        self._set_taps(self._lib.kocr_craft_set_taps, names)

    def crnn_set_taps(self, names=("*",)):
        """Record the named launches of every following crnn_forward (include/kocr.h: kocr_crnn_set_taps); "*" = all,
        an empty list turns taps off.  Replaces detector taps: one network is recorded at a time."""
        self._set_taps(self._lib.kocr_crnn_set_taps, names)

    def crnn_taps(self):
        """What the last crnn_forward recorded: as craft_taps (cell-grid tensors: one whole cell per crop)."""
        return self.craft_taps()

    def craft_taps(self):
        """What the last craft_forward recorded, in launch order: {name: {"kernel": profiler rows '+'-joined,
        "in" / "out" / "pool": (N x H x W x C float32 array, per-image max-|x| slots or None) or None}}."""
        out = {}
        for i in range(self._check(self._lib.kocr_craft_tap_count(self._h))):
            name = ctypes.create_string_buffer(64)
            kernel = ctypes.create_string_buffer(256)
            dims = np.zeros((3, 4), dtype=np.int32)
            self._check(self._lib.kocr_craft_tap_info(self._h, i, name, kernel, _ptr(dims)))
            rec = {"kernel": kernel.value.decode()}
            for which, key in enumerate(("in", "out", "pool")):
                if not dims[which, 0]:
                    rec[key] = None
                    continue
                data = np.empty(tuple(int(v) for v in dims[which]), dtype=np.float32)
                amax = np.empty(int(dims[which, 0]), dtype=np.float32)
                self._check(self._lib.kocr_craft_get_tap(self._h, name.value, which, _ptr(data), _ptr(amax)))
                rec[key] = (data, None if (amax < 0).any() else amax)
            out[name.value.decode()] = rec
        return out

    # -- inner seam #2 ---------------------------------------------------------------
    def crnn_classes(self):
        return self._check(self._lib.kocr_crnn_classes(self._h))

    def crnn_label_width(self):
        """columns of a label row: 50 time-steps minus rnn_steps_to_discard (48 for the default build)"""
        return self._check(self._lib.kocr_crnn_label_width(self._h))

    def crnn_set_rnn_steps_to_discard(self, steps):
        """build_params["rnn_steps_to_discard"] (recognition.py:328) of the recogniser on this context"""
        self._check(self._lib.kocr_crnn_set_rnn_steps_to_discard(self._h, int(steps)))

    def crnn_forward(self, crops, return_probs=False):
        """crops: (M,31,200[,1]) float32 in [0,1].  Returns labels (M,48) int32 (-1 padded)
        [, probs (M,48,n_classes)] (48 = crnn_label_width())."""
        x = self._crops(crops)
        m = x.shape[0]
        c = self.crnn_classes()
        lw = self.crnn_label_width()
        labels = np.full((m, lw), -1, dtype=np.int32)
        probs = np.zeros((m, lw, c), dtype=np.float32) if return_probs else None
        self._check(self._lib.kocr_crnn_forward(self._h, _ptr(x), m, _ptr(labels), _ptr(probs), 0))
        return (labels, probs) if return_probs else labels

    def crnn_forward_scores(self, crops, return_probs=False):
        """crnn_forward with the recogniser's scores (kocr_crnn_forward_scores, one launch for decode and scores): returns
        labels (M,48) int32, log_word (M,) float32 -- the log-probability of every alignment of the crop's own decode --,
        char_scores (M,48) float32 -- per decoded label the peak probability of its run, 0 behind the decode -- [, probs]."""
        x = self._crops(crops)
        m = x.shape[0]
        c = self.crnn_classes()
        lw = self.crnn_label_width()
        labels = np.full((m, lw), -1, dtype=np.int32)
        log_word = np.zeros(m, dtype=np.float32)
        chars = np.zeros((m, lw), dtype=np.float32)
        probs = np.zeros((m, lw, c), dtype=np.float32) if return_probs else None
        self._check(self._lib.kocr_crnn_forward_scores(self._h, _ptr(x), m, _ptr(labels), _ptr(probs), _ptr(log_word),
                                                       _ptr(chars), 0))
        return (labels, log_word, chars, probs) if return_probs else (labels, log_word, chars)

    def crnn_forward_scores_device(self, d_crops, m, d_labels, d_log_word, d_chars, d_probs=None):
        self._check(self._lib.kocr_crnn_forward_scores(self._h, _ptr(d_crops), int(m), _ptr(d_labels), _ptr(d_probs),
                                                       _ptr(d_log_word), _ptr(d_chars), 1))

    # -- scores (include/kocr.h: "Scores") ---------------------------------------------------------------------------
    def set_scores(self, on=True):
        """Whether get_boxes / detect / recognize_boxes / pipeline leave their scores resident (kocr_set_scores)."""
        self._check(self._lib.kocr_set_scores(self._h, int(bool(on))))

    def get_scores(self):
        return bool(self._check(self._lib.kocr_get_scores(self._h)))

    # -- orientation (include/kocr.h: "orientation") --------------------------------------------------------------------
    def set_orientation(self, mode=0, tall_ratio=1.5):
        """Whether recognize_boxes / pipeline read every box in two orientations and keep the better reading
        (kocr_set_orientation): ``mode`` 0 / None (off), "flip" / 1 (turns 0 and 2) or "any" / 2 (turns 1 and 3 for a box with
        h >= tall_ratio * w).  ValueError for another mode, a tall_ratio that is not finite and positive, or while a beam, a
        lexicon match or character boxes are switched on."""
        code = ORIENTATION_MODES.get(mode, mode) if isinstance(mode, str) else int(mode or 0)
        if isinstance(code, str):
            raise ValueError(f"orientation must be one of {sorted(ORIENTATION_MODES)}, got {mode!r}")
        self._check(self._lib.kocr_set_orientation(self._h, code, float(tall_ratio)), value_error=True)

    def get_orientation(self):
        """``(mode code, tall_ratio)`` (kocr_get_orientation)"""
        mode, ratio = ctypes.c_int(0), ctypes.c_double(0)
        self._check(self._lib.kocr_get_orientation(self._h, ctypes.byref(mode), ctypes.byref(ratio)))
        return mode.value, ratio.value

    def recognition_orientation(self):
        """The resident orientation of the last recognize_boxes / pipeline (kocr_recognition_orientation): turns (M,) int32,
        quads (M, 4, 2) float32 -- [tl, tr, br, bl] of the text as read --, log_words (M, 2) float32, the two candidates'
        word log-probabilities; ValueError when nothing is resident or the results were produced with orientation off."""
        m = ctypes.c_int32(0)
        rc = self._lib.kocr_recognition_orientation(self._h, None, None, None, 0, ctypes.byref(m))
        if rc != KOCR_ECAPACITY:  # KOCR_OK: no crops; anything else: nothing to fetch
            self._check(rc, value_error=True)
        turns, quads, pairs = np.zeros(m.value, np.int32), np.zeros((m.value, 4, 2), np.float32), np.zeros((m.value, 2), np.float32)
        if m.value:
            self._check(self._lib.kocr_recognition_orientation(self._h, _ptr(turns), _ptr(quads), _ptr(pairs), m.value, None),
                        value_error=True)
        return turns, quads, pairs

    def warp_crops_turned(self, images, box_groups, orientation="any", tall_ratio=1.5, target_height=31, target_width=200):
        """The crop stage in both orientations (kocr_warp_crops_turned): images (N,H,W,3) uint8, box_groups a list of
        (n_i,4,2).  Returns crops (2M,th,tw) float32, turns (2M,) int32 and quads (2M,4,2) float32; crop 2m + c is candidate c
        of box m."""
        mode, ratio = orientation_args(orientation, tall_ratio)
        x = np.ascontiguousarray(images, dtype=np.uint8)
        n, h, w, c = x.shape
        if c != 3:
            raise ValueError("images must be RGB")
        counts, flat = _flatten_boxes(box_groups)
        m2 = 2 * int(counts.sum())
        crops = np.zeros((m2, target_height, target_width), dtype=np.float32)
        turns, quads = np.zeros(m2, np.int32), np.zeros((m2, 4, 2), np.float32)
        if m2:
            self._check(self._lib.kocr_warp_crops_turned(self._h, _ptr(x), n, h, w, _ptr(flat), _ptr(counts), mode, ratio,
                                                         int(target_height), int(target_width), _ptr(crops), _ptr(turns), _ptr(quads)),
                        value_error=True)
        return crops, turns, quads

    def orient_select(self, labels, log_word, char_scores, turns=None, quads=None):
        """The choice between two candidates per word (kocr_orient_select): labels (M, 2, L) int32, log_word (M, 2), char_scores
        (M, 2, L) float32 [, turns (M, 2) int32, default (0, 2); quads (M, 2, 4, 2) float32, default zeros].  Returns the
        winners' labels (M, L), log_word (M,), char_scores (M, L), turns (M,), quads (M, 4, 2) and the pairs (M, 2)."""
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.ndim != 3 or lab.shape[1] != 2 or lab.shape[2] < 1:
            raise ValueError(f"labels must have shape (M, 2, L), got {lab.shape}")
        m, _, width = lab.shape
        logw = np.ascontiguousarray(log_word, dtype=np.float32).reshape(m, 2)
        chars = np.ascontiguousarray(char_scores, dtype=np.float32).reshape(m, 2, width)
        turns = np.ascontiguousarray(np.tile(np.array([0, 2], np.int32), (m, 1)) if turns is None else turns, dtype=np.int32).reshape(m, 2)
        quads = np.ascontiguousarray(np.zeros((m, 2, 4, 2), np.float32) if quads is None else quads, dtype=np.float32).reshape(m, 2, 4, 2)
        out = (np.full((m, width), -1, np.int32), np.zeros(m, np.float32), np.zeros((m, width), np.float32), np.zeros(m, np.int32),
               np.zeros((m, 4, 2), np.float32), np.zeros((m, 2), np.float32))
        self._check(self._lib.kocr_orient_select(self._h, m, width, _ptr(lab), _ptr(logw), _ptr(chars), _ptr(turns), _ptr(quads),
                                                 *[_ptr(a) for a in out]), value_error=True)
        return out

    # -- long words (include/kocr_windows.h) --------------------------------------------------------------------------------
    def window_plan(self, boxes, aspect=10.0, overlap=40):
        """The window plan of word boxes, computed on the device (kocr_window_plan): boxes (M,4,2) float32.  Returns windows
        (M,) int32 = K per box, quads (sum K,4,2) float32 = every window's ordered source quad and ranges (sum K,2) int32 =
        the frames [lo, hi) kept of every window's crop, for the context's rnn_steps_to_discard.  ValueError for parameters
        out of range, a box beyond the frame cap or a conflicting switch; ZeroDivisionError for a box without width or height."""
        flat = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 4, 2)
        m = len(flat)
        windows, total = np.ones(m, np.int32), ctypes.c_int32(0)
        rc = self._lib.kocr_window_plan(self._h, m, _ptr(flat), float(aspect), int(overlap), _ptr(windows), None, None, 0,
                                        ctypes.byref(total))
        if rc != KOCR_ECAPACITY:
            self._check(rc, value_error=True)
        quads, ranges = np.zeros((total.value, 4, 2), np.float32), np.zeros((total.value, 2), np.int32)
        if total.value:
            self._check(self._lib.kocr_window_plan(self._h, m, _ptr(flat), float(aspect), int(overlap), _ptr(windows), _ptr(quads),
                                                   _ptr(ranges), total.value, None), value_error=True)
        return windows, quads, ranges

    def warp_crops_windowed(self, images, box_groups, aspect=10.0, overlap=40):
        """The crop stage of the windowed route (kocr_warp_crops_windowed): images (N,H,W,3) uint8, box_groups a list of
        (n_i,4,2).  Returns crops (sum K,31,200) float32 and the plan as ``window_plan`` (image-major box order): window k of
        box m is crop offset(m) + k, offset the exclusive prefix sum of windows."""
        x = np.ascontiguousarray(images, dtype=np.uint8)
        n, h, w, c = x.shape
        if c != 3:
            raise ValueError("images must be RGB")
        counts, flat = _flatten_boxes(box_groups)
        m = int(counts.sum())
        windows, total = np.ones(m, np.int32), ctypes.c_int32(0)

        def call(crops, quads, ranges, cap):
            return self._lib.kocr_warp_crops_windowed(self._h, _ptr(x), n, h, w, _ptr(flat), _ptr(counts), float(aspect), int(overlap),
                                                      _ptr(crops), _ptr(windows), _ptr(quads), _ptr(ranges), cap, ctypes.byref(total))

        rc = call(None, None, None, 0)
        if rc != KOCR_ECAPACITY:
            self._check(rc, value_error=True)
        t = total.value
        crops, quads, ranges = np.zeros((t, 31, 200), np.float32), np.zeros((t, 4, 2), np.float32), np.zeros((t, 2), np.int32)
        if t:
            self._check(call(crops, quads, ranges, t), value_error=True)
        return crops, windows, quads, ranges

    def ctc_stitch_decode(self, logits, windows, overlap=40):
        """Stitch and decode on the caller's logits (kocr_ctc_stitch_decode): logits (sum K,50,C) float32, windows (M,) = K per
        word.  Returns labels (M,L) int32 (-1 padded), log_word (M,), char_scores (M,L) float32 and frames (M,) int32 = T',
        L the longest T' (the recogniser's label width for no words)."""
        from . import tools  # pylint: disable=import-outside-toplevel

        k = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1)
        m = len(k)
        discard = 50 - self.crnn_label_width()
        _, overlap, _ = tools.window_args(200 / 31, overlap, discard)
        if m and int(k.min()) < 1:
            raise ValueError("every word has at least one window")
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        if lg.ndim != 3 or lg.shape[0] != int(k.sum()) or lg.shape[1] != 50 or lg.shape[2] != self.crnn_classes():
            raise ValueError(f"logits must have shape (sum of windows = {int(k.sum())}, 50, {self.crnn_classes()}), got {lg.shape}")
        width = int((k.max() - 1) * ((200 - overlap) // 4) + 50 - discard) if m else self.crnn_label_width()
        labels, logw = np.full((m, width), -1, np.int32), np.zeros(m, np.float32)
        chars, frames = np.zeros((m, width), np.float32), np.zeros(m, np.int32)
        self._check(self._lib.kocr_ctc_stitch_decode(self._h, _ptr(lg), m, _ptr(k), overlap, _ptr(labels), _ptr(logw), _ptr(chars),
                                                     _ptr(frames), width), value_error=True)
        return labels, logw, chars, frames

    def windowed_results(self):
        """The resident rows of the last ``recognize_boxes_windowed`` (kocr_windowed_results_shape / kocr_windowed_results):
        labels (M,L) int32, log_word (M,), char_scores (M,L) float32, frames (M,) and windows (M,) int32; ValueError when
        nothing is resident."""
        m, width = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._lib.kocr_windowed_results_shape(self._h, ctypes.byref(m), ctypes.byref(width)), value_error=True)
        m, width = m.value, width.value
        labels, logw = np.full((m, width), -1, np.int32), np.zeros(m, np.float32)
        chars, frames, windows = np.zeros((m, width), np.float32), np.zeros(m, np.int32), np.zeros(m, np.int32)
        self._check(self._lib.kocr_windowed_results(self._h, _ptr(labels), _ptr(logw), _ptr(chars), _ptr(frames), _ptr(windows), m, width),
                    value_error=True)
        return labels, logw, chars, frames, windows

    def recognize_boxes_windowed(self, images, box_groups, aspect=10.0, overlap=40):
        """Recognizer.recognize_from_boxes with long boxes read in overlapping windows (kocr_recognize_boxes_windowed): images
        (N,H,W,3) uint8, box_groups a list of (n_i,4,2).  Returns ``windowed_results()``: ragged rows of width L = the longest
        sequence of the call (the label width for no boxes).  ValueError for parameters out of range, a box beyond the frame
        cap (naming it) or a switch that cannot be combined with it; ZeroDivisionError for a box without width or height."""
        x = np.ascontiguousarray(images, dtype=np.uint8)
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("images must be (N,H,W,3) RGB")
        n, h, w, _ = x.shape
        counts, flat = _flatten_boxes(box_groups)
        self._check(self._lib.kocr_recognize_boxes_windowed(self._h, _ptr(x), n, h, w, _ptr(flat), _ptr(counts), float(aspect),
                                                            int(overlap), 0), value_error=True)
        return self.windowed_results()

    # -- character boxes (include/kocr.h: "characters") ----------------------------------------------------------------
    def set_char_boxes(self, on=True, peak_threshold=0.4, valley_ratio=0.7, extent_threshold=0.2):
        """Whether get_boxes / detect / pipeline leave the character boxes of their word boxes resident
        (kocr_set_char_boxes); ValueError for a rule parameter out of range."""
        self._check(self._lib.kocr_set_char_boxes(self._h, int(bool(on)), float(peak_threshold), float(valley_ratio),
                                                  float(extent_threshold)), value_error=True)

    def get_char_boxes(self):
        """``(on, {"peak_threshold", "valley_ratio", "extent_threshold"})`` (kocr_get_char_boxes)"""
        on = ctypes.c_int(0)
        p, r, e = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_double(0)
        self._check(self._lib.kocr_get_char_boxes(self._h, ctypes.byref(on), ctypes.byref(p), ctypes.byref(r), ctypes.byref(e)))
        return bool(on.value), {"peak_threshold": p.value, "valley_ratio": r.value, "extent_threshold": e.value}

    def detection_char_boxes(self, counts, cap):
        """The resident character boxes (kocr_detection_char_boxes): per image a list of one ``(quads (K, 4, 2) float32,
        scores (K,) float32)`` pair per word box; ValueError when nothing is resident or the results were produced with
        character boxes off."""
        counts = np.asarray(counts, dtype=np.int32)
        per_word = np.zeros((len(counts), int(cap)), dtype=np.int32)
        chars = ctypes.c_int64(0)
        self._check(self._lib.kocr_detection_char_boxes(self._h, _ptr(per_word), None, None, int(cap), 0, ctypes.byref(chars)),
                    value_error=True)
        quads, scores = np.zeros((chars.value, 4, 2), np.float32), np.zeros(chars.value, np.float32)
        if chars.value:
            self._check(self._lib.kocr_detection_char_boxes(self._h, _ptr(per_word), _ptr(quads), _ptr(scores), int(cap), chars.value,
                                                            ctypes.byref(chars)), value_error=True)
        return _char_lists([per_word[i, :counts[i]] for i in range(len(counts))], quads, scores)

    def char_boxes(self, heat, box_groups, peak_threshold=0.4, valley_ratio=0.7, extent_threshold=0.2):
        """The character boxes of word boxes, read off the detector's region map in one call (kocr_char_boxes; DESIGN.md
        section 4, "Characters"): ``heat`` (N, h, w, 2) float32 heat-maps (host array), ``box_groups`` per image (n_i, 4, 2)
        word boxes [tl, tr, br, bl] in detector-input pixels as ``get_boxes`` returns them.  Returns, per image, a list of one
        ``(quads (K, 4, 2) float32, scores (K,) float32)`` pair per word: the characters from tl towards tr, each a slice of
        the word box at its full height, and the region map's value at each character's peak.  ValueError for a rule
        parameter out of range (all finite, 0 < peak_threshold, 0 <= valley_ratio <= 1, 0 <= extent_threshold <=
        peak_threshold) and for a non-finite coordinate (naming page and word)."""
        y = np.ascontiguousarray(heat, dtype=np.float32)
        if y.ndim != 4 or y.shape[3] != 2:
            raise ValueError("heat must have shape (N,h,w,2)")
        if len(box_groups) != len(y):
            raise ValueError(f"{len(y)} heat-maps but {len(box_groups)} groups of boxes")
        n, h, w, _ = y.shape
        counts, quads = _flatten_boxes(box_groups)
        off = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)]).astype(np.int32)
        per_word = np.zeros(len(quads), np.int32)
        chars = ctypes.c_int64(0)
        rule = (float(peak_threshold), float(valley_ratio), float(extent_threshold))
        cap = max(64, 16 * len(quads))  # a guess; KOCR_ECAPACITY reports the true number
        while True:
            out_q, out_s = np.zeros((cap, 4, 2), np.float32), np.zeros(cap, np.float32)
            rc = self._lib.kocr_char_boxes(self._h, _ptr(y), n, h, w, _ptr(quads), _ptr(off), *rule, _ptr(per_word), _ptr(out_q),
                                           _ptr(out_s), cap, ctypes.byref(chars), 0, 0)
            if rc == KOCR_ECAPACITY and chars.value > cap:
                cap = chars.value
                continue
            self._check(rc, value_error=True)
            return _char_lists([per_word[off[i]:off[i + 1]] for i in range(n)], out_q[:chars.value], out_s[:chars.value])

    def detection_scores(self, counts, cap):
        """The resident detection scores (kocr_detection_scores) as a per-image list of (n_i,) float32 arrays; ValueError
        when nothing is resident or the results were produced with scores off."""
        counts = np.asarray(counts, dtype=np.int32)
        buf = np.zeros((len(counts), int(cap)), dtype=np.float32)
        self._check(self._lib.kocr_detection_scores(self._h, _ptr(buf), int(cap)), value_error=True)
        return [buf[i, :counts[i]].copy() for i in range(len(counts))]

    def recognition_scores(self):
        """The resident recogniser scores (kocr_recognition_scores): log_word (M,) and char_scores (M, label width the rows
        were produced with) float32; ValueError as detection_scores."""
        return self._fetch_resident(self._lib.kocr_recognition_scores, 2, lambda m, lw: (
            np.zeros(m, dtype=np.float32), np.zeros((m, lw), dtype=np.float32)))

    def _fetch_resident(self, fn, n_sizes, allocate):
        """The protocol of the three recognition_* fetchers: a call with null buffers reports the sizes (crops first) with
        KOCR_ECAPACITY; ``allocate(*sizes)`` makes the two arrays; a second call fills them (none for zero crops)."""
        sizes = [ctypes.c_int32(0) for _ in range(n_sizes)]
        rc = fn(self._h, None, None, 0, *[ctypes.byref(v) for v in sizes])
        if rc != KOCR_ECAPACITY:  # KOCR_OK: no crops; anything else: nothing to fetch
            self._check(rc, value_error=True)
        first, second = allocate(*[v.value for v in sizes])
        if sizes[0].value:
            self._check(fn(self._h, _ptr(first), _ptr(second), sizes[0].value, *[None] * n_sizes), value_error=True)
        return first, second

    # -- beam search (include/kocr.h: "Beam search") --------------------------------------------------------------------
    def crnn_beam(self, crops, beam_width, top_paths=1):
        """CTC prefix beam search on the crops' logits (kocr_crnn_beam): labels (M, top_paths, 48) int32, -1 padded, best
        first, and log_prob (M, top_paths) float32 = -crnn_ctc_loss of each row, bit for bit; rows that do not exist are all
        -1 with -inf.  ValueError naming the argument for beam_width outside [1, 64] or top_paths outside [1, beam_width]."""
        bw, k = beam_args(beam_width, top_paths)
        x = self._crops(crops)
        m = x.shape[0]
        labels = np.full((m, k, self.crnn_label_width()), -1, dtype=np.int32)
        log_prob = np.full((m, k), -np.inf, dtype=np.float32)
        self._check(self._lib.kocr_crnn_beam(self._h, _ptr(x), m, bw, k, _ptr(labels), _ptr(log_prob), 0), value_error=True)
        return labels, log_prob

    def crnn_beam_device(self, d_crops, m, beam_width, top_paths, d_labels, d_log_prob):
        self._check(self._lib.kocr_crnn_beam(self._h, _ptr(d_crops), int(m), int(beam_width), int(top_paths), _ptr(d_labels),
                                             _ptr(d_log_prob), 1), value_error=True)

    def set_beam(self, beam_width=0, top_paths=1):
        """Whether recognize_boxes / pipeline also leave beam alternatives resident (kocr_set_beam); 0 = off."""
        self._check(self._lib.kocr_set_beam(self._h, int(beam_width), int(top_paths)), value_error=True)

    def get_beam(self):
        bw, k = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.kocr_get_beam(self._h, ctypes.byref(bw), ctypes.byref(k)))
        return bw.value, k.value

    def recognition_beams(self):
        """The resident beam alternatives (kocr_recognition_beams): labels (M, top_paths, label width) int32 and log_prob
        (M, top_paths) float32 as they were produced; ValueError when nothing is resident or the beam was off."""
        return self._fetch_resident(self._lib.kocr_recognition_beams, 3, lambda m, lw, k: (
            np.full((m, k, lw), -1, dtype=np.int32), np.full((m, k), -np.inf, dtype=np.float32)))

    # -- lexicon (include/kocr.h: "Lexicon") ------------------------------------------------------------------------------
    def set_lexicon(self, labels=None, lengths=None):
        """Load the word list (kocr_set_lexicon): labels (V, stride) int32 rows, lengths (V,); it stays resident like weights.
        ``set_lexicon(None)`` unloads.  ValueError naming the argument and the word for a label outside [0, classes - 2] or a
        length outside [1, 32]."""
        if labels is None or len(labels) == 0:
            self._check(self._lib.kocr_set_lexicon(self._h, None, 0, None, 0), value_error=True)
            return
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.ndim != 2:
            raise ValueError(f"lexicon labels must be (V, stride), got shape {lab.shape}")
        lens = np.ascontiguousarray(lengths, dtype=np.int32).reshape(-1)
        if len(lens) != len(lab):
            raise ValueError(f"lexicon lengths: {len(lens)} entries for {len(lab)} words")
        self._check(self._lib.kocr_set_lexicon(self._h, _ptr(lab), lab.shape[1], _ptr(lens), len(lab)), value_error=True)

    def lexicon_size(self):
        return self._check(self._lib.kocr_lexicon_size(self._h))

    def set_lexicon_scratch(self, nbytes=0):
        """The value scratch one chunk of crops may take (kocr_set_lexicon_scratch); 0: the default.  Results do not depend on it."""
        self._check(self._lib.kocr_set_lexicon_scratch(self._h, int(nbytes)))

    def crnn_lexicon(self, crops, top_words, return_values=False):
        """The crops' best lexicon words (kocr_crnn_lexicon): index (M, top_words) int32 into the loaded word list, best first,
        -1 where fewer words are feasible, and log_prob (M, top_words) float32 = -crnn_ctc_loss of crop and word, bit for bit
        (-inf there) [, the scoring kernel's own values (M, V) float32].  ValueError for top_words outside [1, 64] or without
        a lexicon."""
        x = self._crops(crops)
        m, k = x.shape[0], int(top_words)
        index = np.full((m, max(k, 0)), -1, dtype=np.int32)
        log_prob = np.full((m, max(k, 0)), -np.inf, dtype=np.float32)
        values = np.full((m, self.lexicon_size()), -np.inf, dtype=np.float32) if return_values else None
        self._check(self._lib.kocr_crnn_lexicon(self._h, _ptr(x), m, k, _ptr(index), _ptr(log_prob), _ptr(values), 0), value_error=True)
        return (index, log_prob, values) if return_values else (index, log_prob)

    def crnn_lexicon_device(self, d_crops, m, top_words, d_index, d_log_prob, d_values=None):
        self._check(self._lib.kocr_crnn_lexicon(self._h, _ptr(d_crops), int(m), int(top_words), _ptr(d_index), _ptr(d_log_prob),
                                                _ptr(d_values), 1), value_error=True)

    def set_lexicon_match(self, top_words=0):
        """Whether recognize_boxes / pipeline also leave lexicon matches resident (kocr_set_lexicon_match); 0 = off."""
        self._check(self._lib.kocr_set_lexicon_match(self._h, int(top_words)), value_error=True)

    def get_lexicon_match(self):
        k = ctypes.c_int(0)
        self._check(self._lib.kocr_get_lexicon_match(self._h, ctypes.byref(k)))
        return k.value

    def recognition_lexicon(self):
        """The resident lexicon matches (kocr_recognition_lexicon): index (M, top_words) int32 and log_prob (M, top_words)
        float32 as they were produced; ValueError when nothing is resident or the match was off."""
        return self._fetch_resident(self._lib.kocr_recognition_lexicon, 2, lambda m, k: (
            np.full((m, k), -1, dtype=np.int32), np.full((m, k), -np.inf, dtype=np.float32)))

    # -- character sets (include/kocr.h: "Character sets") ---------------------------------------------------------------
    def set_charsets(self, allowed=None):
        """Load the sets (kocr_set_charsets): allowed (S, classes - 1) of 0 / 1, row s = the non-blank classes of set s; the
        table stays resident like a lexicon.  ``set_charsets(None)`` unloads and switches off.  ValueError naming the set for
        an empty one, for more than 256 sets and for a row length other than ``crnn_classes() - 1``."""
        if allowed is None or len(allowed) == 0:
            self._check(self._lib.kocr_set_charsets(self._h, None, 0, 0), value_error=True)
            return
        a = np.ascontiguousarray(np.asarray(allowed) != 0, dtype=np.uint8)
        if a.ndim != 2:
            raise ValueError(f"charsets must be (S, classes - 1), got shape {a.shape}")
        self._check(self._lib.kocr_set_charsets(self._h, _ptr(a), a.shape[0], a.shape[1] + 1), value_error=True)

    def charset_count(self):
        return self._check(self._lib.kocr_charset_count(self._h))

    def set_charset(self, index=-1):
        """The set every decode of the context runs under (kocr_set_charset); -1 = off."""
        self._check(self._lib.kocr_set_charset(self._h, int(index)), value_error=True)

    def get_charset(self):
        k = ctypes.c_int(0)
        self._check(self._lib.kocr_get_charset(self._h, ctypes.byref(k)))
        return k.value

    def _set_of(self, set_of, m, what):
        """``set_of`` as (m,) int32, or ValueError naming the count"""
        s = np.ascontiguousarray(np.reshape(set_of, -1), dtype=np.int32)
        if s.shape != (m,):
            raise ValueError(f"set_of must hold one character set per {what}: {m}, got {s.shape[0]}")
        return s

    # -- patterns (include/kocr.h: "Patterns") ---------------------------------------------------------------------------
    def set_patterns(self, delta=None, accept=None, n_states=None):
        """Load the automata (kocr_set_patterns; ``patterns.Patterns.tables()``): delta (sum S, classes - 1) int32, accept
        (sum S,) of 0 / 1, n_states (P,); they stay resident like a lexicon.  ``set_patterns(None)`` unloads and switches off.
        ValueError naming the pattern for a refused table."""
        if delta is None or len(delta) == 0:
            self._check(self._lib.kocr_set_patterns(self._h, None, None, None, 0, 0), value_error=True)
            return
        d = np.ascontiguousarray(delta, dtype=np.int32)
        a = np.ascontiguousarray(np.asarray(accept) != 0, dtype=np.uint8).reshape(-1)
        n = np.ascontiguousarray(n_states, dtype=np.int32).reshape(-1)
        if d.ndim != 2 or len(a) != len(d) or int(n.sum()) != len(d):
            raise ValueError(f"patterns: delta {d.shape}, accept {a.shape} and n_states (sum {int(n.sum())}) do not describe the same states")
        self._check(self._lib.kocr_set_patterns(self._h, _ptr(d), _ptr(a), _ptr(n), len(n), d.shape[1] + 1), value_error=True)

    def pattern_count(self):
        return self._check(self._lib.kocr_pattern_count(self._h))

    def set_pattern(self, index=-1):
        """The pattern every crop of recognize_boxes / pipeline is also decoded under (kocr_set_pattern); -1 = off."""
        self._check(self._lib.kocr_set_pattern(self._h, int(index)), value_error=True)

    def get_pattern(self):
        k = ctypes.c_int(0)
        self._check(self._lib.kocr_get_pattern(self._h, ctypes.byref(k)))
        return k.value

    def _pattern_of(self, pattern_of, m, what):
        """``pattern_of`` as (m,) int32, or ValueError naming the count"""
        p = np.ascontiguousarray(np.reshape(pattern_of, -1), dtype=np.int32)
        if p.shape != (m,):
            raise ValueError(f"pattern_of must hold one pattern per {what}: {m}, got {p.shape[0]}")
        return p

    def recognition_patterns(self):
        """The resident pattern decodes (kocr_recognition_patterns): labels (M, label width) int32, log_path (M,) and log_prob
        (M,) float32 as they were produced; ValueError when nothing is resident or the pattern was off."""
        m = ctypes.c_int32(0)
        rc = self._lib.kocr_recognition_patterns(self._h, None, None, None, 0, ctypes.byref(m))
        if rc != KOCR_ECAPACITY:
            self._check(rc, value_error=True)
        labels = np.full((m.value, self.crnn_label_width()), -1, dtype=np.int32)
        log_path, log_prob = np.full(m.value, -np.inf, dtype=np.float32), np.full(m.value, -np.inf, dtype=np.float32)
        if m.value:
            self._check(self._lib.kocr_recognition_patterns(self._h, _ptr(labels), _ptr(log_path), _ptr(log_prob), m.value, None),
                        value_error=True)
        return labels, log_path, log_prob

    def crnn_pattern(self, crops, pattern_of=None):
        """The crops' best readings under their patterns (kocr_crnn_pattern): labels (M, 48) int32, -1 padded; log_path (M,)
        float32, the best accepted alignment; log_prob (M,) float32 = -crnn_ctc_loss of the row, bit for bit; -1 / -inf where
        nothing fits or the crop has no pattern.  ``pattern_of`` (M integers in [-1, pattern_count())); None: the context's
        ``set_pattern`` switch."""
        x = self._crops(crops)
        m = x.shape[0]
        of = None if pattern_of is None else self._pattern_of(pattern_of, m, "crop")
        labels = np.full((m, self.crnn_label_width()), -1, dtype=np.int32)
        log_path, log_prob = np.full(m, -np.inf, dtype=np.float32), np.full(m, -np.inf, dtype=np.float32)
        self._check(self._lib.kocr_crnn_pattern(self._h, _ptr(x), m, _ptr(of), _ptr(labels), _ptr(log_path), _ptr(log_prob), 0),
                    value_error=True)
        return labels, log_path, log_prob

    def crnn_pattern_device(self, d_crops, m, d_labels, d_log_path, d_log_prob, pattern_of=None):
        """``crnn_pattern`` on device buffers; ``pattern_of`` stays a host list"""
        of = None if pattern_of is None else self._pattern_of(pattern_of, int(m), "crop")
        self._check(self._lib.kocr_crnn_pattern(self._h, _ptr(d_crops), int(m), _ptr(of), _ptr(d_labels), _ptr(d_log_path),
                                                _ptr(d_log_prob), 1), value_error=True)

    def crnn_decode_logits_patterns(self, logits, pattern_of=None):
        """The pattern launches on given logits (M, 50, classes) float32 (kocr_crnn_decode_logits_patterns; development):
        ``(labels, log_path, log_prob)`` as ``crnn_pattern``."""
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        if lg.ndim != 3 or lg.shape[1:] != (50, self.crnn_classes()):
            raise ValueError(f"logits must be (M, 50, {self.crnn_classes()}), got {lg.shape}")
        m = lg.shape[0]
        of = None if pattern_of is None else self._pattern_of(pattern_of, m, "crop")
        labels = np.full((m, self.crnn_label_width()), -1, dtype=np.int32)
        log_path, log_prob = np.full(m, -np.inf, dtype=np.float32), np.full(m, -np.inf, dtype=np.float32)
        self._check(self._lib.kocr_crnn_decode_logits_patterns(self._h, _ptr(lg), m, _ptr(of), _ptr(labels), _ptr(log_path),
                                                               _ptr(log_prob)), value_error=True)
        return labels, log_path, log_prob

    def crnn_forward_device(self, d_crops, m, d_labels, d_probs=None):
        self._check(self._lib.kocr_crnn_forward(self._h, _ptr(d_crops), int(m), _ptr(d_labels), _ptr(d_probs), 1))

    # -- recognizer.backbone / training_model (recognition.py:319-349) ------------------------------------------------
    @staticmethod
    def _ctc_host_args(labels, label_lengths, input_lengths, m):
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.ndim != 2 or lab.shape[0] != m:
            raise ValueError(f"labels must have shape (M, Lmax) with M = {m}, got {lab.shape}")
        ll = np.ascontiguousarray(np.reshape(label_lengths, -1), dtype=np.int32)
        il = np.ascontiguousarray(np.reshape(input_lengths, -1), dtype=np.int32)
        if ll.shape != (m,) or il.shape != (m,):
            raise ValueError(f"label_lengths and input_lengths must hold M = {m} values")
        return lab, ll, il

    def ctc_batch_cost(self, y_pred, labels, label_lengths, input_lengths):
        """keras.backend.ctc_batch_cost on the GPU (kocr_ctc_batch_cost).  y_pred (M,T,C) float32 probabilities, labels (M,Lmax)
        integer classes (entries from label_lengths[m] on are ignored), label_lengths / input_lengths M integers.  Returns the
        per-sample loss (M,) float32.  A refused argument raises ValueError naming the sample."""
        y = np.ascontiguousarray(y_pred, dtype=np.float32)
        if y.ndim != 3:
            raise ValueError(f"y_pred must have shape (M, T, C), got {y.shape}")
        m, t, c = y.shape
        lab, ll, il = self._ctc_host_args(labels, label_lengths, input_lengths, m)
        loss = np.zeros(m, np.float32)
        self._check(self._lib.kocr_ctc_batch_cost(self._h, _ptr(y), m, t, c, _ptr(lab), lab.shape[1], _ptr(ll), _ptr(il),
                                                  _ptr(loss), 0), value_error=True)
        return loss

    def crnn_ctc_loss(self, crops, labels, label_lengths, input_lengths):
        """training_model.predict (kocr_crnn_ctc_loss): crops (M,31,200[,1]) float32 in [0,1], labels / lengths as
        ctc_batch_cost with T = crnn_label_width().  Returns the per-sample loss (M,) float32."""
        x = self._crops(crops)
        m = x.shape[0]
        lab, ll, il = self._ctc_host_args(labels, label_lengths, input_lengths, m)
        loss = np.zeros(m, np.float32)
        self._check(self._lib.kocr_crnn_ctc_loss(self._h, _ptr(x), m, _ptr(lab), lab.shape[1], _ptr(ll), _ptr(il), _ptr(loss), 0),
                    value_error=True)
        return loss

    def crnn_decode_logits(self, logits, return_probs=False, scores=False, beam=None, top_words=0, return_values=False,
                           loss_labels=None, set_of=None):
        """Development entry (kocr_crnn_decode_logits): the launches behind fc_12 on the caller's logits (M, 50, classes)
        float32, M <= 1024.  Returns a dict: "labels" (M, LW) int32 [, "probs" (M, LW, C)] as crnn_forward; with ``scores``
        "log_word" (M,) and "chars" (M, LW) as crnn_forward_scores; with ``beam=(beam_width, top_paths)`` "beam_labels" /
        "beam_log_prob" as crnn_beam; with ``top_words`` "lex_index" / "lex_log_prob" [, "lex_values"] as crnn_lexicon; with
        ``loss_labels=(labels, label_lengths, input_lengths)`` "loss" (M,) as crnn_ctc_loss.  Refusals as those calls.
        ``set_of`` (M integers in [-1, charset_count())): each crop's character set (kocr_crnn_decode_logits_charsets), -1 =
        unconstrained; None: the context's ``set_charset`` switch.  The loss is never masked."""
        x = np.ascontiguousarray(logits, dtype=np.float32)
        c, lw = self.crnn_classes(), self.crnn_label_width()
        if x.ndim != 3 or x.shape[1:] != (50, c):
            raise ValueError(f"logits must have shape (M, 50, {c}), got {x.shape}")
        m = x.shape[0]
        out = {"labels": np.full((m, lw), -1, dtype=np.int32)}
        if return_probs:
            out["probs"] = np.zeros((m, lw, c), np.float32)
        if scores:
            out["log_word"] = np.zeros(m, np.float32)
            out["chars"] = np.zeros((m, lw), np.float32)
        bw, k = beam_args(*beam) if beam is not None else (0, 1)
        if bw:
            out["beam_labels"] = np.full((m, k, lw), -1, dtype=np.int32)
            out["beam_log_prob"] = np.full((m, k), -np.inf, dtype=np.float32)
        tw = int(top_words or 0)
        if tw:
            out["lex_index"] = np.full((m, max(tw, 0)), -1, dtype=np.int32)
            out["lex_log_prob"] = np.full((m, max(tw, 0)), -np.inf, dtype=np.float32)
            if return_values:
                out["lex_values"] = np.full((m, self.lexicon_size()), -np.inf, dtype=np.float32)
        lab = ll = il = None
        stride = 0
        if loss_labels is not None:
            lab, ll, il = self._ctc_host_args(*loss_labels, m)
            stride = lab.shape[1]
            out["loss"] = np.zeros(m, np.float32)
        g = out.get
        args = (self._h, _ptr(x), m, _ptr(out["labels"]), _ptr(g("probs")), _ptr(g("log_word")), _ptr(g("chars")), bw, k,
                _ptr(g("beam_labels")), _ptr(g("beam_log_prob")), tw, _ptr(g("lex_index")), _ptr(g("lex_log_prob")), _ptr(g("lex_values")),
                _ptr(lab), stride, _ptr(ll), _ptr(il), _ptr(g("loss")))
        if set_of is None:
            self._check(self._lib.kocr_crnn_decode_logits(*args), value_error=True)
        else:
            sets = self._set_of(set_of, m, "crop")
            self._check(self._lib.kocr_crnn_decode_logits_charsets(*args, _ptr(sets)), value_error=True)
        return out

    def crnn_features(self, crops):
        """backbone.predict (kocr_crnn_features): crops (M,31,200[,1]) -> the BiLSTM features (M,50,256) float32."""
        x = self._crops(crops)
        feats = np.zeros((x.shape[0], 50, 256), np.float32)
        self._check(self._lib.kocr_crnn_features(self._h, _ptr(x), x.shape[0], _ptr(feats), 0))
        return feats

    @staticmethod
    def _crops(crops):
        x = np.ascontiguousarray(crops, dtype=np.float32)
        if x.ndim == 4 and x.shape[-1] == 1:
            x = x[..., 0]
        if x.ndim != 3 or x.shape[1:] != (31, 200):
            raise ValueError("crops must have shape (M,31,200[,1])")
        return np.ascontiguousarray(x)

    # -- detection.getBoxes ----------------------------------------------------------------
    def get_boxes(self, heat, detection_threshold=0.7, text_threshold=0.4, link_threshold=0.4,
                  size_threshold=10, cap=None, min_area_rect=None, return_scores=False, char_boxes=None):
        """heat: (N,h,w,2) float32 host array -> list of (n_i,4,2) float32 arrays
        (``np.array([])`` for an image without boxes, detection.py:286).  ``min_area_rect``: ``"exact"`` /
        ``"opencv"`` for this call only, ``None`` = the context's rule (``set_min_area_rect``).  ``return_scores``:
        ``(boxes, scores)``, scores a list of (n_i,) float32 arrays -- each box's detection score, the maximum of the text map
        over its component.  ``char_boxes`` (True, or a dict of ``char_boxes``' rule parameters): a last element, per image a
        list of one ``(quads (K,4,2), scores (K,))`` pair per box -- its characters as ``char_boxes`` gives them, computed in
        the same call on the heat-maps in HBM."""
        y = np.ascontiguousarray(heat, dtype=np.float32)
        if y.ndim != 4 or y.shape[3] != 2:
            raise ValueError("heat must have shape (N,h,w,2)")
        return self._get_boxes(y, detection_threshold, text_threshold, link_threshold, size_threshold, cap, min_area_rect,
                               return_scores, char_boxes).render_detection()

    def _get_boxes(self, y, detection_threshold, text_threshold, link_threshold, size_threshold, cap, min_area_rect=None,
                   return_scores=False, char_boxes=None):
        n, h, w, _ = y.shape
        return self._boxes_grow_cap(n, cap, lambda boxes, counts, cap: self._lib.kocr_get_boxes(
            self._h, _ptr(y), n, h, w, float(detection_threshold), float(text_threshold), float(link_threshold),
            int(size_threshold), _ptr(boxes), _ptr(counts), cap, 0), min_area_rect, return_scores, char_boxes)

    def _boxes_grow_cap(self, n, cap, call, min_area_rect=None, return_scores=False, char_boxes=None):
        """call(boxes, counts, cap) -> rc into (n, cap) buffers, under the per-call switches, repeated with the true maximum
        on KOCR_ECAPACITY (the counts hold it): a ``Results`` of the boxes [, the resident detection scores of the call that
        succeeded] [, its resident character boxes]"""
        cap = int(cap) if cap else 1024
        extras = Extras(min_area_rect=min_area_rect, scores=return_scores, char_boxes=char_rule(char_boxes))
        with self._extras_scope(extras):
            while True:
                boxes = np.zeros((n, cap, 4, 2), dtype=np.float32)
                counts = np.zeros(n, dtype=np.int32)
                rc = call(boxes, counts, cap)
                if rc == KOCR_ECAPACITY and n and counts.max() > cap:
                    cap = int(counts.max())
                    continue
                self._check(rc)
                return self._fetch_extras(Results(_box_lists(boxes, counts), None), extras, n, counts, cap)

    # -- the per-call extras: one scope over the switches, one fetch of what they left resident ----------------------------
    @contextlib.contextmanager
    def _extras_scope(self, extras):
        """The context's switches for one call: every field of ``extras`` (an ``extras.Extras``) that asks for something sets
        its switch, in the order of ``_SWITCHES``, and the old settings come back in reverse -- also when a later setter
        raises.  A field that asks for nothing makes no call at all: the context's own setting holds."""
        with contextlib.ExitStack() as stack:
            for field, value_of, get, set_, restore in _SWITCHES:
                value = value_of(getattr(extras, field))
                if value is not None:
                    old = get(self)
                    set_(self, value)
                    stack.callback(restore or set_, self, old)
            yield

    def _fetch_extras(self, out, extras, n, counts=None, cap=None):
        """``out`` with what the call left resident for ``extras``, or the empty values when nothing ran (``n`` == 0: no
        images, or no crops for a call on boxes).  ``counts`` / ``cap`` (of a call that ran the detector): the boxes per image
        and the capacity they were produced with; scores have a recogniser part where ``out`` has labels."""
        if extras.scores:
            detection = None if counts is None else self.detection_scores(counts, cap) if n else []
            recognition = (None, None) if out.labels is None else self.recognition_scores() if n else empty_scores(self.crnn_label_width())[1:]
            out.scores = (detection, *recognition)
        if extras.beam is not None:
            out.beam = self.recognition_beams() if n else empty_beam(extras.beam[1], self.crnn_label_width())
        if extras.lexicon_top is not None:
            out.lexicon = self.recognition_lexicon() if n else empty_lexicon(extras.lexicon_top)
        if extras.orientation is not None:
            out.orientation = self.recognition_orientation() if n else empty_orientation()
        if extras.patterned:
            out.pattern = self.recognition_patterns() if n else empty_pattern(self.crnn_label_width())
        if extras.characters:
            out.characters = self.detection_char_boxes(counts, cap) if n else []
        return out

    # -- Detector.detect, device-resident heat-maps -----------------------------------------------
    def detect(self, images, detection_threshold=0.7, text_threshold=0.4, link_threshold=0.4, size_threshold=10,
               micro_batch=0, cap=None, min_area_rect=None, return_scores=False, char_boxes=None):
        """images: (N,H,W,3) uint8 (raw RGB) or float32 (normalised).  Returns list of (n_i,4,2) boxes.
        ``min_area_rect``, ``return_scores``, ``char_boxes``: as ``get_boxes``."""
        return self._detect(images, detection_threshold, text_threshold, link_threshold, size_threshold, micro_batch, cap,
                            min_area_rect, return_scores, char_boxes).render_detection()

    def _detect(self, images, detection_threshold, text_threshold, link_threshold, size_threshold, micro_batch, cap,
                min_area_rect=None, return_scores=False, char_boxes=None):
        """detect's ``Results``"""
        x, dt = _detector_input(images)
        n, h, w, _ = x.shape
        return self._boxes_grow_cap(n, cap, lambda boxes, counts, cap: self._lib.kocr_detect(
            self._h, _ptr(x), dt, n, h, w, float(detection_threshold), float(text_threshold), float(link_threshold),
            int(size_threshold), int(micro_batch), _ptr(boxes), _ptr(counts), cap, 0), min_area_rect, return_scores, char_boxes)

    # -- Recognizer.recognize_from_boxes, device-resident crops ---------------------------------------
    def recognize_boxes(self, images, box_groups, return_scores=False, beam=None, lexicon_top=None, orientation=None, set_of=None,
                        pattern=None, pattern_of=None):
        """images: (N,H,W,3) uint8; box_groups: list of (n_i,4,2).  Returns labels (M,48) int32 [, log_word (M,), char_scores
        (M,48) float32 as ``crnn_forward_scores``] [, beam labels (M,K,48), beam log_prob (M,K) as ``crnn_beam``, with
        ``beam=(beam_width, top_paths)``; the other results are the same bits] [, lexicon index (M,K), log_prob (M,K) as
        ``crnn_lexicon``, with ``lexicon_top=K``] [, turns (M,), quads (M,4,2), log_words (M,2) as ``recognition_orientation``,
        with ``orientation=(mode, tall_ratio)``: labels and scores are then those of each word's better reading; not
        together with ``beam`` or ``lexicon_top`` (ValueError)].  ``set_of`` (one integer per box, image-major, in
        [-1, charset_count())): each box's character set (kocr_recognize_boxes_charsets), -1 = unconstrained; None: the
        context's ``set_charset`` switch.  ``pattern`` (an index in [0, pattern_count())): every box is also decoded under
        that pattern, or ``pattern_of`` (one integer per box in [-1, pattern_count()), -1 = none:
        kocr_recognize_boxes_patterns); last come pattern labels (M,48), log_path (M,), log_prob (M,) as ``crnn_pattern``.
        Not together with ``orientation`` or ``set_of`` (ValueError)."""
        return self._recognize_boxes(images, box_groups, Extras(
            scores=return_scores, beam=beam, lexicon_top=lexicon_top, orientation=orientation, set_of=set_of, pattern=pattern,
            pattern_of=pattern_of).validate()).render_recognition()

    def _recognize_boxes(self, images, box_groups, extras):
        """recognize_boxes' ``Results`` (no boxes; the detection part of its scores is None) for a validated ``extras.Extras``;
        no library call for zero boxes beyond the switches"""
        x = np.ascontiguousarray(images, dtype=np.uint8)
        n, h, w, _ = x.shape
        counts, flat = _flatten_boxes(box_groups)
        m = int(counts.sum())
        sets = None if extras.set_of is None else self._set_of(extras.set_of, m, "box")
        pats = None if extras.pattern_of is None else self._pattern_of(extras.pattern_of, m, "box")
        with self._extras_scope(extras):
            out = Results(None, np.full((m, self.crnn_label_width()), -1, dtype=np.int32))
            args = (self._h, _ptr(x), n, h, w, _ptr(flat), _ptr(counts), _ptr(out.labels), 0)
            if m and pats is not None:
                self._check(self._lib.kocr_recognize_boxes_patterns(*args, _ptr(pats)), value_error=True)
            elif m and sets is not None and not extras.patterned:
                self._check(self._lib.kocr_recognize_boxes_charsets(*args, _ptr(sets)), value_error=True)
            elif m:
                self._check(self._lib.kocr_recognize_boxes(*args), value_error=extras.patterned)
            return self._fetch_extras(out, extras, m)

    # -- crops --------------------------------------------------------------------------------
    def warp_crops(self, images, box_groups, target_height=31, target_width=200):
        """images: (N,H,W,3) uint8; box_groups: list of (n_i,4,2).  Returns (M,th,tw) float32."""
        x = np.ascontiguousarray(images, dtype=np.uint8)
        n, h, w, c = x.shape
        if c != 3:
            raise ValueError("images must be RGB")
        counts, flat = _flatten_boxes(box_groups)
        out = np.zeros((int(counts.sum()), target_height, target_width), dtype=np.float32)
        if len(out):
            self._check(self._lib.kocr_warp_crops(self._h, _ptr(x), n, h, w, _ptr(flat), _ptr(counts), int(target_height),
                                                  int(target_width), _ptr(out), 0))
        return out

    def warp_quads(self, images, src_quads, dst_quads, image_index, crop_wh, target_height, target_width,
                   return_transforms=False):
        """General tools.warpBox: images (N,H,W,3) uint8; src_quads / dst_quads (M,4,2) float32 (source already
        ordered tl,tr,br,bl); crop_wh (M,2) = the warp's dsize.  Returns crops (M,th,tw) float32 gray/255
        [, transforms (M,3,3) float64]."""
        x = np.ascontiguousarray(images, dtype=np.uint8)
        n, h, w, c = x.shape
        if c != 3:
            raise ValueError("images must be RGB")
        src = np.ascontiguousarray(src_quads, dtype=np.float32).reshape(-1, 4, 2)
        dst = np.ascontiguousarray(dst_quads, dtype=np.float32).reshape(-1, 4, 2)
        m = len(src)
        idx = np.ascontiguousarray(image_index, dtype=np.int32).reshape(m)
        wh = np.asarray(crop_wh, dtype=np.int64).reshape(m, 2)
        cw = np.ascontiguousarray(np.minimum(wh[:, 0], target_width), dtype=np.int32)
        chh = np.ascontiguousarray(np.minimum(wh[:, 1], target_height), dtype=np.int32)
        out = np.zeros((m, target_height, target_width), dtype=np.float32)
        tf = np.zeros((m, 3, 3), dtype=np.float64) if return_transforms else None
        self._check(self._lib.kocr_warp_quads(self._h, _ptr(x), n, h, w, m, _ptr(src), _ptr(dst), _ptr(idx), _ptr(cw),
                                              _ptr(chh), int(target_height), int(target_width), _ptr(out), _ptr(tf)))
        return (out, tf) if return_transforms else out

    # -- tools.resize_image + pad --------------------------------------------------------------
    def resize_pad(self, images, dsize, out_hw=None, cval=255):
        """images: (n,sh,sw,3) uint8; dsize=(dw,dh) as cv2.resize; out_hw=(Hmax,Wmax) canvas."""
        x = np.ascontiguousarray(images, dtype=np.uint8)
        n, sh, sw, c = x.shape
        if c != 3:
            raise ValueError("images must be RGB")
        dw, dh = int(dsize[0]), int(dsize[1])
        hmax, wmax = (dh, dw) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        out = np.empty((n, hmax, wmax, 3), dtype=np.uint8)
        self._check(self._lib.kocr_resize_pad(self._h, _ptr(x), n, sh, sw, dh, dw, hmax, wmax, int(cval), _ptr(out), 0))
        return out

    def resize_pad_f32(self, images, dsize, out_hw=None, cval=255.0):
        """float images: (n,sh,sw,c) float32; dsize=(dw,dh) as cv2.resize (bilinear, in float); out_hw=(Hmax,Wmax) canvas."""
        x = np.ascontiguousarray(images, dtype=np.float32)
        n, sh, sw, c = x.shape
        dw, dh = int(dsize[0]), int(dsize[1])
        hmax, wmax = (dh, dw) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
        out = np.empty((n, hmax, wmax, c), dtype=np.float32)
        self._check(self._lib.kocr_resize_pad_f32(self._h, _ptr(x), n, sh, sw, c, dh, dw, hmax, wmax, float(cval), _ptr(out)))
        return out

    def warp_crops_f32(self, images, box_groups, target_height=31, target_width=200):
        """float images: (N,H,W,3 or 1) float32; box_groups: list of (n_i,4,2).  Returns (M,th,tw) float32 gray crops in the
        image's own value range (NOT divided by 255)."""
        x = np.ascontiguousarray(images, dtype=np.float32)
        n, h, w, c = x.shape
        if c not in (1, 3):
            raise ValueError("images must be RGB or gray")
        counts, flat = _flatten_boxes(box_groups)
        out = np.zeros((int(counts.sum()), target_height, target_width), dtype=np.float32)
        if len(out):
            self._check(self._lib.kocr_warp_crops_f32(self._h, _ptr(x), n, h, w, c, _ptr(flat), _ptr(counts), int(target_height),
                                                      int(target_width), _ptr(out)))
        return out

    # -- fused Pipeline.recognize ----------------------------------------------------------------
    def pipeline(self, ptrs, hs, ws, dhs, dws, hmax, wmax, detection_threshold=0.7, text_threshold=0.4,
                 link_threshold=0.4, size_threshold=10, micro_batch=0, on_device=False, cap=256, max_crops=None,
                 min_area_rect=None, return_scores=False, beam=None, lexicon_top=None, char_boxes=None, orientation=None,
                 tiled=False, pattern=None):
        """ptrs: per-image source pointers (ints) or host uint8 arrays.  Returns ``Results.render_context()``: (boxes
        list[(n_i,4,2) f32, detector-input px], labels (M,48) int32), then one element per extra asked for, as the fields of
        ``results.Results`` describe them -- ``return_scores``: its ``scores``; ``beam=(beam_width, top_paths)``: its ``beam``,
        or ``lexicon_top=K``: its ``lexicon`` (boxes, labels and scores are the same bits); ``char_boxes`` (True or a dict of
        rule parameters): its ``characters`` (detector-input px).  ``min_area_rect``: as ``get_boxes``.
        ``orientation=(mode, tall_ratio)``, mode "flip" / "any": every box is read in two orientations (include/kocr.h:
        "orientation"); labels and scores are those of each word's better reading, the boxes stay getBoxes' bits, and its
        ``orientation`` comes last (quads in detector-input px).  Not together with ``beam``, ``lexicon_top`` or ``char_boxes``
        (ValueError).  ``tiled`` (``pipeline_tiled``): ``hmax`` / ``wmax`` are the tile and the overlap of kocr_pipeline_tiled.
        ``pattern`` (an index in [0, pattern_count())): every crop is also decoded under that pattern (include/kocr.h:
        "Patterns") and its ``pattern`` comes last of all; not together with ``orientation`` (ValueError)."""
        extras = Extras(char_boxes=char_rule(char_boxes), min_area_rect=min_area_rect, scores=return_scores, beam=beam,
                        lexicon_top=lexicon_top, orientation=orientation, pattern=pattern).validate()
        with self._extras_scope(extras):
            out = self._pipeline(ptrs, hs, ws, dhs, dws, hmax, wmax, detection_threshold, text_threshold, link_threshold,
                                 size_threshold, micro_batch, on_device, cap, max_crops, tiled=tiled)
            # the boxes' own counts and the cap they were produced with (the largest count after a capacity overflow)
            counts = [len(b) for b in out.boxes]
            return self._fetch_extras(out, extras, len(ptrs), counts, max([int(cap)] + counts)).render_context()

    def _pipeline(self, ptrs, hs, ws, dhs, dws, hmax, wmax, detection_threshold, text_threshold, link_threshold,
                  size_threshold, micro_batch, on_device, cap, max_crops, return_scores=False, tiled=False):
        n = len(ptrs)
        keep = [np.ascontiguousarray(p, dtype=np.uint8) if not isinstance(p, (int, np.integer)) else p for p in ptrs]
        c_ptrs = (ctypes.c_void_p * n)(*[int(p) if isinstance(p, (int, np.integer)) else p.ctypes.data for p in keep])
        arr = [np.ascontiguousarray(v, dtype=np.int32) for v in (hs, ws, dhs, dws)]
        cap = int(cap)
        max_crops = int(max_crops) if max_crops else max(64, n * cap)
        lw = self.crnn_label_width()
        boxes = np.zeros((n, cap, 4, 2), dtype=np.float32)
        counts = np.zeros(n, dtype=np.int32)
        labels = np.full((max_crops, lw), -1, dtype=np.int32)
        n_crops = np.zeros(1, dtype=np.int32)
        rc = (self._lib.kocr_pipeline_tiled if tiled else self._lib.kocr_pipeline)(
            self._h, n, c_ptrs, *[a.ctypes.data_as(_c_int_p) for a in arr], int(hmax), int(wmax),
            float(detection_threshold), float(text_threshold), float(link_threshold), int(size_threshold),
            int(micro_batch), _ptr(boxes), _ptr(counts), cap, _ptr(labels), max_crops, _ptr(n_crops),
            int(bool(on_device)))
        if rc == KOCR_ECAPACITY and n and (counts.max() > cap or int(n_crops[0]) > max_crops):
            # KOCR_ECAPACITY with the true counts: the whole chain has run ONCE and its results are resident in HBM (round 6:
            # no second detector forward) -- fetch them into buffers of the right size
            cap = max(cap, int(counts.max()))
            max_crops = max(max_crops, int(n_crops[0]))
            boxes = np.zeros((n, cap, 4, 2), dtype=np.float32)
            lw = self.pipeline_results_shape()[1]  # the width the resident rows were produced with
            labels = np.full((max_crops, lw), -1, dtype=np.int32)
            rc = self._lib.kocr_pipeline_results(self._h, _ptr(boxes), cap, _ptr(labels), max_crops)
        self._check(rc)
        out = Results(_box_lists(boxes, counts), labels[:int(n_crops[0])].copy())
        return self._fetch_extras(out, Extras(scores=True), n, counts, cap) if return_scores else out

    # -- tiled pages (include/kocr.h: "tiled pages") ------------------------------------------------
    def pipeline_tiled(self, ptrs, hs, ws, dhs, dws, tile, overlap, **kwargs):
        """``pipeline`` with the detector run in overlapping tiles (kocr_pipeline_tiled): ``tile`` / ``overlap`` as
        ``tools.tile_plan`` in place of ``hmax`` / ``wmax`` -- the batch is padded to the plan's canvas of the largest
        ``dhs`` x ``dws``.  Every keyword and every element of the result as ``pipeline``; boxes in canvas = detector-input
        pixels.  ValueError for a refused tile or overlap."""
        from . import tools  # pylint: disable=import-outside-toplevel,cyclic-import
        if len(ptrs):
            tools.tile_plan(max(int(v) for v in dhs), max(int(v) for v in dws), tile, overlap)
        return self.pipeline(ptrs, hs, ws, dhs, dws, int(tile), int(overlap), tiled=True, **kwargs)

    def tile_plan(self, height, width, tile, overlap):
        """kocr_tile_plan: ``(ny, nx, Hc, Wc, S, nT)`` as the library computes them (``tools.tile_plan`` is the same plan
        without a library call); ValueError for refused parameters."""
        out = np.zeros(6, dtype=np.int32)
        self._check(self._lib.kocr_tile_plan(self._h, int(height), int(width), int(tile), int(overlap), _ptr(out)), value_error=True)
        return tuple(int(v) for v in out)

    def _canvases(self, canvas, tile, overlap):
        """(N,Hc,Wc,3) uint8 canvases of the plan -> (array, n, hc, wc, tiles per canvas); ValueError otherwise"""
        from . import tools  # pylint: disable=import-outside-toplevel,cyclic-import
        x = np.ascontiguousarray(canvas, dtype=np.uint8)
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("canvas must have shape (N,Hc,Wc,3)")
        n, hc, wc, _ = x.shape
        plan = tools.tile_plan(hc, wc, tile, overlap)
        if plan.canvas != (hc, wc):
            raise ValueError(f"{hc} x {wc} is not a canvas of tile {tile} and overlap {overlap}: tile_plan gives {plan.canvas}")
        return x, n, hc, wc, plan.counts[0] * plan.counts[1]

    def gather_tiles(self, canvas, tile, overlap):
        """canvas: (N,Hc,Wc,3) uint8, Hc x Wc a canvas of ``tools.tile_plan``.  Returns the tiles (N * nT, T, T, 3) uint8,
        canvas-major, row-major within a canvas: a pure copy (tile_gather)."""
        x, n, hc, wc, n_tiles = self._canvases(canvas, tile, overlap)
        out = np.empty((n * n_tiles, int(tile), int(tile), 3), dtype=np.uint8)
        self._check(self._lib.kocr_gather_tiles(self._h, _ptr(x), n, hc, wc, int(tile), int(overlap), _ptr(out), 0))
        return out

    def stitch_heat(self, tile_heat, canvas_hw, tile, overlap):
        """tile_heat: (N * nT, T/2, T/2, 2) float32 heat-maps of the tiles of N canvases of ``canvas_hw`` = (Hc, Wc).  Returns
        (N, Hc/2, Wc/2, 2) float32: every pixel the bits of the one tile whose core contains it (heat_stitch)."""
        from . import tools  # pylint: disable=import-outside-toplevel,cyclic-import
        hc, wc = int(canvas_hw[0]), int(canvas_hw[1])
        plan = tools.tile_plan(hc, wc, tile, overlap)
        if plan.canvas != (hc, wc):
            raise ValueError(f"{hc} x {wc} is not a canvas of tile {tile} and overlap {overlap}: tile_plan gives {plan.canvas}")
        n_tiles, t2 = plan.counts[0] * plan.counts[1], int(tile) // 2
        y = np.ascontiguousarray(tile_heat, dtype=np.float32)
        if y.ndim != 4 or y.shape[1:] != (t2, t2, 2) or y.shape[0] % n_tiles:
            raise ValueError(f"tile_heat must have shape (N * {n_tiles}, {t2}, {t2}, 2)")
        n = y.shape[0] // n_tiles
        out = np.empty((n, hc // 2, wc // 2, 2), dtype=np.float32)
        self._check(self._lib.kocr_stitch_heat(self._h, _ptr(y), n, hc, wc, int(tile), int(overlap), _ptr(out), 0))
        return out

    def craft_forward_tiled(self, canvas, tile, overlap, micro_batch=0):
        """canvas: (N,Hc,Wc,3) uint8 as ``gather_tiles``.  Returns the stitched heat-maps (N, Hc/2, Wc/2, 2) float32 of a
        detector pass over the tiles, ``micro_batch`` tiles at a time (kocr_craft_forward_tiled)."""
        x, n, hc, wc, _ = self._canvases(canvas, tile, overlap)
        out = np.empty((n, hc // 2, wc // 2, 2), dtype=np.float32)
        self._check(self._lib.kocr_craft_forward_tiled(self._h, _ptr(x), n, hc, wc, int(tile), int(overlap), _ptr(out),
                                                       int(micro_batch), 0))
        return out

    def _detect_tiled(self, canvas, tile, overlap, detection_threshold, text_threshold, link_threshold, size_threshold, micro_batch,
                      cap, min_area_rect=None, return_scores=False, char_boxes=None):
        """``_detect`` on canvases read in tiles (kocr_detect_tiled)"""
        x, n, hc, wc, _ = self._canvases(canvas, tile, overlap)
        return self._boxes_grow_cap(n, cap, lambda boxes, counts, cap: self._lib.kocr_detect_tiled(
            self._h, _ptr(x), n, hc, wc, int(tile), int(overlap), float(detection_threshold), float(text_threshold),
            float(link_threshold), int(size_threshold), int(micro_batch), _ptr(boxes), _ptr(counts), cap, 0),
            min_area_rect, return_scores, char_boxes)

    def pipeline_results_shape(self):
        """``(m, lw)`` of the label rows the last `pipeline()` call left resident (kocr_pipeline_results_shape): ``lw`` is the
        label width they were PRODUCED with, whatever ``crnn_label_width()`` says by now."""
        m, lw = ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._lib.kocr_pipeline_results_shape(self._h, ctypes.byref(m), ctypes.byref(lw)))
        return m.value, lw.value

    def pipeline_device_results(self):
        """Device pointers of the last `pipeline()` call's results (include/kocr.h: kocr_pipeline_device_results):
        {"boxes": ptr of [n][cap][4][2] f32, "counts": ptr of [n] i32, "labels": ptr of [m][lw] i32 or 0, "n", "cap", "m",
        "lw": the label width the rows were produced with (48 by default)}; valid until the next call on this context."""
        pb, pc, pl = ctypes.c_void_p(0), ctypes.c_void_p(0), ctypes.c_void_p(0)
        n, cap, m = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        self._check(self._lib.kocr_pipeline_device_results(self._h, ctypes.byref(pb), ctypes.byref(pc), ctypes.byref(pl),
                                                           ctypes.byref(n), ctypes.byref(cap), ctypes.byref(m)))
        return {"boxes": pb.value or 0, "counts": pc.value or 0, "labels": pl.value or 0, "n": n.value, "cap": cap.value, "m": m.value,
                "lw": self.pipeline_results_shape()[1]}

    def conv2d_nhwc(self, x, w_hwio, dilation=1, pre_a=None, pre_b=None, relu=False, post_a=None, post_b=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(w_hwio, dtype=np.float32)
        n, h, wd, cin = x.shape
        kh, kw, cin2, cout = w.shape
        assert cin == cin2
        out = np.empty((n, h, wd, cout), dtype=np.float32)
        vecs = [None if v is None else np.ascontiguousarray(v, dtype=np.float32) for v in (pre_a, pre_b, post_a, post_b)]
        self._check(self._lib.kocr_conv2d_nhwc(self._h, _ptr(x), n, h, wd, cin, _ptr(w), kh, kw, int(dilation), cout,
                                               _ptr(vecs[0]), _ptr(vecs[1]), int(bool(relu)), _ptr(vecs[2]),
                                               _ptr(vecs[3]), _ptr(out)))
        return out

    def conv2d_cells(self, x, w_hwio, cell_w, cell_wv, pool=False, need_full=True, pre_a=None, pre_b=None, relu=False,
                     post_a=None, post_b=None):
        """3x3 convolution of a cell grid (include/kocr.h: kocr_conv2d_cells).  Returns (out or None, pooled or None,
        per-cell max |x| of what was written [N, W // cell_w])."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        w = np.ascontiguousarray(w_hwio, dtype=np.float32)
        n, h, wd, cin = x.shape
        assert w.shape[:3] == (3, 3, cin)
        cout = w.shape[3]
        out = np.empty((n, h, wd, cout), dtype=np.float32) if (need_full or not pool) else None
        pooled = np.empty((n, h // 2, wd // 2, cout), dtype=np.float32) if pool else None
        amax = np.zeros((n, wd // cell_w), dtype=np.float32)
        vecs = [None if v is None else np.ascontiguousarray(v, dtype=np.float32) for v in (pre_a, pre_b, post_a, post_b)]
        self._check(self._lib.kocr_conv2d_cells(self._h, _ptr(x), n, h, wd, cin, _ptr(w), cout, _ptr(vecs[0]), _ptr(vecs[1]),
                                                int(bool(relu)), _ptr(vecs[2]), _ptr(vecs[3]), int(cell_w), int(cell_wv),
                                                int(bool(pool)), _ptr(out), _ptr(pooled), _ptr(amax)))
        return out, pooled, amax

    # -- arithmetic of the wide convolutions (include/kocr.h: KOCR_SPLIT_*) ---------------
    SPLIT_BF16X3, SPLIT_F16X2, SPLIT_F16X1 = 0, 1, 2

    def set_split_mode(self, mode):
        if isinstance(mode, str):
            mode = {"bf16": 0, "bf16x3": 0, "f16": 1, "fp16": 1, "f16x2": 1, "f16x1": 2, "fast": 2}[mode]
        self._check(self._lib.kocr_set_split_mode(self._h, int(mode)))

    def get_split_mode(self):
        return self._check(self._lib.kocr_get_split_mode(self._h))

    def set_schedule(self, fold_linear_chain=True, fold_upsample=True):
        """CRAFT schedule switches (include/kocr.h kocr_set_schedule); both on by default."""
        self._check(self._lib.kocr_set_schedule(self._h, int(bool(fold_linear_chain)), int(bool(fold_upsample))))

    def get_schedule(self):
        """(fold_linear_chain, fold_upsample) in force on this context (include/kocr.h kocr_get_schedule)."""
        lin, up = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.kocr_get_schedule(self._h, ctypes.byref(lin), ctypes.byref(up)))
        return bool(lin.value), bool(up.value)

    # -- minAreaRect rule of getBoxes (include/kocr.h: kocr_set_min_area_rect) ---------------
    def set_min_area_rect(self, rule):
        """``"exact"`` (default: exact-integer min-area rectangle) or ``"opencv"`` (cv2.minAreaRect's float32 rotating
        calipers and cv2.boxPoints) for every later getBoxes on this context."""
        self._check(self._lib.kocr_set_min_area_rect(self._h, _min_area_rect_code(rule)))

    def get_min_area_rect(self):
        code = self._check(self._lib.kocr_get_min_area_rect(self._h))
        return {v: k for k, v in MIN_AREA_RECT_RULES.items()}[code]

    # -- measurement -------------------------------------------------------------------
    # -- the detector's training data and validation loss (detection.py:106-198, :696) ----------------------------------
    def compute_maps(self, heatmap, image_height, image_width, line_groups):
        """detection.compute_maps for a batch of pages (kocr_compute_maps): ``line_groups`` holds, per page, a list of lines
        of (points (4, 2), character) -- the ``lines`` argument of the reference.  Returns (N, H/2, W/2, 2) float32.
        ``heatmap``: 2-D uint8.  The points are taken as float32.  An odd height or width raises AssertionError, an empty
        line IndexError (as the reference)."""
        hm = np.ascontiguousarray(heatmap)
        if hm.ndim != 2 or hm.dtype != np.uint8:
            raise NotImplementedError(f"compute_maps takes a 2-D uint8 heat-map, got {hm.dtype} of shape {hm.shape}")
        assert image_height % 2 == 0, "Height must be an even number"
        assert image_width % 2 == 0, "Width must be an even number"
        q, sp, loff, ioff = _flatten_lines(line_groups)
        n = len(ioff) - 1
        out = np.zeros((n, image_height // 2, image_width // 2, 2), dtype=np.float32)
        self._check(self._lib.kocr_compute_maps(self._h, _ptr(hm), hm.shape[0], hm.shape[1], n, int(image_height),
                                                int(image_width), len(q), _ptr(q), _ptr(sp), len(loff) - 1, _ptr(loff),
                                                _ptr(ioff), _ptr(out), 0))
        return out

    def heat_mse(self, y_true, y_pred):
        """Per-image float64 sums of Keras' mse on (N, h, w, 2) maps (kocr_heat_mse): sum over pixels of the channel mean
        of (y_true - y_pred)^2."""
        y = np.ascontiguousarray(y_true, dtype=np.float32)
        p = np.ascontiguousarray(y_pred, dtype=np.float32)
        if y.shape != p.shape or y.ndim != 4 or y.shape[3] != 2:
            raise ValueError(f"y_true and y_pred must both have shape (N, h, w, 2), got {y.shape} and {p.shape}")
        sums = np.zeros(y.shape[0], np.float64)
        self._check(self._lib.kocr_heat_mse(self._h, _ptr(y), _ptr(p), y.shape[0], y.shape[1], y.shape[2], _ptr(sums), 0))
        return sums

    def craft_mse(self, images, y_true, micro_batch=0):
        """craft_forward(images) and heat_mse against y_true in one call (kocr_craft_mse): the heat-maps stay in HBM."""
        x, dt = _detector_input(images)
        if x.ndim != 4 or x.shape[3] != 3:
            raise ValueError("images must have shape (N,H,W,3)")
        n, h, w, _ = x.shape
        y = np.ascontiguousarray(y_true, dtype=np.float32)
        if y.shape != (n, h // 2, w // 2, 2):
            raise ValueError(f"y must have shape {(n, h // 2, w // 2, 2)}, got {y.shape}")
        sums = np.zeros(n, np.float64)
        self._check(self._lib.kocr_craft_mse(self._h, _ptr(x), dt, n, h, w, _ptr(y), int(micro_batch), _ptr(sums), 0))
        return sums

    # -- evaluation (include/kocr.h: "evaluation"; evaluation.py:13-147) ------------------------------------------------
    def iou_table(self, truth_quads, truth_offsets, pred_quads, pred_offsets):
        """IoU of every (truth, prediction) pair of N images (kocr_iou_table): quads int32 (n, 4, 2), offsets (N + 1,).
        Returns float64 (P,), P = sum nt_i * np_i, image-major, truth-major inside an image.  ValueError for offsets that
        do not start at 0 or decrease and for a coordinate outside (-2^24, 2^24), naming image and annotation."""
        tq, toff, pq, poff = _eval_quads(truth_quads, truth_offsets, pred_quads, pred_offsets)
        pairs = max(0, int((np.diff(toff).astype(np.int64) * np.diff(poff).astype(np.int64)).sum()))
        iou = np.zeros(pairs, np.float64)
        self._check(self._lib.kocr_iou_table(self._h, len(toff) - 1, _ptr(tq), _ptr(toff), _ptr(pq), _ptr(poff), _ptr(iou), pairs,
                                             None, 0), value_error=True)
        return iou

    def score_tables(self, truth_quads, truth_offsets, pred_quads, pred_offsets, ignore, truth_text, truth_text_offsets,
                     pred_text, pred_text_offsets, iou_threshold=0.5, similarity_threshold=0.5, return_iou=False):
        """evaluation.score's tables for N images in one call (kocr_score): quads / offsets as iou_table, ``ignore`` uint8
        (nt,), texts as concatenated int32 code points with offsets (nt + 1,) / (np + 1,), at most 256 code points each.
        Returns ``(pair_class uint8 (P,), truth_missed uint8 (nt,), pred_unclaimed uint8 (np,), counts int64 (3,)[, iou
        float64 (P,)])``: class 0 no overlap, 1 true positive, 2 near true positive, 3 overlap with an ignored truth;
        counts = truths with a class-1 pair, unclaimed predictions, missed truths.  ValueError as iou_table, and for a
        longer text."""
        tq, toff, pq, poff = _eval_quads(truth_quads, truth_offsets, pred_quads, pred_offsets)
        ign = np.ascontiguousarray(ignore, dtype=np.uint8)
        tt, tto = np.ascontiguousarray(truth_text, dtype=np.int32), np.ascontiguousarray(truth_text_offsets, dtype=np.int32)
        pt, pto = np.ascontiguousarray(pred_text, dtype=np.int32), np.ascontiguousarray(pred_text_offsets, dtype=np.int32)
        if len(ign) != len(tq) or len(tto) != len(tq) + 1 or len(pto) != len(pq) + 1:
            raise ValueError("score_tables: ignore / text offsets do not match the number of boxes")
        if len(tt) < tto[-1] or len(pt) < pto[-1]:
            raise ValueError("score_tables: text offsets run past the texts")
        pairs = max(0, int((np.diff(toff).astype(np.int64) * np.diff(poff).astype(np.int64)).sum()))
        cls, missed, unclaimed = np.zeros(pairs, np.uint8), np.zeros(len(tq), np.uint8), np.zeros(len(pq), np.uint8)
        counts = np.zeros(3, np.int64)
        iou = np.zeros(pairs, np.float64) if return_iou else None
        self._check(self._lib.kocr_score(self._h, len(toff) - 1, _ptr(tq), _ptr(toff), _ptr(pq), _ptr(poff), _ptr(ign), _ptr(tt),
                                         _ptr(tto), _ptr(pt), _ptr(pto), float(iou_threshold), float(similarity_threshold),
                                         _ptr(cls), _ptr(missed), _ptr(unclaimed), _ptr(counts), _ptr(iou), pairs, None, 0),
                    value_error=True)
        return (cls, missed, unclaimed, counts) + ((iou,) if return_iou else ())

    # -- lines (include/kocr.h: "lines") ------------------------------------------------------------------------------------
    def group_lines(self, quads, offsets, max_angle=15.0, min_height_ratio=0.5, max_offset=0.5, max_gap=1.5, return_boxes=True):
        """The words of N pages grouped into text lines in reading order, in one call (kocr_group_lines; DESIGN.md section 4,
        "Lines"): ``quads`` float32 (total, 4, 2), the pages' word boxes [tl, tr, br, bl] one after the other, ``offsets``
        (N + 1,), at most 2048 words on a page.  Returns ``(line_of int32 (total,), order int32 (total,), line_counts int32
        (N,), line_boxes float32 (lines, 4, 2) or None)``: the index of each word's line among its page's lines; per page
        the page-local word indices in reading order, line after line; the lines per page; the box of every line of every
        page in that order.  ValueError for ``max_angle`` outside [0, 90), another rule parameter out of range, offsets that
        do not start at 0 or decrease, a page of more than 2048 words and a non-finite coordinate (naming page and word).
        Columns are not detected: ``group_blocks`` on the line boxes cuts a page into columns and paragraphs."""
        max_angle = float(max_angle)
        if not 0 <= max_angle < 90:
            raise ValueError(f"group_lines: max_angle {max_angle} outside [0, 90)")
        q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 4, 2)
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        if len(off) < 1 or off[-1] != len(q):
            raise ValueError(f"group_lines: offsets must hold N + 1 entries and end at the number of boxes, {len(q)}")
        n, total = len(off) - 1, len(q)
        line_of, order, counts = np.zeros(total, np.int32), np.zeros(total, np.int32), np.zeros(n, np.int32)
        boxes = np.zeros((total, 4, 2), np.float32) if return_boxes else None  # a page has at most as many lines as words
        lines = ctypes.c_int64(0)
        self._check(self._lib.kocr_group_lines(self._h, n, _ptr(q), _ptr(off), math.cos(math.radians(max_angle)), float(min_height_ratio),
                                               float(max_offset), float(max_gap), _ptr(line_of), _ptr(order), _ptr(counts), _ptr(boxes),
                                               total if return_boxes else 0, ctypes.byref(lines), 0), value_error=True)
        return line_of, order, counts, (boxes[:lines.value].copy() if return_boxes else None)

    def group_blocks(self, quads, offsets, min_gap_x=1.0, min_gap_y=0.75, return_boxes=True):
        """The quads of N pages -- any quads, in practice ``group_lines``' line boxes -- cut into blocks (columns,
        paragraphs) by a recursive XY-cut and put into reading order, in one call (kocr_group_lines with
        KOCR_LINES_BLOCKS; DESIGN.md section 4, "Blocks"): ``quads`` float32 (total, 4, 2), ``offsets`` (N + 1,), at most
        2048 quads on a page.  A quad counts as its axis-aligned box.  A set of boxes is cut at every gap along x of at
        least ``min_gap_x`` mean line heights (columns, left to right), otherwise at the widest gap along y of at least
        ``min_gap_y`` mean line heights (paragraphs, headings, footers; top first), otherwise it is a block.  The defaults
        are judgement, not fitted to real pages.  Returns ``(block_of int32 (total,), order int32 (total,), block_counts
        int32 (N,), block_boxes float32 (blocks, 4, 2) or None)``: the index of each quad's block among its page's blocks;
        per page the page-local quad indices in reading order, block after block, top to bottom inside a block; the
        blocks per page; the box [tl, tr, br, bl] of every block of every page in that order.  The cut is axis-aligned (a
        rotated page goes to ``group_blocks_deskewed``) and whitespace is its only cue.  ValueError for a gap that is
        negative or not finite, offsets that do not start at 0 or decrease, a page of more than 2048 quads and a
        non-finite coordinate (naming page and quad)."""
        return Context._group_blocks(self, quads, offsets, min_gap_x, min_gap_y, return_boxes, KOCR_LINES_BLOCKS)

    def group_blocks_deskewed(self, quads, offsets, min_gap_x=1.0, min_gap_y=0.75, return_boxes=True):
        """``group_blocks`` for rotated pages -- a skewed scan, a photo, a page fed in sideways or upside down
        (kocr_group_lines with KOCR_LINES_BLOCKS | KOCR_LINES_DESKEW; DESIGN.md section 4, "Rotated pages").  Every page's
        text direction is estimated on the GPU from its own quads (the weighted medoid of their tl -> tr directions), the
        cut runs in that frame, and ``block_boxes`` are rotated rectangles in page coordinates, tl -> tr along the text
        (``layout.box_angle`` reads the skew off any of them).  Arguments, the rest of the return value and the
        ValueErrors are ``group_blocks``'; so are the numbers on a page that is not rotated.  Not covered: a page whose
        text runs in several directions, and quads whose tl -> tr is not the reading direction."""
        return Context._group_blocks(self, quads, offsets, min_gap_x, min_gap_y, return_boxes, KOCR_LINES_BLOCKS | KOCR_LINES_DESKEW)

    def _group_blocks(self, quads, offsets, min_gap_x, min_gap_y, return_boxes, flags):
        """both block modes; called through the class, so that the arguments are refused by name on any object"""
        gaps = {"min_gap_x": float(min_gap_x), "min_gap_y": float(min_gap_y)}
        for name, value in gaps.items():
            if not (value >= 0 and math.isfinite(value)):
                raise ValueError(f"group_blocks: {name} {value} is not a finite number >= 0")
        q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 4, 2)
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        if len(off) < 1 or off[-1] != len(q):
            raise ValueError(f"group_blocks: offsets must hold N + 1 entries and end at the number of boxes, {len(q)}")
        n, total = len(off) - 1, len(q)
        block_of, order, counts = np.zeros(total, np.int32), np.zeros(total, np.int32), np.zeros(n, np.int32)
        boxes = np.zeros((total, 4, 2), np.float32) if return_boxes else None  # a page has at most as many blocks as quads
        blocks = ctypes.c_int64(0)
        # cos_max and min_height_ratio are checked and not read; the two gaps travel as max_offset and max_gap
        self._check(self._lib.kocr_group_lines(self._h, n, _ptr(q), _ptr(off), 1.0, 0.0, gaps["min_gap_x"], gaps["min_gap_y"], _ptr(block_of),
                                               _ptr(order), _ptr(counts), _ptr(boxes), total if return_boxes else 0, ctypes.byref(blocks),
                                               flags), value_error=True)
        return block_of, order, counts, (boxes[:blocks.value].copy() if return_boxes else None)

    def group_table(self, quads, offsets, min_gap_x=1.0, min_gap_y=0.25, min_support=0.5, return_boxes=True):
        """The quads of N pages -- any quads, in practice the word boxes of ONE table each: a whole page, or the words of one
        ``Block`` -- put into rows, columns and spanning cells by the white space between them, in one call
        (kocr_group_lines with KOCR_LINES_TABLE; DESIGN.md section 4, "Tables"): ``quads`` float32 (total, 4, 2),
        ``offsets`` (N + 1,), at most 2048 quads on a page.  A quad counts as its axis-aligned box.  Rows: the page is cut at
        every gap along y of at least ``min_gap_y`` mean heights.  Columns: a separator stands where at least
        ``min_support`` of the rows (rounded up, at least one) are white over a stretch of at least ``min_gap_x`` mean
        heights that ends before the page's right edge; a row's margins up to the page's extent count as white.  The
        defaults are judgement, not fitted to real pages.  Returns ``(row_of int32 (total,), col_first int32 (total,),
        col_last int32 (total,), row_counts int32 (N,), col_counts int32 (N,), row_boxes, col_boxes)``: the row of every
        quad and the first and last column it touches (``col_last > col_first``: a spanning cell); rows and columns per
        page (0 and 0 for a page without quads); the bands [tl, tr, br, bl] of all rows of all pages in page order, float32
        (rows, 4, 2), and likewise of all columns -- both None without ``return_boxes``.  The rule is axis-aligned and
        whitespace is its only cue; one table per page.  ValueError for a gap that is negative or not finite,
        ``min_support`` outside [0, 1], offsets that do not start at 0 or decrease, a page of more than 2048 quads and a
        non-finite coordinate (naming page and quad)."""
        rule = {"min_gap_x": float(min_gap_x), "min_gap_y": float(min_gap_y)}
        for name, value in rule.items():
            if not (value >= 0 and math.isfinite(value)):
                raise ValueError(f"group_table: {name} {value} is not a finite number >= 0")
        min_support = float(min_support)
        if not 0 <= min_support <= 1:
            raise ValueError(f"group_table: min_support {min_support} outside [0, 1]")
        q = np.ascontiguousarray(quads, dtype=np.float32).reshape(-1, 4, 2)
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        if len(off) < 1 or off[-1] != len(q):
            raise ValueError(f"group_table: offsets must hold N + 1 entries and end at the number of boxes, {len(q)}")
        n, total = len(off) - 1, len(q)
        row_of, cols, counts = np.zeros(total, np.int32), np.zeros(total, np.int32), np.zeros(n, np.int32)
        boxes = np.zeros((2 * total, 4, 2), np.float32) if return_boxes else None  # a page of n quads has at most 2 n bands
        bands = ctypes.c_int64(0)
        # cos_max is checked and not read; the gaps travel as max_offset and max_gap, min_support as min_height_ratio
        self._check(self._lib.kocr_group_lines(self._h, n, _ptr(q), _ptr(off), 1.0, min_support, rule["min_gap_x"], rule["min_gap_y"],
                                               _ptr(row_of), _ptr(cols), _ptr(counts), _ptr(boxes), 2 * total if return_boxes else 0,
                                               ctypes.byref(bands), KOCR_LINES_TABLE), value_error=True)
        # a page's rows: 1 + its largest row (every row has a member); its columns: the other bands
        row_counts = np.array([int(row_of[a:b].max()) + 1 if b > a else 0 for a, b in zip(off[:-1], off[1:])], np.int32).reshape(n)
        col_counts = counts - row_counts
        row_boxes = col_boxes = None
        if return_boxes:
            first = np.concatenate([[0], np.cumsum(counts, dtype=np.int64)])
            is_row = np.zeros(int(bands.value), bool)
            for i in range(n):
                is_row[first[i]:first[i] + row_counts[i]] = True
            row_boxes, col_boxes = boxes[:bands.value][is_row], boxes[:bands.value][~is_row]
        return row_of, cols & 0xFFFF, cols >> 16, row_counts, col_counts, row_boxes, col_boxes

    def profile_enable(self, on=True):
        self._check(self._lib.kocr_profile_enable(self._h, int(bool(on))))

    def profile_reset(self):
        self._check(self._lib.kocr_profile_reset(self._h))

    def profile_report(self):
        cap = 128
        names = ctypes.create_string_buffer(cap * 64)
        launches = np.zeros(cap, dtype=np.int64)
        ms = np.zeros(cap, dtype=np.float64)
        flops = np.zeros(cap, dtype=np.float64)
        byts = np.zeros(cap, dtype=np.float64)
        n = self._check(self._lib.kocr_profile_report(
            self._h, cap, names, launches.ctypes.data_as(_c_i64_p), ms.ctypes.data_as(_c_dbl_p),
            flops.ctypes.data_as(_c_dbl_p), byts.ctypes.data_as(_c_dbl_p)))
        rows = {}
        for i in range(min(n, cap)):
            nm = names.raw[i * 64:(i + 1) * 64].split(b"\0", 1)[0].decode()
            rows[nm] = {"launches": int(launches[i]), "ms": float(ms[i]), "flops": float(flops[i]),
                        "bytes": float(byts[i])}
        return rows


    # -- range statistics of the fp16x2 arithmetic (include/kocr.h; developer instrumentation) ----------
    def range_stats_enable(self, on=True):
        self._check(self._lib.kocr_range_stats_enable(self._h, int(bool(on))))

    def range_stats_report(self):
        """{layer: {launches, elements, nonzero, below_2^-4, below_2^-14, frac_below_2^-4 (of the non-zero elements),
        frac_below_2^-14, share_of_sum_abs_below_2^-4}} accumulated since range_stats_enable(True)."""
        cap = 256
        names = ctypes.create_string_buffer(cap * 64)
        vals = np.zeros(cap * 7, dtype=np.float64)
        n = self._check(self._lib.kocr_range_stats_report(self._h, cap, names, vals.ctypes.data_as(_c_dbl_p)))
        rows = {}
        for i in range(min(n, cap)):
            nm = names.raw[i * 64:(i + 1) * 64].split(b"\0", 1)[0].decode()
            la, el, nz, b4, b14, sa, sb = vals[i * 7:i * 7 + 7]
            rows[nm] = {"launches": int(la), "elements": el, "nonzero": nz, "below_2^-4": b4, "below_2^-14": b14,
                        "frac_below_2^-4": b4 / nz if nz else 0.0, "frac_below_2^-14": b14 / nz if nz else 0.0,
                        "share_of_sum_abs_below_2^-4": sb / sa if sa else 0.0}
        return rows

    # -- workspace arenas (include/kocr.h: for tests, not for callers) ----------------------------------
    def arena_names(self):
        return [self._lib.kocr_debug_arena_name(i).decode() for i in range(self._lib.kocr_debug_arena_count())]

    def arena_stats(self):
        """{arena: {cap, requested, peak, excess}} in bytes (kocr_debug_arena_stats)"""
        out = {}
        for i, name in enumerate(self.arena_names()):
            v = [ctypes.c_uint64(0) for _ in range(4)]
            self._check(self._lib.kocr_debug_arena_stats(self._h, i, *[ctypes.byref(x) for x in v]))
            out[name] = dict(zip(("cap", "requested", "peak", "excess"), (int(x.value) for x in v)))
        return out

    def debug_memory(self):
        """{persistent_count, persistent_bytes, arena_bytes, process_count, process_bytes} (kocr_debug_memory_stats): the device
        memory this context owns, and what the library holds in the whole process -- counted, never read from the device."""
        v = [ctypes.c_uint64(0) for _ in range(5)]
        self._check(self._lib.kocr_debug_memory_stats(self._h, *[ctypes.byref(x) for x in v]))
        return dict(zip(("persistent_count", "persistent_bytes", "arena_bytes", "process_count", "process_bytes"),
                        (int(x.value) for x in v)))

    def release_arenas(self):
        """Frees every arena and forgets every resident result: the context is cold again, its networks stay loaded."""
        self._check(self._lib.kocr_debug_release_arenas(self._h))

    def set_arena_guards(self, on=True):
        self._check(self._lib.kocr_debug_set_arena_guards(self._h, int(bool(on))))

    def set_arena_poison(self, byte=None):
        """Poison mode (kocr_debug_set_arena_poison): every workspace allocation is filled with ``byte`` (0..255) on the stream
        when it is made; None switches the mode off."""
        self._check(self._lib.kocr_debug_set_arena_poison(self._h, -1 if byte is None else int(byte)))

    def check_arena_guards(self):
        """(damaged guards since the last check, first one's arena name or None, its buffer's offset, its first damaged byte)"""
        arena, off, byte = ctypes.c_int(-1), ctypes.c_uint64(0), ctypes.c_uint64(0)
        n = self._check(self._lib.kocr_debug_check_arena_guards(self._h, ctypes.byref(arena), ctypes.byref(off), ctypes.byref(byte)))
        names = self.arena_names()
        return n, (names[arena.value] if 0 <= arena.value < len(names) else None), int(off.value), int(byte.value)


# Context._extras_scope's switches in the order they are set: (field of extras.Extras, the field -> what the setter takes
# (None: it asks for nothing), getter, setter, how the old setting is restored (None: the setter)).  A lexicon, character sets
# or patterns unloaded meanwhile took their switch with them: then nothing is restored.
_SWITCHES = (
    ("char_boxes", lambda v: char_rule(v) and (True, char_rule(v)), Context.get_char_boxes,
     lambda ctx, new: ctx.set_char_boxes(new[0], **new[1]),
     lambda ctx, old: (ctx.set_char_boxes(True, **old[1]), ctx.set_char_boxes(old[0], **old[1]))),  # the parameters, then the switch
    ("min_area_rect", lambda v: v, Context.get_min_area_rect, Context.set_min_area_rect, None),
    ("scores", lambda v: True if v else None, Context.get_scores, Context.set_scores, None),
    ("beam", lambda v: None if v is None else beam_args(*v), Context.get_beam, lambda ctx, new: ctx.set_beam(*new), None),
    ("lexicon_top", lambda v: v, Context.get_lexicon_match, Context.set_lexicon_match,
     lambda ctx, old: ctx.lexicon_size() and ctx.set_lexicon_match(old)),
    ("orientation", lambda v: v, Context.get_orientation, lambda ctx, new: ctx.set_orientation(*new), None),
    ("charset", lambda v: v if v is None else int(v), Context.get_charset, Context.set_charset, lambda ctx, old: old < ctx.charset_count() and ctx.set_charset(old)),
    ("pattern", lambda v: v if v is None else int(v), Context.get_pattern, Context.set_pattern, lambda ctx, old: old < ctx.pattern_count() and ctx.set_pattern(old)),
)


def _detector_input(images):
    """images as the detector takes them: uint8 (raw RGB, KOCR_U8) as they are, anything else as float32 (KOCR_F32)"""
    x = np.ascontiguousarray(images)
    if x.dtype == np.uint8:
        return x, KOCR_U8
    return np.ascontiguousarray(x, dtype=np.float32), KOCR_F32


def _eval_quads(truth_quads, truth_offsets, pred_quads, pred_offsets):
    """iou_table / score_tables arguments as contiguous int32 arrays, shapes checked against the offsets' last entries"""
    tq = np.ascontiguousarray(truth_quads, dtype=np.int32).reshape(-1, 4, 2)
    pq = np.ascontiguousarray(pred_quads, dtype=np.int32).reshape(-1, 4, 2)
    toff = np.ascontiguousarray(truth_offsets, dtype=np.int32).reshape(-1)
    poff = np.ascontiguousarray(pred_offsets, dtype=np.int32).reshape(-1)
    if len(toff) < 1 or len(toff) != len(poff):
        raise ValueError("truth_offsets and pred_offsets must both hold N + 1 entries")
    if toff[-1] != len(tq) or poff[-1] != len(pq):
        raise ValueError(f"offsets end at {toff[-1]} / {poff[-1]} but there are {len(tq)} / {len(pq)} boxes")
    return tq, toff, pq, poff


def _flatten_lines(line_groups):
    """per page a list of lines of (points, character) -> char_quads float32 (n, 4, 2), is_space uint8 (n,), line_offsets
    int32 (n_lines + 1,), image_line_offsets int32 (N + 1,): one np.asarray per line.  An empty line raises IndexError (as
    the reference's fix_line), a non-finite point ValueError."""
    quads, spaces, line_len, page_len = [], [], [], []
    for lines in line_groups:
        page_len.append(len(lines))
        for line in lines:
            if len(line) == 0:
                raise IndexError("too many indices for array: array is 1-dimensional, but 2 were indexed")
            boxes, chars = zip(*line)
            quads.append(np.asarray(boxes, dtype=np.float32).reshape(len(line), 4, 2))
            spaces.append(np.fromiter((c == " " for c in chars), dtype=np.uint8, count=len(line)))
            line_len.append(len(line))
    q = np.ascontiguousarray(np.concatenate(quads) if quads else np.zeros((0, 4, 2), np.float32))
    if not np.isfinite(q).all():
        raise ValueError("compute_maps: character points must be finite")
    sp = np.ascontiguousarray(np.concatenate(spaces) if spaces else np.zeros(0, np.uint8))
    loff = np.concatenate([[0], np.cumsum(line_len, dtype=np.int64)]).astype(np.int32)
    ioff = np.concatenate([[0], np.cumsum(page_len, dtype=np.int64)]).astype(np.int32)
    return q, sp, loff, ioff


def _flatten_boxes(box_groups):
    """list of (n_i,4,2) -> counts int32[N], boxes float32 (sum n_i,4,2) in image order"""
    counts = np.array([len(b) for b in box_groups], dtype=np.int32)
    flat = [np.asarray(b, dtype=np.float32).reshape(-1, 4, 2) for b in box_groups if len(b)]
    return counts, np.ascontiguousarray(np.concatenate(flat) if flat else np.zeros((0, 4, 2), np.float32))


def _box_lists(boxes, counts):
    """(n, cap, 4, 2) boxes -> per-image list of (n_i,4,2) (``np.array([])`` for an image without boxes, detection.py:286)"""
    return [boxes[i, :counts[i]].copy() if counts[i] else np.array([]) for i in range(len(counts))]


def _min_area_rect_code(rule):
    if not isinstance(rule, str) or rule not in MIN_AREA_RECT_RULES:
        raise ValueError(f"min_area_rect must be one of {sorted(MIN_AREA_RECT_RULES)}, got {rule!r}")
    return MIN_AREA_RECT_RULES[rule]


_default_ctx = None


def default_context():
    """The process-wide context: HIP device LOCAL_RANK (one process per GPU) or 0."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(int(os.environ.get("LOCAL_RANK", "0")))
    return _default_ctx
