"""The statement of tiled pages ("Tiled pages"; include/kocr.h, "tiled pages") in numpy: the tile
plan, the two copies, and the tiled detector pass and pipeline composed from the CPU oracle.  TEST INFRASTRUCTURE ONLY.

The plan, with tile T and overlap O in detector-input pixels (T a multiple of 32, T >= 64; O a multiple of 16, O >= 0;
stride S = T - 2 O >= 32), per axis of length d >= 1:
  n = 1 if d <= T else ceil((d - T) / S) + 1;  origin_k = k S;  canvas = (n - 1) S + T;
  core_k = [origin_k + (O if k > 0 else 0), origin_k + T - (O if k < n - 1 else 0)).
A tile's 2-D core is the product of its axis cores; tiles are numbered row-major."""
import collections
import functools
import math

import numpy as np

Plan = collections.namedtuple("Plan", "tile overlap stride counts canvas origins cores")


def axis_plan(d, tile, overlap):
    """(n, origins, cores) of one axis"""
    stride = tile - 2 * overlap
    n = 1 if d <= tile else math.ceil((d - tile) / stride) + 1
    origins = [k * stride for k in range(n)]
    cores = [(o + (overlap if k > 0 else 0), o + tile - (overlap if k < n - 1 else 0)) for k, o in enumerate(origins)]
    return n, origins, cores


def plan(height, width, tile, overlap):
    if tile % 32 or tile < 64 or overlap % 16 or overlap < 0 or tile - 2 * overlap < 32 or height < 1 or width < 1:
        raise ValueError((height, width, tile, overlap))
    (ny, oy, cy), (nx, ox, cx) = axis_plan(height, tile, overlap), axis_plan(width, tile, overlap)
    stride = tile - 2 * overlap
    return Plan(tile, overlap, stride, (ny, nx), ((ny - 1) * stride + tile, (nx - 1) * stride + tile),
                [(y, x) for y in oy for x in ox], [(y0, y1, x0, x1) for y0, y1 in cy for x0, x1 in cx])


def gather(canvas, p):
    """canvas (Hc, Wc, C) -> tiles (nT, T, T, C), a copy"""
    assert canvas.shape[:2] == p.canvas
    return np.stack([canvas[y:y + p.tile, x:x + p.tile] for y, x in p.origins])


def stitch(tiles, p, shrink=1):
    """tiles (nT, T / shrink, T / shrink, C), maps of the tiles at 1 / shrink of their resolution -> the canvas' map
    (Hc / shrink, Wc / shrink, C): every pixel from the one tile whose core contains it"""
    t = p.tile // shrink
    assert tiles.shape[:3] == (len(p.origins), t, t)
    out = np.empty((p.canvas[0] // shrink, p.canvas[1] // shrink) + tiles.shape[3:], tiles.dtype)
    for tile, (oy, ox), (y0, y1, x0, x1) in zip(tiles, p.origins, p.cores):
        oy, ox, y0, y1, x0, x1 = (v // shrink for v in (oy, ox, y0, y1, x0, x1))
        out[y0:y1, x0:x1] = tile[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
    return out


def canvas_of(resized_page, p):
    """tools.pad's 255 on the right and at the bottom, up to the plan's canvas"""
    from oracle import tools as otools

    return otools.pad(resized_page, width=p.canvas[1], height=p.canvas[0])


def tiled_heat(weights, resized_page, tile, overlap):
    """The heat-map (Hc / 2, Wc / 2, 2) of a resized page read in tiles by the oracle's detector, and the canvas"""
    from oracle import craft as ocraft

    p = plan(resized_page.shape[0], resized_page.shape[1], tile, overlap)
    canvas = canvas_of(resized_page, p)
    return stitch(ocraft.detector_predict(weights, gather(canvas, p)), p, shrink=2), canvas


def resize(page, scale):
    """The page as recognize_tiled resizes it: int(h scale) x int(w scale), no max_size"""
    from oracle import tools as otools

    return otools.cv_resize_linear_u8(page, (int(page.shape[1] * scale), int(page.shape[0] * scale)))


def recognize_tiled(craft_w, crnn_w, page, scale, tile, overlap, heat_out=None):
    """One page -> [(text, box in input-image pixels)]; ``heat_out`` (a list) receives the stitched heat-map"""
    from oracle import pipeline as opipe, postproc as opost, tools as otools

    heat, canvas = tiled_heat(craft_w, resize(page, scale), tile, overlap)
    if heat_out is not None:
        heat_out.append(heat)
    boxes = opost.get_boxes(heat[None])[0]
    texts = opipe.recognize_from_boxes(crnn_w, [canvas], [boxes])[0]
    boxes = otools.adjust_boxes(boxes=boxes, scale=1 / scale) if scale != 1 else boxes
    return list(zip(texts, boxes))


def crosses_seam(box, p):
    """A box (4, 2) in canvas pixels has pixels in more than one core: an interior core edge lies strictly inside its extent"""
    box = np.asarray(box, np.float64)
    xs = sorted({x0 for _, _, x0, _ in p.cores} - {0})
    ys = sorted({y0 for y0, _, _, _ in p.cores} - {0})
    return any(box[:, 0].min() < e < box[:, 0].max() for e in xs) or any(box[:, 1].min() < e < box[:, 1].max() for e in ys)


# (page arguments of synth.text_page, scale, tile, overlap): tests/test_tiling_statement_cpu.py asserts what they contain
FIXTURES = {"A": ((80, 120, 8, 25), 2, 64, 16), "B": ((96, 128, 8, 22), 2, 128, 32)}
Fixture = collections.namedtuple("Fixture", "page scale tile overlap plan weights heat canvas want")


@functools.lru_cache(maxsize=None)
def fixture(name):
    """The fixture's page, the detector weights calibrated on its own tiled oracle heat-map (so that the random-init network
    emits word boxes), that heat-map under the calibrated weights, the canvas, and the oracle's answer (computed once)"""
    import keras_ocr_amd
    from tests import synth

    (h, w, words, seed), scale, tile, overlap = FIXTURES[name]
    page = synth.text_page(h, w, words, seed=seed)
    raw = keras_ocr_amd.weights.synthetic_craft_weights(1234)
    crnn_w = keras_ocr_amd.weights.synthetic_crnn_weights(4321)
    heat, _ = tiled_heat(raw, resize(page, scale), tile, overlap)
    weights = keras_ocr_amd.weights.calibrate_craft_head(raw, heat[None], text_frac=0.10, link_frac=0.04)
    heats = []
    want = recognize_tiled(weights, crnn_w, page, scale, tile, overlap, heat_out=heats)
    resized = resize(page, scale)
    p = plan(resized.shape[0], resized.shape[1], tile, overlap)
    return Fixture(page, scale, tile, overlap, p, weights, heats[0], canvas_of(resized, p), want)
