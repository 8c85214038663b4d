"""What tests/test_w43h_bits_gpu.py and tests/golden/make_w43h_bits.py share: the cases that reach every K-loop form of the
fp16 F(4,3) kernels (csrc/conv_w43h.hip) and the digests of what the library writes for them.

The kernels' input transform may be rescheduled or re-selected (scalar against packed fp32 instructions) but its roundings
are part of the arithmetic the project states: the outputs and the per-image max-|x| slots are held bit for bit against
digests recorded with an earlier build of the library (tests/golden/w43h_bits.json).

    single layers   every row of dispatch_cases.DEFAULT that runs conv_w4hv* / conv_w4ht* / conv_w4hr* / conv_w4hf*, the
                    conv_w4q* rows of dispatch_cases.F16X1 in that mode (inputs of dispatch_cases.problem: IMAGE_SCALES
                    applied, the scale is folded into the transform's constants), and two shapes that make two and four
                    trips through the unrolled loop body with two images;
    CRAFT           every tap of two 128 x 128 pages (levels 128 / 64 / 32 / 16 / 8: the 64-cout kernel pooled, the wide one
                    pooled and plain, 8 x 32 tiles, flattened tiles, the dilated composite) and of one 100 x 140 page (ragged);
    recogniser      every tap of 17 crops (a second, ragged row of cells: conv_2 .. conv_7, both poolings).
"""
import hashlib

import numpy as np

from tests import batch_edge_cases as bec
from tests import dispatch_cases as dc
from tests import synth

LOOP_TRIPS = [(1, 4, 64, 128, 128, 3, 1), (2, 8, 64, 64, 128, 3, 1)]
_ROWS = ("conv_w4hv", "conv_w4ht", "conv_w4hr", "conv_w4hf")
SINGLE_DEFAULT = [c for c, row in dc.DEFAULT if row.startswith(_ROWS)] + LOOP_TRIPS
SINGLE_F16X1 = [c for c, row in dc.F16X1 if row.startswith("conv_w4q")]
CRAFT_PAGES = {"2x128x128": (2, 128, 128), "1x100x140": (1, 100, 140)}
N_CROPS = 17


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is None:
            h.update(b"<none>")
        else:
            a = np.ascontiguousarray(a)
            h.update(repr((a.shape, a.dtype.str)).encode())
            h.update(a.tobytes())
    return h.hexdigest()


def _tap_digests(taps):
    """{tap: {"kernel": rows, "out": digest of (data, slots), "pool": ...}} of what a forward recorded"""
    out = {}
    for name, t in taps.items():
        rec = {"kernel": t["kernel"]}
        for key in ("out", "pool"):
            rec[key] = None if t[key] is None else _sha(t[key][0], t[key][1])
        out[name] = rec
    return out


def _single(ctx, case):
    p = dc.problem(case)
    ctx.profile_enable(True)
    ctx.profile_reset()
    try:
        got = ctx.conv2d_nhwc(p["x"], p["w"], dilation=case[6], pre_a=p["pre_a"], pre_b=p["pre_b"], relu=True)
        rows = sorted(k for k in ctx.profile_report() if k.startswith("conv"))
    finally:
        ctx.profile_enable(False)
    return {"kernel": "+".join(rows), "out": _sha(got)}


def pages(key):
    n, h, w = CRAFT_PAGES[key]
    return np.stack([synth.text_page(h, w, 3, seed=h * w + i, scale=0.4) for i in range(n)])


def digests(ctx, craft_weights, crnn_weights):
    """Everything the fixture holds, computed with the library behind `ctx` (the split mode is put back)."""
    out = {"single": {}, "single_f16x1": {}, "craft": {}, "crnn": {}}
    prev = ctx.get_split_mode()
    try:
        ctx.set_split_mode("f16x2")
        for case in SINGLE_DEFAULT:
            out["single"][dc.case_id(case)] = _single(ctx, case)
        ctx.set_split_mode("f16x1")
        for case in SINGLE_F16X1:
            out["single_f16x1"][dc.case_id(case)] = _single(ctx, case)
        ctx.set_split_mode("f16x2")
        ctx.load_craft(craft_weights)
        ctx.craft_set_taps(["*"])
        try:
            for key in CRAFT_PAGES:
                heat = ctx.craft_forward(pages(key))
                rec = _tap_digests(ctx.craft_taps())
                rec["<heat>"] = {"kernel": "", "out": _sha(heat), "pool": None}
                out["craft"][key] = rec
        finally:
            ctx.craft_set_taps([])
        ctx.load_crnn(crnn_weights)
        ctx.crnn_set_taps(["*"])
        try:
            labels, probs = ctx.crnn_forward(bec.crops(N_CROPS), return_probs=True)
            rec = _tap_digests(ctx.crnn_taps())
            rec["<labels, probs>"] = {"kernel": "", "out": _sha(labels, probs), "pool": None}
            out["crnn"][str(N_CROPS)] = rec
        finally:
            ctx.crnn_set_taps([])
    finally:
        ctx.set_split_mode(prev)
    return out
