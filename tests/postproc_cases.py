"""Heat-maps that sit on the edges of the heat-map -> boxes kernels (csrc/postproc.hip, K1 - K12 and the error path), shared by
tests/test_postproc_edges_cpu.py (which anchors the oracle at them by hand) and tests/test_postproc_edges_gpu.py (which holds
the kernels to the oracle).  Plain numpy, every seed fixed.

A case is a dict: ``name``; ``heat`` (N, h, w, 2) float32, read-only; ``kwargs`` for get_boxes; ``expect`` -- "boxes" or
"index_error"; ``aims`` -- the kernel line it is there for; and what can be said about it by hand, independently of
oracle/postproc.py: ``counts`` (boxes per image), ``comps`` (per image, the kept components in label order as
(area, x, y, w, h) of their bounding boxes) and ``extents`` (per image, (l, t, r, b) in map pixels of the chosen fragment after
the dilation, for the cases whose box is the axis-parallel rectangle [[l, t], [r, t], [r, b], [l, b]] * 2) or ``corners`` where
it is not.  Heat values are 0 or 1 and the link map is zero unless the case says otherwise.

The hand rules (detection.py:258-264): niter = int(sqrt(area * min(w, h) / (w * h)) * 2); the ROI is the bounding box grown
by niter to the left and above and by niter + 1 to the right and below (exclusive end), clipped to the map; the dilation
kernel has k = 1 + niter taps with anchor k // 2, so a pixel spreads k - 1 - k // 2 to the left / up and k // 2 to the right /
down: for even k one pixel further right and down."""
import functools
import math

import numpy as np

F32 = np.float32
NAN_POSITIVE, NAN_NEGATIVE = 0x7FC00000, 0xFFC00000


def niter_of(area, w, h):
    return int(math.sqrt(area * min(w, h) / (w * h)) * 2)


def roi_of(comp, W, H):
    """(sx, sy, ex, ey) of detection.py:259-260 for a component (area, x, y, w, h) on a W x H map"""
    area, x, y, w, h = comp
    n = niter_of(area, w, h)
    return max(x - n, 0), max(y - n, 0), min(x + w + n + 1, W), min(y + h + n + 1, H)


def grown(comp, W, H):
    """(l, t, r, b) of a FILLED w x h rectangle after its own dilation, clipped to the map"""
    area, x, y, w, h = comp
    k = 1 + niter_of(area, w, h)
    a = k // 2
    return max(x - (k - 1 - a), 0), max(y - (k - 1 - a), 0), min(x + w - 1 + a, W - 1), min(y + h - 1 + a, H - 1)


def rect_box(extent):
    l, t, r, b = extent
    return F32(2) * np.array([[l, t], [r, t], [r, b], [l, b]], F32)


def _heat(text, link=None):
    text = np.asarray(text, F32)
    if text.ndim == 2:
        text = text[None]
    link = np.zeros_like(text) if link is None else np.asarray(link, F32).reshape(text.shape)
    y = np.ascontiguousarray(np.stack([text, link], -1))
    y.flags.writeable = False
    return y


def _case(name, heat, aims, expect="boxes", counts=None, comps=None, extents=None, corners=None, **kwargs):
    return dict(name=name, heat=heat, kwargs=kwargs, expect=expect, aims=aims, counts=counts, comps=comps, extents=extents,
                corners=corners)


def _from_rects(name, shape, rects, aims, value=1.0, **kwargs):
    """A case of filled rectangles (y0, y1, x0, x1) per image that never touch: every rectangle is one component; its label
    is its rank by (y0, x0), its bounding box is itself and its box is its grown extent."""
    n, h, w = shape
    text = np.zeros(shape, F32)
    comps, extents = [], []
    for i, rs in enumerate(rects):
        rs = sorted(rs, key=lambda r: (r[0], r[2]))
        for y0, y1, x0, x1 in rs:
            text[i, y0:y1, x0:x1] = value
        comps.append([((y1 - y0) * (x1 - x0), x0, y0, x1 - x0, y1 - y0) for y0, y1, x0, x1 in rs])
        extents.append([grown(c, w, h) for c in comps[-1]])
    return _case(name, _heat(text), aims, counts=[len(c) for c in comps], comps=comps, extents=extents, **kwargs)


def _nan(bits):
    return np.array([bits], np.uint32).view(F32)[0]


# ---------------------------------------------------------------------------------------------------------------------
def _pixel_grid():
    # k_boxes: 9216 components > the 8192 workgroups of grid_for(ncomp, 1), so a workgroup takes a second component and
    # reuses hull_s / cand_s behind one __syncthreads().  k_assign: 32 kept roots in every ballot of the even rows.  The
    # binding's default cap of 1024 overflows: its retry runs.  Every ROI holds its neighbours' pixels (label == root).
    return _from_rects("pixel_grid", (1, 192, 192), [[(y, y + 1, x, x + 1) for y in range(0, 192, 2) for x in range(0, 192, 2)]],
                       "k_boxes: ncomp > gridDim; k_assign: 32 roots per ballot; the cap retry", size_threshold=1)


def _square_grid():
    # k_geometry: 500 components = two 256-chunks; the second starts inside image 0 (component 256) and ends in image 2, so
    # s_cbase / s_rbase carry over and the image binary search (img_base = [0, 400, 400, 500]) crosses the empty image 1.
    def sq(cols):
        return [(6 * gy, 6 * gy + 4, 6 * gx, 6 * gx + 4) for gy in range(20) for gx in range(cols)]
    return _from_rects("square_grid", (3, 120, 120), [sq(20), [], sq(5)],
                       "k_geometry: the carry into the second 256-chunk; the image search across an empty image")


def _seams():
    # k_merge4: x > 0 and (i / w) % h > 0 are all that keep pixel (y, 7) from merging with (y + 1, 0), and the last row of
    # image 0 from merging with the first of image 1 (both columns are foreground on either side of both seams).
    return _from_rects("seams", (2, 6, 8), [[(0, 6, 0, 1), (0, 6, 7, 8)]] * 2, "k_merge4: the row seam and the image seam",
                       size_threshold=1)


def _all_foreground():
    # one component per image, its ROI clipped on all four sides; 1 x 1 is a hull of one point, 1 x W and H x 1 of two
    out = []
    for n, h, w in ((2, 33, 31), (1, 1, 1), (1, 1, 37), (1, 41, 1), (1, 2, 2)):
        c = _from_rects(f"all_foreground_{h}x{w}", (n, h, w), [[(0, h, 0, w)]] * n,
                        "the ROI clipped on four sides; hulls of one and two points", size_threshold=1)
        if h == 1 and w > 1:
            # a horizontal segment: boxPoints of a rectangle without height lists each end point twice (OpenCV's n == 2
            # case), [[0, 0], [0, 0], [w - 1, 0], [w - 1, 0]] -- the same corner set as the closed form of a w x 1 rectangle,
            # listed in another order.  (On H x 1 the two orders coincide.)
            c["extents"] = None
            c["corners"] = [[F32(2) * np.array([[0, 0], [0, 0], [w - 1, 0], [w - 1, 0]], F32)]]
        out.append(c)
    return out


def _block_edges():
    # bpi = ceil(h * w / 1024): maps one pixel short of a compaction block, exactly one block, one pixel into the second and
    # one pixel into the third.  Two images each, so that image 1's pixels start at a global index that is no multiple of
    # 1024 (blocks are per image).  Every map has a 2 x 5 block that ends on its last pixel.
    out = []
    for h, w in ((33, 31), (32, 32), (25, 41), (3, 683)):
        first, last = (0, 2, 0, 5), (h - 2, h, w - 5, w)
        kw = {}
        if (h, w) == (25, 41):
            # pixel 1023 = (24, 39) is the last of block 0 and 1024 = (24, 40) the only pixel of block 1: no 2 x 5 block can
            # have its raster-first pixel there, so a 1 x 2 component stands in, rooted on the last pixel of block 0 with
            # the rest of it in block 1 (size_threshold 1); the 2 x 5 block that would end on the last pixel moves up
            rects = [first, (20, 22, 36, 41), (24, 25, 39, 41)]
            kw["size_threshold"] = 1
        elif (h, w) == (3, 683):
            # pixel 1023 = (1, 340): the raster-first pixel of the middle block is the last pixel of compaction block 0 and
            # its other nine pixels are in blocks 1 and 2; the last block's final pixel, 2048, is alone in block 2.  `first`
            # would touch nothing but sits in rows 0 - 1 like the others: keep it away from them in x
            rects = [first, (1, 3, 340, 345), last]
        else:
            rects = [first, last]
        extra = (0, 2, 10, 15)  # image 1 has one block more, so the two images' counts differ
        out.append(_from_rects(f"block_edges_{h}x{w}", (2, h, w), [rects, rects + [extra]],
                               "k_count / k_assign: bpi boundaries, a root on the last pixel of a block", **kw))
    return out


def _equalities():
    # k_threshold: strict > text_threshold; comp_kept: area >= size_threshold, max >= detection_threshold (both kept AT equality)
    t = np.zeros((30, 30), F32)
    t[2:4, 2:7] = F32(0.7)                            # max == detection_threshold: kept
    t[2:4, 12:17] = np.nextafter(F32(0.7), F32(0))    # one ulp below: dropped
    t[8:10, 2:6] = 1.0                                # area 8: dropped
    t[14, 2:11] = 1.0                                 # area 9 == size_threshold - 1: dropped ...
    t[14, 11:15] = F32(0.4)                           # ... and would be 13 if a pixel AT text_threshold were foreground
    comp = (10, 2, 2, 5, 2)
    return _case("equalities", _heat(t), "k_threshold: strict >; comp_kept: >= at equality", counts=[1], comps=[[comp]],
                 extents=[[grown(comp, 30, 30)]])


def _even_kernel_corners():
    # area 9, 3 x 3: niter = 3, k = 4, anchor 2: one pixel left / up, two right / down (k_dilate_h / k_dilate_v: x0 = lx - a,
    # x1 = lx + k - 1 - a on the SOURCE side).  The corner squares' ROIs and dilations are clipped by the map.
    r = [(0, 3, 0, 3), (0, 3, 9, 12), (4, 7, 4, 7), (9, 12, 0, 3), (9, 12, 9, 12)]
    return _from_rects("even_kernel_corners", (1, 12, 12), [r], "k_dilate_h / k_dilate_v: even k, ROI clipped at the corners",
                       size_threshold=1)


def _big_kernel_corner():
    # 40 x 40 square: niter = 12, k = 13, ROI clipped above and left.  The issue's 3 x 30 bar can be clipped at two borders of
    # a 64-wide map only (k = 4 reaches 3 pixels); a 3 x 60 bar on the bottom rows is clipped left, right and below.
    return _from_rects("big_kernel_corner", (1, 64, 64), [[(0, 40, 0, 40), (61, 64, 2, 62)]],
                       "k = 13 with the ROI clipped at two borders; k = 4 clipped at three")


def _splits():
    # K10 / K11: text AND link cuts the bar in two pieces 30 pixels apart, which k = 5 cannot close; findContours lists the
    # piece whose raster-first pixel comes last: the right one, the lower one, and a single pixel at the lower right.
    t = np.zeros((40, 100), F32)
    t[15:21, 20:80] = 1.0
    l = np.zeros_like(t)
    l[15:21, 35:65] = 1.0
    comp = (360, 20, 15, 60, 6)  # niter 4
    side = _case("split_side_by_side", _heat(t, l), "k_flatten_select: atomicMax over fragment roots, pieces side by side",
                 counts=[1], comps=[[comp]], extents=[[(63, 13, 81, 22)]])
    stacked = _case("split_stacked", _heat(t.T, l.T), "k_flatten_select: pieces one above the other", counts=[1],
                    comps=[[(360, 15, 20, 6, 60)]], extents=[[(13, 63, 22, 81)]])
    l2 = np.zeros_like(t)
    l2[15:21, 35:80] = 1.0
    l2[20, 79] = 0.0  # the piece that is left at the lower right is one pixel; dilated it is 5 x 5
    tiny = _case("split_last_is_tiny", _heat(t, l2), "k_flatten_select: the last piece is a single pixel", counts=[1],
                 comps=[[comp]], extents=[[(77, 18, 81, 22)]])
    return [side, stacked, tiny]


def _snake():
    # one 1-pixel-wide path of 8414 pixels whose raster-first pixel (0, 100) is one END of it: the longest union-find chain
    # the suite has (uf_union / uf_find across every workgroup of k_merge4), and the label every pixel must reach
    t = np.zeros((129, 130), F32)
    t[0::2] = 1.0
    t[1::4, 129] = 1.0
    t[3::4, 0] = 1.0
    t[0, :100] = 0.0
    comp = (65 * 130 - 100 + 64, 0, 0, 130, 129)
    return _case("snake", _heat(t), "k_merge4 / k_flatten_stats: one long chain", counts=[1], comps=[[comp]],
                 extents=[[(0, 0, 129, 128)]])


def _ring_and_core():
    # labels go by raster-first pixel: the ring (5, 5) before the block inside it, though most of the ring comes later.  The
    # ring's ROI holds every pixel of the block: k_canvas_fill's label == root must leave them out, or the block would be
    # the ring's last fragment.
    t = np.zeros((40, 40), F32)
    t[5:35, 5:35] = 1.0
    t[6:34, 6:34] = 0.0
    t[15:25, 15:25] = 1.0
    ring, core = (116, 5, 5, 30, 30), (100, 15, 15, 10, 10)
    # the ring is no filled rectangle but its outline dilates like one: k = 4 -> 4 .. 36
    return _case("ring_and_core", _heat(t), "k_assign: label order; k_canvas_fill: label == root", counts=[2],
                 comps=[[ring, core]], extents=[[(4, 4, 36, 36), grown(core, 40, 40)]])


_BLOCK = (50, 5, 5, 10, 5)  # the 5 x 10 link block of the cases below: niter 4


def _link_block(name, text_inside, aims, special=None, text_outside=-1.0, **kwargs):
    t = np.full((20, 20), text_outside, F32)
    l = np.zeros_like(t)
    t[5:10, 5:15] = text_inside
    l[5:10, 5:15] = 1.0
    if special is not None:
        t[7, 9] = special
    return _case(name, _heat(t, l), aims, counts=[1], comps=[[_BLOCK]], extents=[[grown(_BLOCK, 20, 20)]], **kwargs)


def _float_key_cases():
    return [
        # fg = text OR link: no pixel of the component is over text_threshold but one, which is text AND link and leaves the
        # segmap; the maximum is taken over the text values of LINK pixels: 0.9
        _link_block("link_only", -1.0, "k_threshold: fg = text OR link; k_flatten_stats: max over link pixels", special=0.9,
                    text_outside=0.0, link_threshold=0.4),
        # np.max gives -0.0 and -0.0 < 0.0 is false: kept.  float_key(-0.0) = -1 < float_key(+0.0) = 0
        _link_block("signed_zero_max", -0.0, "comp_kept: float_key(-0.0) against float_key(+0.0)", detection_threshold=0.0),
        # np.max propagates a NaN of either sign and NaN < 0.0 is false: kept
        _link_block("nan_in_text_positive", -1.0, "float_key of a NaN, sign bit clear", special=_nan(NAN_POSITIVE),
                    detection_threshold=0.0),
        _link_block("nan_in_text_negative", -1.0, "float_key of a NaN, sign bit set", special=_nan(NAN_NEGATIVE),
                    detection_threshold=0.0),
        # max < NaN is false whatever the maximum: kept
        _link_block("nan_detection_threshold", 0.25, "comp_kept: a NaN detection_threshold rejects nothing",
                    detection_threshold=float("nan")),
    ]


def _negative_thresholds():
    # every pixel is foreground and float_key sees negative values: image 0's maximum is positive, image 1's is negative.
    # With the zero link map of the issue's table every pixel would be text AND link (0 > -1) and the call would raise (that
    # map is `negative_thresholds_link_zero` below); the link map is -2 here, under its threshold.
    rng = np.random.default_rng(16)
    v = rng.uniform(-0.5, 0.5, (16, 16)).astype(F32)
    t = np.stack([v, -np.abs(v) - F32(0.001)])
    comp = (256, 0, 0, 16, 16)
    boxes = _case("negative_thresholds", _heat(t, np.full_like(t, -2.0)), "float_key of negative values; a negative maximum",
                  counts=[1, 1], comps=[[comp], [comp]], extents=[[(0, 0, 15, 15)]] * 2, detection_threshold=-1.0,
                  text_threshold=-1.0, link_threshold=-1.0, size_threshold=1)
    raises = _case("negative_thresholds_link_zero", _heat(v), "k_boxes: sel < 0 for a component that is the whole map",
                   expect="index_error", detection_threshold=-1.0, text_threshold=-1.0, link_threshold=-1.0, size_threshold=1)
    return [boxes, raises]


def _empty_contours():
    # k_boxes: sel < 0 -> totals[2] -> KOCR_EEMPTYCONTOUR -> IndexError (detection.py:272)
    t = np.zeros((40, 40), F32)
    t[10:20, 10:30] = 1.0
    alone = _case("empty_contour_alone", _heat(t, t), "k_boxes: sel < 0", expect="index_error")
    # image 0: one word; image 1: a word, the text AND link block, a word -- in raster order of their first pixels
    t2 = np.zeros((2, 40, 60), F32)
    l2 = np.zeros_like(t2)
    t2[0, 5:10, 5:25] = 1.0
    t2[1, 3:8, 4:24] = 1.0
    t2[1, 15:21, 20:40] = 1.0
    l2[1, 15:21, 20:40] = 1.0
    t2[1, 30:35, 30:55] = 1.0
    among = _case("empty_contour_among_valid", _heat(t2, l2), "k_boxes: sel < 0 between two valid components",
                  expect="index_error")
    return [alone, among]


@functools.lru_cache(maxsize=None)
def cases():
    out = [_pixel_grid(), _square_grid(), _seams()] + _all_foreground() + _block_edges()
    out += [_equalities(), _even_kernel_corners(), _big_kernel_corner()] + _splits() + [_snake(), _ring_and_core()]
    out += _float_key_cases() + _negative_thresholds() + _empty_contours()
    assert len({c["name"] for c in out}) == len(out)
    return tuple(out)


def names(expect=None, multi_image=False):
    return [c["name"] for c in cases() if (expect is None or c["expect"] == expect) and (not multi_image or len(c["heat"]) > 1)]


def case(name):
    return next(c for c in cases() if c["name"] == name)


def without_link(heat):
    """the same maps with the link map under every threshold: what the index_error cases become valid with"""
    y = np.array(heat)
    y[..., 1] = -np.inf
    return y


def expected_boxes(c):
    """the hand-derived boxes of a case, per image (None where the case states none)"""
    if c["corners"] is not None:
        return [np.array(g) if len(g) else np.array([]) for g in c["corners"]]
    if c["extents"] is None:
        return None
    return [np.array([rect_box(e) for e in g]) if len(g) else np.array([]) for g in c["extents"]]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(boxes, debug) of oracle.postproc.get_boxes on a "boxes" case: computed once, shared by the tests, never modified"""
    from oracle import postproc

    c = case(name)
    return postproc.get_boxes(c["heat"], return_debug=True, **c["kwargs"])


def rule_statements(want, dbg):
    """(exact boxes, cv32 boxes, per-component max corner deviation between the two) from the (boxes, debug) of the oracle's
    getBoxes: every component's box rebuilt from its hull under either min-area-rectangle rule.  The hull's extremes are the
    fragment's, which is all the diamond rule reads."""
    from oracle import postproc

    exact, cv32, dev = [], [], []
    for boxes, comps in zip(want, dbg):
        e, c = [], []
        for comp in comps:
            hull = comp["hull"]
            hx, hy = np.array([p[0] for p in hull]), np.array([p[1] for p in hull])
            e.append(postproc.box_from_hull(hull, hx, hy, cv32=False))
            c.append(postproc.box_from_hull(hull, hx, hy, cv32=True))
            dev.append(float(np.abs(e[-1] - c[-1]).max()))
        assert len(e) == len(boxes) and all(np.array_equal(a, b) for a, b in zip(e, boxes))
        exact.append(np.array(e) if e else np.array([]))
        cv32.append(np.array(c) if c else np.array([]))
    return exact, cv32, np.array(dev)


@functools.lru_cache(maxsize=None)
def statements(name):
    """rule_statements of a "boxes" case, computed once"""
    return rule_statements(*oracle(name))
