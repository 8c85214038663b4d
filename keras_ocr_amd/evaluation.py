"""Mirror of ``keras_ocr.evaluation`` (reference ``keras_ocr/evaluation.py:13-147``): polygon IoU and
precision/recall scoring of pipeline output.  SURVEY.md §8(f) item 4.  Two paths: the host one, pure
numpy/Python, where pyclipper, cv2.contourArea and editdistance are re-stated (simple polygons
are triangulated by ear clipping and intersected triangle by triangle with Sutherland-Hodgman); and, with
``ctx``, the same rule for 2- and 4-corner boxes on the GPU (kocr_score: DESIGN.md section 4, "Evaluation")."""
import typing
import warnings

import numpy as np


def _area2(poly):
    x, y = poly[:, 0], poly[:, 1]
    return float(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def _ccw(poly):
    return poly if _area2(poly) > 0 else poly[::-1]


def _triangulate(poly):
    """Ear clipping of a simple polygon (counter-clockwise) -> list of (3,2) triangles."""
    pts = [tuple(map(float, p)) for p in _ccw(np.asarray(poly, dtype=np.float64))]
    pts = [p for i, p in enumerate(pts) if p != pts[i - 1]]
    tris = []

    def cross(o, a, b):
        return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])

    guard = 0
    while len(pts) > 3 and guard < 10000:
        guard += 1
        n = len(pts)
        for i in range(n):
            a, b, c = pts[i - 1], pts[i], pts[(i + 1) % n]
            if cross(a, b, c) <= 0:
                continue  # reflex or degenerate corner
            if any(cross(a, b, q) >= 0 and cross(b, c, q) >= 0 and cross(c, a, q) >= 0
                   for q in pts if q not in (a, b, c)):
                continue
            tris.append(np.array([a, b, c]))
            del pts[i]
            break
        else:
            break  # numerically degenerate: stop with what is left
    if len(pts) == 3:
        tris.append(np.array(pts))
    return tris


def _clip_convex(subject, clip):
    """Sutherland-Hodgman: subject polygon clipped by a CONVEX counter-clockwise clip polygon."""
    out = [tuple(p) for p in subject]
    n = len(clip)
    for i in range(n):
        a, b = clip[i], clip[(i + 1) % n]
        inp, out = out, []
        if not inp:
            break

        def inside(p):
            return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) >= 0

        def inter(p, q):
            d1 = (b[0] - a[0], b[1] - a[1])
            d2 = (q[0] - p[0], q[1] - p[1])
            den = d1[0] * d2[1] - d1[1] * d2[0]
            t = ((p[0] - a[0]) * d2[1] - (p[1] - a[1]) * d2[0]) / den
            return (a[0] + t * d1[0], a[1] + t * d1[1])

        s = inp[-1]
        for e in inp:
            if inside(e):
                if not inside(s):
                    out.append(inter(s, e))
                out.append(e)
            elif inside(s):
                out.append(inter(s, e))
            s = e
    return np.array(out, dtype=np.float64) if len(out) >= 3 else None


def iou_score(box1, box2):
    """evaluation.iou_score (evaluation.py:13-53): IoU of two polygons given as lists of (x, y);
    a 2-point box is an axis-aligned (x1,y1),(x2,y2) rectangle; coordinates are truncated to int32
    like the reference does before clipping."""
    if len(box1) == 2:
        (x1, y1), (x2, y2) = box1
        box1 = np.array([[x1, y1], [x2, y1], [x2, y2], [x1, y2]])
    if len(box2) == 2:
        (x1, y1), (x2, y2) = box2
        box2 = np.array([[x1, y1], [x2, y1], [x2, y2], [x1, y2]])
    p1 = np.array(box1, dtype="int32").astype(np.float64)
    p2 = np.array(box2, dtype="int32").astype(np.float64)
    a1, a2 = abs(_area2(p1)) / 2, abs(_area2(p2)) / 2
    if a1 == 0 or a2 == 0:
        warnings.warn("A box with zero area was detected.")
        return 0
    intersection = 0.0
    for t1 in _triangulate(p1):
        for t2 in _triangulate(p2):
            c = _clip_convex(_ccw(t1), _ccw(t2))
            if c is not None:
                intersection += abs(_area2(c)) / 2
    union = a1 + a2 - intersection
    return intersection / union


def _edit_distance(a, b):
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def _text_similarity(a, b):
    """1 - normalised Levenshtein distance (evaluation.py:119-127); two empty strings are identical."""
    longest = max(len(a), len(b))
    return 1 if longest == 0 else 1 - _edit_distance(a, b) / longest


def _int_quad(box, image_id, kind, index):
    """A 2- or 4-point box as iou_score takes it: the (4, 2) int32 array it hands to the clipper."""
    if len(box) == 2:
        (x1, y1), (x2, y2) = box
        box = np.array([[x1, y1], [x2, y1], [x2, y2], [x1, y2]])
    quad = np.array(box, dtype="int32")
    if quad.shape != (4, 2):
        raise ValueError(f"image {image_id!r}, {kind} {index}: the device path takes boxes of 2 or 4 corners, got vertices of "
                         f"shape {quad.shape}")
    return quad


def _context(ctx):
    from . import _lib  # pylint: disable=import-outside-toplevel
    return _lib.default_context() if ctx is True else ctx


def iou_matrix(boxes_a, boxes_b, ctx=None):
    """iou_score of every pair of two lists of boxes of one image on the GPU (kocr_iou_table): (A, B) float64.  2-point
    and 4-point boxes, truncated to int32 exactly as iou_score does."""
    qa = [_int_quad(b, 0, "box of the first list", i) for i, b in enumerate(boxes_a)]
    qb = [_int_quad(b, 0, "box of the second list", i) for i, b in enumerate(boxes_b)]
    qa = np.array(qa, dtype=np.int32).reshape(-1, 4, 2)
    qb = np.array(qb, dtype=np.int32).reshape(-1, 4, 2)
    if _zero_area(qa).any() or _zero_area(qb).any():
        if len(qa) and len(qb):
            warnings.warn("A box with zero area was detected.")
    table = _context(True if ctx is None else ctx).iou_table(qa, [0, len(qa)], qb, [0, len(qb)])
    return table.reshape(len(qa), len(qb))


def _zero_area(quads):
    """per (n, 4, 2) int32 quad: is its shoelace area zero (exact in int64 for |coordinate| < 2^24)"""
    q = quads.astype(np.int64)
    x, y = q[:, :, 0], q[:, :, 1]
    return (x * np.roll(y, -1, axis=1) - y * np.roll(x, -1, axis=1)).sum(axis=1) == 0


def _code_points(texts, image_ids, kind):
    """texts -> (concatenated int32 code points, int32 offsets); ValueError for one over 256 code points"""
    lengths = np.fromiter((len(t) for _, _, t in texts), dtype=np.int64, count=len(texts))
    if len(lengths) and lengths.max() > 256:
        image, index, text = texts[int(np.argmax(lengths > 256))]
        raise ValueError(f"image {image_ids[image]!r}, {kind} {index}: text of {len(text)} code points, the device path takes at "
                         "most 256")
    joined = "".join(t for _, _, t in texts)
    points = np.frombuffer(joined.encode("utf-32-le", "surrogatepass"), dtype="<u4").astype(np.int32)
    return points, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


def _score_device(true, pred, iou_threshold, similarity_threshold, translator, ctx, return_results):
    """score() through one kocr_score call; the dictionaries are rebuilt from its flag arrays in the host path's order."""
    image_ids = sorted(true)
    assert all(a == b for a, b in zip(image_ids, sorted(pred))), "true and pred dictionaries must have the same keys"
    clean = (lambda t: t.translate(translator)) if translator is not None else (lambda t: t)
    quads, texts, counts, ignore = ([], []), ([], []), ([], []), []
    for n, image_id in enumerate(image_ids):
        for side, (kind, annotations) in enumerate((("truth", true[image_id]), ("prediction", pred[image_id]))):
            counts[side].append(len(annotations))
            for index, annotation in enumerate(annotations):
                quads[side].append(_int_quad(annotation["vertices"], image_id, kind, index))
                texts[side].append((n, index, annotation["text"]))
        ignore += [bool(t.get("ignore", False)) for t in true[image_id]]
    nt, npred = np.array(counts[0], np.int64), np.array(counts[1], np.int64)
    # the translator runs only where the host path runs it: it cannot be known before the IoUs which pairs those are,
    # so every text is cleaned once (a translator is a pure table lookup)
    texts = tuple([(n, i, clean(t)) for n, i, t in side] for side in texts)
    tq = np.array(quads[0], dtype=np.int32).reshape(-1, 4, 2)
    pq = np.array(quads[1], dtype=np.int32).reshape(-1, 4, 2)
    toff = np.concatenate([[0], np.cumsum(nt)]).astype(np.int32)
    poff = np.concatenate([[0], np.cumsum(npred)]).astype(np.int32)
    tt, tto = _code_points(texts[0], image_ids, "truth")
    pt, pto = _code_points(texts[1], image_ids, "prediction")
    paired = np.repeat((nt > 0) & (npred > 0), nt), np.repeat((nt > 0) & (npred > 0), npred)
    if (_zero_area(tq) & paired[0]).any() or (_zero_area(pq) & paired[1]).any():
        warnings.warn("A box with zero area was detected.")
    cls, missed, unclaimed, totals = _context(ctx).score_tables(tq, toff, pq, poff, np.array(ignore, np.uint8), tt, tto, pt, pto,
                                                                iou_threshold, similarity_threshold)
    n_tp, n_fp, n_fn = (int(v) for v in totals)
    if not return_results:
        return None, (n_tp / (n_tp + n_fp), n_tp / (n_tp + n_fn))
    results = {"true_positives": [], "false_positives": [], "near_true_positives": [], "false_negatives": []}
    pair_off = np.concatenate([[0], np.cumsum(nt * npred)])
    for key, value in (("true_positives", 1), ("near_true_positives", 2)):
        flat = np.flatnonzero(cls == value)
        image = np.searchsorted(pair_off, flat, side="right") - 1
        local = flat - pair_off[image]
        width = npred[image]
        results[key] = [{"true_idx": ti, "pred_idx": pi, "image_id": image_ids[n]}
                        for n, ti, pi in zip(image.tolist(), (local // width).tolist(), (local % width).tolist())]
    flat = np.flatnonzero(missed)
    image = np.searchsorted(toff, flat, side="right") - 1
    results["false_negatives"] = [{"image_id": image_ids[n], "true_idx": ti} for n, ti in zip(image.tolist(), (flat - toff[image]).tolist())]
    flat = np.flatnonzero(unclaimed)
    image = np.searchsorted(poff, flat, side="right") - 1
    results["false_positives"] = [{"pred_index": pi, "image_id": image_ids[n]} for n, pi in zip(image.tolist(), (flat - poff[image]).tolist())]
    return results, (n_tp / (n_tp + n_fp), n_tp / (n_tp + n_fn))


def score(true, pred, iou_threshold=0.5, similarity_threshold=0.5, translator=None, ctx=None, return_results=True):
    """evaluation.score (evaluation.py:56-147): detection + recognition precision / recall.

    ``true`` / ``pred``: ``{image_id: [{"text", "vertices"[, "ignore"]}]}`` with the same keys.  Returns
    ``(results, (precision, recall))``; ``results`` lists ``true_positives`` / ``near_true_positives`` (one entry per
    (truth, prediction) pair whose IoU reaches ``iou_threshold``, split by text similarity), ``false_negatives``
    (truths no prediction overlaps) and ``false_positives`` (predictions overlapping no truth).  An ``ignore``d truth
    absorbs the predictions it overlaps and is itself never counted.  Precision and recall count distinct matched
    truths, as the reference does (so two predictions on one truth are one true positive).

    Written as: IoU table per image -> pair classification -> bookkeeping (the reference interleaves the three).

    ``ctx`` (a ``Context``, or True for the default one) scores the whole dictionary in one GPU call and returns an equal
    value; boxes then have 2 or 4 corners and texts at most 256 code points (ValueError naming image id and annotation
    index otherwise: the host path remains for those).  Both limits hold for every annotation of the dictionaries, also
    for one that plays no part in the score (an ignored truth, a box that overlaps nothing): which texts the score needs
    is known only after the IoUs, so every text is translated and staged.  The host path translates and compares only
    the texts of overlapping pairs with a truth that is not ignored.

    ``return_results=False`` returns ``(None, (precision, recall))`` on either path; with ``ctx`` it also skips the
    assembly of the dictionary (on the host path the lists are the computation, so it saves nothing there)."""
    if ctx is not None and ctx is not False:
        return _score_device(true, pred, iou_threshold, similarity_threshold, translator, ctx, return_results)
    image_ids = sorted(true)
    assert all(a == b for a, b in zip(image_ids, sorted(pred))), "true and pred dictionaries must have the same keys"
    clean = (lambda t: t.translate(translator)) if translator is not None else (lambda t: t)
    results = {"true_positives": [], "false_positives": [], "near_true_positives": [], "false_negatives": []}
    for image_id in image_ids:
        truths, preds = true[image_id], pred[image_id]
        overlaps = [[iou_score(t["vertices"], p["vertices"]) >= iou_threshold for p in preds] for t in truths]
        for ti, (truth, row) in enumerate(zip(truths, overlaps)):
            ignored = bool(truth.get("ignore", False))
            partners = [pi for pi, hit in enumerate(row) if hit]
            if not partners:
                if not ignored:
                    results["false_negatives"].append({"image_id": image_id, "true_idx": ti})
                continue
            if ignored:
                continue
            for pi in partners:
                pair = {"true_idx": ti, "pred_idx": pi, "image_id": image_id}
                good = _text_similarity(clean(truth["text"]), clean(preds[pi]["text"])) >= similarity_threshold
                results["true_positives" if good else "near_true_positives"].append(pair)
        claimed = {pi for row in overlaps for pi, hit in enumerate(row) if hit}
        results["false_positives"] += [{"pred_index": pi, "image_id": image_id} for pi in range(len(preds)) if pi not in claimed]
    n_fn, n_fp = len(results["false_negatives"]), len(results["false_positives"])
    n_tp = len({(m["image_id"], m["true_idx"]) for m in results["true_positives"]})
    return (results if return_results else None), (n_tp / (n_tp + n_fp), n_tp / (n_tp + n_fn))
