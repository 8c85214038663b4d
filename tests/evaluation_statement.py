"""The rule keras_ocr_amd/csrc/evaluate.hip implements (kocr_iou_table / kocr_score), stated in plain Python floats with
every operation in a fixed order: IEEE float64 `+ - * /` one at a time, never fused.  The kernels carry out the same
operations in the same order, so their IoUs carry the same bits (tests/test_evaluation_gpu.py).

It restates keras_ocr_amd/evaluation.py (iou_score, score), which in turn restates the reference's evaluation.py:13-147;
the only freedom taken is the summation order of the shoelace sums, which evaluation.py leaves to np.dot.

A box is four (x, y) corners with int32 coordinates (a 2-point box is expanded by the caller, `as_quad`).  With
|coordinate| < 2^24 every product of two coordinate differences or coordinates is below 2^50 in magnitude and every sum
of up to eight of them below 2^53, so the areas of the boxes and every orientation test on their corners are exact.
Only the corners that clipping creates, and what is computed from them, are rounded.
"""

MAX_TEXT = 256  # KOCR_SCORE_MAX_TEXT


def as_quad(box):
    """2 or 4 points -> four (x, y) tuples of Python ints truncated as np.array(box, dtype="int32") truncates (toward 0)."""
    pts = [(int(x), int(y)) for x, y in box]
    if len(pts) == 2:
        (x1, y1), (x2, y2) = pts
        pts = [(x1, y1), (x2, y1), (x2, y2), (x1, y2)]
    if len(pts) != 4:
        raise ValueError(f"a box has 2 or 4 corners, got {len(pts)}")
    return pts


def area2(poly):
    """Twice the signed area: s1 = sum_i x_i y_(i+1), s2 = sum_i y_i x_(i+1), each accumulated from 0.0 in corner order
    (i + 1 wraps to 0), then s1 - s2."""
    n = len(poly)
    s1 = 0.0
    for i in range(n):
        s1 = s1 + poly[i][0] * poly[(i + 1) % n][1]
    s2 = 0.0
    for i in range(n):
        s2 = s2 + poly[i][1] * poly[(i + 1) % n][0]
    return s1 - s2


def cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def ieee_div(num, den):
    """num / den as the hardware divides (numpy scalars in evaluation.py, the kernel): a zero denominator gives +-inf or
    nan, not an exception."""
    if den != 0.0:
        return num / den
    if num != num or num == 0.0:
        return float("nan")
    negative = (num < 0.0) != (str(den)[0] == "-")
    return float("-inf") if negative else float("inf")


def triangulate_quad(quad, a2):
    """evaluation._triangulate for four corners; `a2` = area2(quad), non-zero.  Returns 0, 1 or 2 triangles.

    1. orientation: the corners as given when a2 > 0, else in reverse order (p3, p2, p1, p0);
    2. a corner equal to its predecessor (corner 0: to corner 3) is dropped; three corners left are the one triangle,
       fewer give none;
    3. four corners: the first i in 0..3 with cross(p[i-1], p[i], p[i+1]) > 0 whose ear does not contain the fourth
       corner q = p[i+2] (contained: all three of cross(a,b,q), cross(b,c,q), cross(c,a,q) >= 0) gives the triangles
       (p[i-1], p[i], p[i+1]) and the remaining three corners in their order; no such i gives none.
    A convex quad is cut at corner 0; a chevron at the first convex corner whose ear misses the reflex one."""
    p = [(float(x), float(y)) for x, y in quad]
    if not a2 > 0:
        p = p[::-1]
    kept = [p[i] for i in range(4) if p[i] != p[i - 1]]
    if len(kept) == 3:
        return [kept]
    if len(kept) < 3:
        return []
    for i in range(4):
        a, b, c, q = p[(i + 3) % 4], p[i], p[(i + 1) % 4], p[(i + 2) % 4]
        if cross(a, b, c) <= 0:
            continue
        if cross(a, b, q) >= 0 and cross(b, c, q) >= 0 and cross(c, a, q) >= 0:
            continue
        return [[a, b, c], [p[j] for j in range(4) if j != i]]
    return []


def ccw_triangle(t):
    """evaluation._ccw on a triangle: as given when area2 > 0, else reversed (c, b, a)."""
    return t if area2(t) > 0 else t[::-1]


def clip_triangle(subject, clip):
    """evaluation._clip_convex: Sutherland-Hodgman, `subject` clipped by the three edges (clip[i], clip[i+1]) in order.
    At most 3 + 3 corners come out; an empty list stays empty."""
    out = list(subject)
    for i in range(3):
        a, b = clip[i], clip[(i + 1) % 3]
        inp, out = out, []
        if not inp:
            break
        d1x = b[0] - a[0]
        d1y = b[1] - a[1]

        def inside(p):
            return d1x * (p[1] - a[1]) - d1y * (p[0] - a[0]) >= 0

        def inter(p, q):
            d2x = q[0] - p[0]
            d2y = q[1] - p[1]
            den = d1x * d2y - d1y * d2x
            t = ieee_div((p[0] - a[0]) * d2y - (p[1] - a[1]) * d2x, den)
            return (a[0] + t * d1x, a[1] + t * d1y)

        s = inp[-1]
        s_in = inside(s)
        for e in inp:
            e_in = inside(e)
            if e_in:
                if not s_in:
                    out.append(inter(s, e))
                out.append(e)
            elif s_in:
                out.append(inter(s, e))
            s, s_in = e, e_in
    return out


def iou(quad_a, quad_b):
    """IoU of two boxes of four integer corners (float64)."""
    qa = [(float(x), float(y)) for x, y in quad_a]
    qb = [(float(x), float(y)) for x, y in quad_b]
    a2a, a2b = area2(qa), area2(qb)
    area_a, area_b = abs(a2a) / 2, abs(a2b) / 2
    if area_a == 0 or area_b == 0:
        return 0.0
    tris_a = [ccw_triangle(t) for t in triangulate_quad(qa, a2a)]
    tris_b = [ccw_triangle(t) for t in triangulate_quad(qb, a2b)]
    inter = 0.0
    for ta in tris_a:
        for tb in tris_b:
            c = clip_triangle(ta, tb)
            if len(c) >= 3:
                inter = inter + abs(area2(c)) / 2
    return inter / (area_a + area_b - inter)


def levenshtein(a, b):
    """Edit distance over code points (insert, delete, substitute, each 1)."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i]
        for j in range(1, len(b) + 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1])))
        prev = cur
    return prev[-1]


def similarity(a, b):
    longest = max(len(a), len(b))
    return 1.0 if longest == 0 else 1.0 - levenshtein(a, b) / longest


def score_tables(truth_quads, truth_ignore, truth_texts, pred_quads, pred_texts, iou_threshold, similarity_threshold):
    """What kocr_score returns, image by image in the order given (evaluation.score walks sorted image ids).

    Per image i: truth_quads[i] / pred_quads[i] lists of quads, truth_ignore[i] booleans, truth_texts[i] / pred_texts[i]
    sequences of code points (the translator already applied).  Returns a dict:
      iou          per image an nt x np table of IoUs
      pair_class   per image an nt x np table: 0 iou < iou_threshold; 3 overlap with an ignored truth; otherwise 1 (true
                   positive: similarity >= similarity_threshold) or 2 (near true positive)
      truth_missed per image nt flags: not ignored and no pair of its row with iou >= iou_threshold
      pred_unclaimed per image np flags: no pair of its column with iou >= iou_threshold, ignored truths included
      counts       [truths with a class-1 pair, unclaimed predictions, missed truths] over all images
    """
    tables = {"iou": [], "pair_class": [], "truth_missed": [], "pred_unclaimed": [], "counts": [0, 0, 0]}
    for tq, ign, tt, pq, pt in zip(truth_quads, truth_ignore, truth_texts, pred_quads, pred_texts):
        ious = [[iou(t, p) for p in pq] for t in tq]
        cls = []
        for ti, row in enumerate(ious):
            crow = []
            for pi, v in enumerate(row):
                if not v >= iou_threshold:
                    crow.append(0)
                elif ign[ti]:
                    crow.append(3)
                else:
                    if len(tt[ti]) > MAX_TEXT or len(pt[pi]) > MAX_TEXT:
                        raise ValueError("text longer than KOCR_SCORE_MAX_TEXT")
                    crow.append(1 if similarity(tt[ti], pt[pi]) >= similarity_threshold else 2)
            cls.append(crow)
        missed = [int(not ign[ti] and not any(cls[ti])) for ti in range(len(tq))]
        unclaimed = [int(not any(cls[ti][pi] for ti in range(len(tq)))) for pi in range(len(pq))]
        tables["iou"].append(ious)
        tables["pair_class"].append(cls)
        tables["truth_missed"].append(missed)
        tables["pred_unclaimed"].append(unclaimed)
        tables["counts"][0] += sum(1 for crow in cls if 1 in crow)
        tables["counts"][1] += sum(unclaimed)
        tables["counts"][2] += sum(missed)
    return tables


def results_from_tables(image_ids, tables):
    """The `results` dict and (precision, recall) of evaluation.score from score_tables' output."""
    results = {"true_positives": [], "false_positives": [], "near_true_positives": [], "false_negatives": []}
    for image_id, cls, missed, unclaimed in zip(image_ids, tables["pair_class"], tables["truth_missed"], tables["pred_unclaimed"]):
        for ti, crow in enumerate(cls):
            if missed[ti]:
                results["false_negatives"].append({"image_id": image_id, "true_idx": ti})
            for pi, c in enumerate(crow):
                if c in (1, 2):
                    pair = {"true_idx": ti, "pred_idx": pi, "image_id": image_id}
                    results["true_positives" if c == 1 else "near_true_positives"].append(pair)
        results["false_positives"] += [{"pred_index": pi, "image_id": image_id} for pi, u in enumerate(unclaimed) if u]
    n_tp, n_fp, n_fn = tables["counts"]
    return results, (n_tp / (n_tp + n_fp), n_tp / (n_tp + n_fn))
