"""Inputs shared by tests/test_evaluation_statement_cpu.py and tests/test_evaluation_gpu.py: generated pairs of quads, the
two scoring scenarios of tests/test_evaluation_cpu.py, a generated set of 32 labelled pages and four crowded images."""
import math
import string

import numpy as np

LIMIT = (1 << 24) - 1


def _rot_rect(rng, cx, cy, w, h, angle):
    c, s = math.cos(angle), math.sin(angle)
    return [(int(round(cx + dx * c - dy * s)), int(round(cy + dx * s + dy * c)))
            for dx, dy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))]


def _convex(rng, cx, cy, rx, ry):
    """four points on an ellipse at sorted angles at least 0.3 rad apart: a convex quad, random start and orientation"""
    while True:
        angles = np.sort(rng.uniform(0, 2 * math.pi, 4))
        if np.diff(np.concatenate([angles, [angles[0] + 2 * math.pi]])).min() > 0.3:
            break
    pts = [(int(round(cx + rx * math.cos(a))), int(round(cy + ry * math.sin(a)))) for a in angles]
    k = int(rng.integers(4))
    pts = pts[k:] + pts[:k]
    return pts[::-1] if rng.random() < 0.5 else pts


def _dart(rng, cx, cy, r):
    """a chevron: three corners of a triangle and a fourth strictly inside it"""
    tri = _convex(rng, cx, cy, r, r)[:3]
    w = rng.dirichlet([2, 2, 2])
    q = (int(round(sum(wi * p[0] for wi, p in zip(w, tri)))), int(round(sum(wi * p[1] for wi, p in zip(w, tri)))))
    pts = tri + [q]
    k = int(rng.integers(4))
    return pts[k:] + pts[:k]


def _jitter(rng, quad, amount):
    return [(x + int(rng.integers(-amount, amount + 1)), y + int(rng.integers(-amount, amount + 1))) for x, y in quad]


def _shift(quad, dx, dy):
    return [(x + dx, y + dy) for x, y in quad]


KINDS = ("rect", "rect", "rect", "convex", "convex", "dart", "dart", "touch", "disjoint", "same", "negative", "huge",
         "triangle", "zero", "bowtie", "mixed")


def kind_of(i):
    """the kind of the i-th pair of quad_pairs"""
    return KINDS[i % len(KINDS)]


def quad_pairs(n, seed):
    """n pairs of quads (lists of four int tuples) over the kinds the IoU rule has to get right.  Small boxes stay within a
    few thousand pixels of the origin (pages); the coordinates near +-2^24 belong to boxes of that size: evaluation.py's
    shoelace sums of corner products lose the area of a small box far from the origin to cancellation (products near 2^48
    carry an absolute error near 2^-5), which is the host formula's own limit and says nothing about an implementation of
    it."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        kind = kind_of(len(out))
        cx, cy = rng.uniform(100, 1500, 2)
        if kind == "rect":
            a = _rot_rect(rng, cx, cy, rng.uniform(20, 200), rng.uniform(10, 60), rng.uniform(-math.pi, math.pi))
            b = _jitter(rng, a, int(rng.integers(1, 12)))
        elif kind == "convex":
            a = _convex(rng, cx, cy, rng.uniform(20, 150), rng.uniform(20, 150))
            b = _convex(rng, cx + rng.uniform(-40, 40), cy + rng.uniform(-40, 40), rng.uniform(20, 150), rng.uniform(20, 150))
        elif kind == "dart":
            a = _dart(rng, cx, cy, rng.uniform(30, 150))
            b = _dart(rng, cx + rng.uniform(-30, 30), cy + rng.uniform(-30, 30), rng.uniform(30, 150)) if rng.random() < 0.5 else \
                _rot_rect(rng, cx, cy, rng.uniform(20, 200), rng.uniform(10, 100), rng.uniform(-math.pi, math.pi))
        elif kind == "touch":
            x, y, w, h = int(cx), int(cy), int(rng.integers(5, 80)), int(rng.integers(5, 40))
            a = [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]
            b = _shift(a, w, 0) if rng.random() < 0.5 else _shift(a, w, h)  # an edge or a corner in common
        elif kind == "disjoint":
            a = _rot_rect(rng, cx, cy, 50, 20, rng.uniform(-1, 1))
            b = _shift(a, 400, 300)
        elif kind == "same":
            a = _convex(rng, cx, cy, 60, 30) if rng.random() < 0.5 else _dart(rng, cx, cy, 80)
            b = list(a) if rng.random() < 0.5 else a[2:] + a[:2]
        elif kind == "negative":
            a = _shift(_rot_rect(rng, cx, cy, rng.uniform(20, 200), rng.uniform(10, 60), rng.uniform(-3, 3)), -1600, -1600)
            b = _jitter(rng, a, 6)
        elif kind == "huge":
            r = LIMIT - 8
            a = _convex(rng, 0, 0, r * rng.uniform(0.6, 1), r * rng.uniform(0.6, 1))
            b = [(max(-LIMIT, min(LIMIT, x)), max(-LIMIT, min(LIMIT, y))) for x, y in _jitter(rng, a, 1 << int(rng.integers(1, 22)))]
        elif kind == "triangle":  # a repeated corner
            a = _convex(rng, cx, cy, 60, 40)
            k = int(rng.integers(4))
            a[k] = a[k - 1]
            b = _jitter(rng, _convex(rng, cx, cy, 60, 40), 3)
        elif kind == "zero":  # a box without area: collinear corners, or two corners twice
            x, y = int(cx), int(cy)
            a = [(x, y), (x + 10, y + 5), (x + 20, y + 10), (x + 30, y + 15)] if rng.random() < 0.5 else [(x, y), (x, y), (x + 9, y), (x + 9, y)]
            b = _rot_rect(rng, cx, cy, 60, 30, 0.2)
            if rng.random() < 0.5:
                a, b = b, a
        elif kind == "bowtie":  # self-intersecting: the rule's answer is whatever its operations give
            x, y, w, h = int(cx), int(cy), int(rng.integers(10, 80)), int(rng.integers(10, 80))
            a = [(x, y), (x + w, y + h), (x + w, y), (x, y + h + int(rng.integers(0, 9)))]
            b = _rot_rect(rng, cx + w / 2, cy + h / 2, w, h, rng.uniform(-0.5, 0.5))
        else:
            a = _convex(rng, cx, cy, rng.uniform(20, 150), rng.uniform(20, 150))
            b = _rot_rect(rng, cx, cy, rng.uniform(20, 200), rng.uniform(10, 100), rng.uniform(-math.pi, math.pi))
        out.append((a, b))
    return out


def sq(x, y):
    return [(x, y), (x + 10, y), (x + 10, y + 10), (x, y + 10)]


def scenario_precision_recall():
    """the inputs of tests/test_evaluation_cpu.py::test_score_precision_recall"""
    true = {"a": [{"text": "hello", "vertices": sq(0, 0)}, {"text": "world", "vertices": sq(50, 0)},
                  {"text": "skip", "vertices": sq(0, 50), "ignore": True}]}
    pred = {"a": [{"text": "hallo", "vertices": sq(1, 0)}, {"text": "xxxxx", "vertices": sq(50, 1)},
                  {"text": "extra", "vertices": sq(80, 80)}]}
    return true, pred, {}


def scenario_bookkeeping():
    """the inputs of tests/test_evaluation_cpu.py::test_score_bookkeeping_rules"""
    true = {"b": [{"text": "Hello!", "vertices": sq(0, 0)}, {"text": "", "vertices": sq(30, 0)},
                  {"text": "ign", "vertices": sq(60, 0), "ignore": True}, {"text": "lost", "vertices": sq(0, 40)},
                  {"text": "ign2", "vertices": sq(60, 60), "ignore": True}],
            "a": []}
    pred = {"a": [{"text": "ghost", "vertices": sq(5, 5)}],
            "b": [{"text": "hello", "vertices": sq(0, 1)}, {"text": "HELLO", "vertices": sq(1, 0)},
                  {"text": "", "vertices": sq(30, 1)}, {"text": "whatever", "vertices": sq(60, 1)}]}
    return true, pred, {"translator": str.maketrans(string.ascii_uppercase, string.ascii_lowercase, string.punctuation)}


PAGES_SEED = 7
WORDS = ("alpha", "Bravo", "charlie", "delta!", "echo", "fox-trot", "golf", "Hotel", "india", "juliet", "kilo", "lima", "ab", "")


def scenario_pages(seed=PAGES_SEED, pages=32, words=22):
    """32 labelled pages of 22 truths: rotated word boxes on a loose grid; the predictions are the truths jittered, some
    dropped, some extra, some truths ignored, texts edited (a substitution, case and punctuation the translator removes,
    another word, "ab" / "ax" -- similarity exactly 0.5 --, "" / "").  float32 vertices, as a pipeline returns them."""
    rng = np.random.default_rng(seed)
    true, pred = {}, {}
    for n in range(pages):
        truths, preds = [], []
        for k in range(words):
            cx, cy = 90 + 170 * (k % 4) + rng.uniform(-10, 10), 60 + 110 * (k // 4) + rng.uniform(-10, 10)
            box = _rot_rect(rng, cx, cy, rng.uniform(60, 150), rng.uniform(20, 50), rng.uniform(-0.3, 0.3))
            text = WORDS[int(rng.integers(len(WORDS)))]
            truth = {"text": text, "vertices": box}
            if rng.random() < 0.1:
                truth["ignore"] = True
            elif rng.random() < 0.1:
                truth["ignore"] = False
            truths.append(truth)
            roll = rng.random()
            if roll < 0.1:
                continue  # missed word
            amount = 2 if roll < 0.7 else 14 if roll < 0.9 else 40
            edit = rng.random()
            guess = text if edit < 0.5 else text.upper() + "?" if edit < 0.6 else "ax" if text == "ab" else \
                ("x" + text[1:]) if edit < 0.8 and text else WORDS[int(rng.integers(len(WORDS)))]
            preds.append({"text": guess, "vertices": np.array(_jitter(rng, box, amount), np.float32) + np.float32(rng.random() < 0.5) / 2})
            if rng.random() < 0.08:  # a second prediction on the same word
                preds.append({"text": text, "vertices": np.array(_jitter(rng, box, 3), np.float32)})
        for _ in range(int(rng.integers(0, 4))):  # predictions of nothing
            preds.append({"text": "noise", "vertices": [(int(rng.integers(0, 700)), 720), (int(rng.integers(700, 760)), 760)]})
        order = rng.permutation(len(preds))
        true[f"page_{n:02d}"] = truths
        pred[f"page_{n:02d}"] = [preds[i] for i in order]
    return true, pred, {"translator": str.maketrans(string.ascii_uppercase, string.ascii_lowercase, string.punctuation)}


CROWDED_LENGTHS = (0, 1, 64, 65, 256)


def scenario_crowded(seed=17):
    """Four images, ids in sorted order, whose work outgrows one block and one grid of the scoring kernels:

    ``a``  40 truths on sq(0, 0) and 40 predictions on sq(1, 0): all 1600 pairs overlap (IoU 9 / 11).  Truth 7 is ignored, the
           other 1560 pairs are listed for the text kernel.  The texts are random words over "ab" of 3 to 12 code points, and
           of CROWDED_LENGTHS code points at five places among the truths and five among the predictions: two words of like
           length mostly agree in half their places (class 1), a long word against a short one does not (class 2).
    ``b``  300 truths on a 20 x 15 grid and 5 predictions on truths 3, 100, 256, 257 (ignored) and 299.
    ``c``  5 truths, on predictions 2, 255, 256 and 299 of 300 on the same grid, and one (ignored) on prediction 150.
    ``d``  no truths and no predictions."""
    rng = np.random.default_rng(seed)

    def text(n):
        return "".join("ab"[int(v)] for v in rng.integers(0, 2, n))

    def texts(places):
        out = [text(int(rng.integers(3, 13))) for _ in range(40)]
        for at, n in zip(places, CROWDED_LENGTHS):
            out[at] = text(n)
        return out

    grid = [sq(30 * (k % 20), 30 * (k // 20)) for k in range(300)]
    true = {"a": [{"text": t, "vertices": sq(0, 0)} for t in texts((2, 11, 19, 20, 33))],
            "b": [{"text": text(4), "vertices": q} for q in grid],
            "c": [{"text": text(4), "vertices": _shift(grid[k], 0, 1)} for k in (2, 255, 150, 256, 299)],
            "d": []}
    true["a"][7]["ignore"] = True
    true["b"][257]["ignore"] = True
    true["c"][2]["ignore"] = True
    pred = {"a": [{"text": t, "vertices": sq(1, 0)} for t in texts((5, 6, 21, 30, 38))],
            "b": [{"text": true["b"][k]["text"] if k != 100 else "zzzzzzzz", "vertices": _shift(grid[k], 1, 0)} for k in (299, 3, 257, 100, 256)],
            "c": [{"text": text(4), "vertices": q} for q in grid],
            "d": []}
    return true, pred, {}


def scenarios():
    return {"precision_recall": scenario_precision_recall(), "bookkeeping": scenario_bookkeeping(), "pages": scenario_pages(),
            "crowded": scenario_crowded()}


def tables_input(true, pred, translator=None):
    """a scoring scenario as tests/evaluation_statement.py::score_tables takes it (images in sorted id order)"""
    from tests import evaluation_statement as es

    ids = sorted(true)
    clean = (lambda t: t.translate(translator)) if translator is not None else (lambda t: t)
    quads = lambda anns: [es.as_quad(np.array(_expand(a["vertices"]), dtype="int32").tolist()) for a in anns]  # noqa: E731
    return ids, dict(
        truth_quads=[quads(true[i]) for i in ids], truth_ignore=[[bool(a.get("ignore", False)) for a in true[i]] for i in ids],
        truth_texts=[[[ord(c) for c in clean(a["text"])] for a in true[i]] for i in ids],
        pred_quads=[quads(pred[i]) for i in ids], pred_texts=[[[ord(c) for c in clean(a["text"])] for a in pred[i]] for i in ids])


def _expand(box):
    if len(box) == 2:
        (x1, y1), (x2, y2) = box
        return [[x1, y1], [x2, y1], [x2, y2], [x1, y2]]
    return box
