"""Cases for the character boxes (tests/chars_statement.py): words constructed from Gaussian blobs, hand-made profiles whose
samples fall on pixel centres, and the batches the GPU suite compares bit for bit."""
import math

import numpy as np

F32 = np.float32
# every value a float32, so that a map value can EQUAL a threshold
EXACT_RULE = {"peak_threshold": 0.5, "valley_ratio": 0.5, "extent_threshold": 0.25}


def rectangle(cx, cy, length, height, angle):
    """[tl, tr, br, bl] in heat-map coordinates (float64) of a rectangle around (cx, cy), its long axis at ``angle``"""
    dx, dy = math.cos(angle), math.sin(angle)
    nx, ny = -dy, dx
    a, b = length / 2.0, height / 2.0
    return np.array([[cx - dx * a - nx * b, cy - dy * a - ny * b], [cx + dx * a - nx * b, cy + dy * a - ny * b],
                     [cx + dx * a + nx * b, cy + dy * a + ny * b], [cx - dx * a + nx * b, cy - dy * a + ny * b]], np.float64)


def render(text_map, cx, cy, n, pitch, height, angle):
    """n characters of ``pitch`` x ``height`` along ``angle`` around (cx, cy) into the map (maximum with what is there): each
    a Gaussian whose sigma is the half-size / 1.5.  Returns the word's quad in detector-input pixels, float32: its
    rectangle grown by 2 heat-map pixels on every side."""
    h, w = text_map.shape
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    dx, dy = math.cos(angle), math.sin(angle)
    along = (xs - cx) * dx + (ys - cy) * dy
    across = -(xs - cx) * dy + (ys - cy) * dx
    sx, sy = pitch / 2.0 / 1.5, height / 2.0 / 1.5
    for k in range(n):
        t = (k + 0.5) * pitch - n * pitch / 2.0
        blob = np.exp(-0.5 * (((along - t) / sx) ** 2 + (across / sy) ** 2))
        np.maximum(text_map, blob.astype(F32), out=text_map)
    return (rectangle(cx, cy, n * pitch + 4.0, height + 4.0, angle) * 2.0).astype(F32)


def constructed_word(rng, shape=(64, 128)):
    """one word alone on a map: pitch 5 - 12, 1 - 8 characters, height 1 - 1.8 pitches, angle within 0.3 rad.  Returns
    ``(map, quad, n, pitch)``"""
    pitch = float(rng.uniform(5, 12))
    n = int(rng.integers(1, 9))
    height = pitch * float(rng.uniform(1.0, 1.8))
    angle = float(rng.uniform(-0.3, 0.3))
    text_map = np.zeros(shape, F32)
    cx, cy = shape[1] / 2.0 + float(rng.uniform(-3, 3)), shape[0] / 2.0 + float(rng.uniform(-3, 3))
    quad = render(text_map, cx, cy, n, pitch, height, angle)
    return text_map, quad, n, pitch


def constructed_words(count=200, seed=2024):
    rng = np.random.default_rng(seed)
    return [constructed_word(rng) for _ in range(count)]


def exact_word(values, x0=3, y=2, height=1, shape=None):
    """A map whose row ``y`` holds ``values`` from column ``x0`` on, and the axis-aligned quad over them, ``height`` rows
    tall, whose samples fall on pixel centres: with len(values) a power of two and height 1 the profile IS ``values``."""
    values = np.asarray(values, F32)
    n = len(values)
    shape = shape or (y + height + 3, max(x0, 0) + n + 4)
    text_map = np.zeros(shape, F32)
    for k, v in enumerate(values):
        if 0 <= x0 + k < shape[1]:
            text_map[y, x0 + k] = v
    left, right, top, bottom = x0 - 0.5, x0 - 0.5 + n, y - 0.5, y - 0.5 + height
    quad = np.array([[left, top], [right, top], [right, bottom], [left, bottom]], np.float64) * 2.0
    return text_map, quad.astype(F32)


def hand_made():
    """``(name, map, quad, rule, bounds, peaks)``: the answer known by hand; EXACT_RULE throughout"""
    up = lambda v: np.nextafter(F32(v), F32(2))  # noqa: E731
    down = lambda v: np.nextafter(F32(v), F32(-2))  # noqa: E731
    z = 0.0
    rows = [
        ("a peak equal to peak_threshold", [z, 0.3, 0.5, 0.3, z, z, z, z], [1, 4], [2]),
        ("a peak one ulp below peak_threshold", [z, 0.3, down(0.5), 0.3, z, z, z, z], [], []),
        ("ends equal to extent_threshold", [z, 0.25, 0.6, 0.25, z, z, z, z], [1, 4], [2]),
        ("ends one ulp below extent_threshold", [z, down(0.25), 0.6, down(0.25), z, z, z, z], [2, 3], [2]),
        ("a valley equal to valley_ratio x the lower peak", [z, 0.75, 0.25, 0.5, z, z, z, z], [1, 2, 4], [1, 3]),
        ("a valley one ulp above it", [z, 0.75, up(0.25), 0.5, z, z, z, z], [1, 4], [1]),
        ("a plateau: its first column is the peak", [z, 0.6, 0.6, 0.6, z, z, z, z], [1, 4], [1]),
        ("a higher peak replaces the current one without a cut", [z, 0.6, 0.5, 0.8, z, z, z, z], [1, 4], [3]),
        ("a lower peak after a shallow valley is dropped", [z, 0.8, 0.5, 0.6, z, z, z, z], [1, 4], [1]),
        ("tied minima: the first is the cut", [z, 0.8, 0.2, 0.3, 0.2, 0.8, z, z], [1, 2, 6], [1, 5]),
        ("three characters", [0.9, 0.1, 0.9, 0.1, 0.9, z, z, z], [0, 1, 3, 5], [0, 2, 4]),
        ("peaks at both ends of the quad", [0.7, z, z, z, z, z, z, 0.7], [0, 1, 8], [0, 7]),
        ("a single column", [0.7], [0, 1], [0]),
        ("nothing reaches extent_threshold", [z, 0.1, 0.2, 0.1, z, z, z, z], [], []),
    ]
    cases = [(name,) + exact_word(values) + (EXACT_RULE, bounds, peaks) for name, values, bounds, peaks in rows]
    # partly outside the map: the quad starts two columns left of it, the columns there are 0
    cases.append(("partly outside the map",) + exact_word([9, 9, 0.3, 0.7, 0.3, z, z, z], x0=-2) + (EXACT_RULE, [2, 5], [3]))
    text_map, quad = exact_word([0.7] * 8, x0=-20, shape=(6, 12))
    text_map[:] = 0.9
    cases.append(("wholly outside the map", text_map, quad, EXACT_RULE, [], []))
    text_map, quad = exact_word([z, 0.3, 0.7, 0.3, z, z, z, z])
    flat = quad.copy()
    flat[1], flat[2] = flat[0], flat[3]
    cases.append(("a quad of zero width", text_map, flat, EXACT_RULE, [], []))
    flat = quad.copy()
    flat[3], flat[2] = flat[0], flat[1]
    cases.append(("a quad of zero height", text_map, flat, EXACT_RULE, [], []))
    return cases


def wide_word():
    """a 16 x 1200 map with one word of 21 characters of pitch 52: wider than 512 heat-map pixels.  ``(map, quad, 21)``"""
    text_map = np.zeros((16, 1200), F32)
    quad = render(text_map, 600.0, 8.0, 21, 52.0, 9.0, 0.0)
    return text_map, quad, 21


def tall_word():
    """a 64 x 64 map with one word of 2 characters 40 heat-map pixels tall.  ``(map, quad, 2)``"""
    text_map = np.zeros((64, 64), F32)
    quad = render(text_map, 32.0, 32.0, 2, 12.0, 40.0, 0.0)
    return text_map, quad, 2


BATCH_WORDS = (5, 0, 12, 1, 8, 3)


def batch(seed=7, shape=(48, 160)):
    """The ragged batch of the GPU suite: six pages, BATCH_WORDS words each.  Returns ``(heat (6, h, w, 2), pages, inside)``:
    ``pages`` the quads per page, ``inside`` how many words lie with all their characters inside the map -- each of those
    has at least one character under the default rule (the column of its profile's maximum samples a blob within half a
    pixel of its centre, far above peak_threshold, and is a peak candidate).  Every third word is pushed across an edge of
    the map; the link channel holds noise that no result may depend on."""
    rng = np.random.default_rng(seed)
    h, w = shape
    heat = np.zeros((len(BATCH_WORDS), h, w, 2), F32)
    heat[..., 1] = rng.random((len(BATCH_WORDS), h, w), dtype=F32)
    pages, inside = [], 0
    for i, words in enumerate(BATCH_WORDS):
        text_map = np.zeros(shape, F32)
        quads = []
        for k in range(words):
            pitch = float(rng.uniform(5, 9))
            n = int(rng.integers(1, 6))
            height = pitch * float(rng.uniform(1.0, 1.5))
            angle = float(rng.uniform(-0.3, 0.3))
            if k % 3 == 2:
                cx, cy = float(rng.choice([-2.0, w + 1.0, rng.uniform(0, w)])), float(rng.choice([0.0, h - 1.0]))
            else:
                # the word's half extent along x and y, its 2 pixels of margin included: at most 32 and 16
                reach_x = n * pitch / 2.0 * math.cos(angle) + height / 2.0 * abs(math.sin(angle)) + 2.0
                reach_y = n * pitch / 2.0 * abs(math.sin(angle)) + height / 2.0 * math.cos(angle) + 2.0
                cx, cy = float(rng.uniform(reach_x, w - 1 - reach_x)), float(rng.uniform(reach_y, h - 1 - reach_y))
                inside += 1
            quads.append(render(text_map, cx, cy, n, pitch, height, angle))
        heat[i, :, :, 0] = text_map
        pages.append(np.array(quads, F32).reshape(-1, 4, 2))
    return heat, pages, int(inside)


def exact_batch():
    """the hand-made cases as one batch: ``(heat, pages)`` -- one page and one word per case, on maps padded to one size"""
    cases = hand_made()
    h = max(c[1].shape[0] for c in cases)
    w = max(c[1].shape[1] for c in cases)
    heat = np.zeros((len(cases), h, w, 2), F32)
    for i, case in enumerate(cases):
        heat[i, :case[1].shape[0], :case[1].shape[1], 0] = case[1]
    return heat, [case[2].reshape(1, 4, 2) for case in cases]


MANY_WORDS = (0, 255, 256, 257, 1, 0, 300)  # 1069 words: five blocks of chars_pack_kernel (256 words each)
DEAD_WORDS = (512, 768)  # the flat word range without characters: the whole of block 2
FULLEST_VALUES = [0.9, 0.1] * 256  # under EXACT_RULE: 512 columns, 256 peaks, bounds [0, 1, 3, ..., 509, 511]


def _dead(rng, quad, w, h):
    """a quad without characters: of zero width, of zero height, or wholly off the map"""
    kind = int(rng.integers(3))
    dead = quad.copy()
    if kind == 0:
        dead[1], dead[2] = dead[0], dead[3]
    elif kind == 1:
        dead[3], dead[2] = dead[0], dead[1]
    else:
        dead += np.array([4 * w, -4 * h] if rng.random() < 0.5 else [-4 * w, 4 * h], F32)
    return dead


def many_words_batch(seed=11, shape=(48, 160)):
    """Seven pages of MANY_WORDS words, to be run under EXACT_RULE.  Returns ``(heat, pages, fullest)``: the maps padded to
    one size as in ``exact_batch()``, the quads per page, and the flat index of the fullest word, the first of the last
    page: ``exact_word(FULLEST_VALUES)``, 256 characters, on a map of its own width.

    A 48 x 160 map has no room for 300 separate words, so every page ``render``s ten words of five blobs on a 5 x 2 grid
    below row 8, and each of its words is the quad over a run of 1 to 5 neighbouring blobs of one of them (grown by 2 pixels,
    as ``render``'s).  Flat words DEAD_WORDS[0] .. DEAD_WORDS[1] - 1 have no characters (a mix of ``_dead``'s kinds);
    elsewhere about one word in six is dead."""
    rng = np.random.default_rng(seed)
    h, w = shape
    full_map, full_quad = exact_word(FULLEST_VALUES, shape=(h, 3 + len(FULLEST_VALUES) + 4))
    width = max(w, full_map.shape[1])
    heat = np.zeros((len(MANY_WORDS), h, width, 2), F32)
    heat[..., 1] = rng.random((len(MANY_WORDS), h, width), dtype=F32)
    pages, flat = [], 0
    for i, words in enumerate(MANY_WORDS):
        text_map = np.zeros((h, width), F32)
        sites = []
        for k in range(10):
            pitch, angle = float(rng.uniform(5, 6)), float(rng.uniform(-0.15, 0.15))
            height = pitch * float(rng.uniform(1.0, 1.5))
            cx, cy = 16.0 + 32.0 * (k % 5) + float(rng.uniform(-1, 1)), 18.0 + 20.0 * (k // 5) + float(rng.uniform(-1, 1))
            render(text_map[:, :w], cx, cy, 5, pitch, height, angle)
            sites.append((cx, cy, pitch, height, angle))
        quads = []
        for k in range(words):
            cx, cy, pitch, height, angle = sites[int(rng.integers(len(sites)))]
            n = int(rng.integers(1, 6))
            first = int(rng.integers(0, 6 - n))  # blobs first .. first + n - 1 of the site's five
            along = (first + n / 2.0) * pitch - 5 * pitch / 2.0
            quad = (rectangle(cx + math.cos(angle) * along, cy + math.sin(angle) * along, n * pitch + 4.0, height + 4.0, angle) * 2.0).astype(F32)
            if i == len(MANY_WORDS) - 1 and k == 0:
                quad = full_quad
            elif DEAD_WORDS[0] <= flat < DEAD_WORDS[1] or rng.random() < 1 / 6:
                quad = _dead(rng, quad, w, h)
            quads.append(quad)
            flat += 1
        if i == len(MANY_WORDS) - 1:
            text_map[:4] = full_map[:4]
        heat[i, :, :, 0] = text_map
        pages.append(np.array(quads, F32).reshape(-1, 4, 2))
    return heat, pages, sum(MANY_WORDS[:-1])
