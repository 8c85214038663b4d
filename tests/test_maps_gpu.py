"""GPU: kocr_compute_maps (warp.hip) against the full-map statement tests/maps_statement.py bit for bit, the detector's
get_batch_generator, and model.evaluate (kocr_craft_mse / kocr_heat_mse) against the float64 mse statement."""
import itertools
import math
import os

import numpy as np
import pytest

from tests import maps_statement as ms

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maps_golden.npz")
F32 = np.float32
LETTERS = "abcdefghij "


def rect(x, y, w, h, angle=0.0):
    c, s = np.cos(angle), np.sin(angle)
    pts = np.array([[0, 0], [w, 0], [w, h], [0, h]], np.float64)
    return (pts @ np.array([[c, s], [-s, c]]) + [x, y]).astype(F32)


def random_line(rng, H, W, n_max=12, degenerate=True):
    """Characters along a (possibly vertical, rotated) direction with perspective jitter, spaces, characters off the
    canvas, and (``degenerate``) the cases of the singular path: duplicates, collinear, zero-area and single-point boxes,
    and quads larger than the map."""
    n = int(rng.integers(1, n_max + 1))
    vertical = rng.random() < 0.3
    angle = rng.uniform(-0.6, 0.6)
    cw, ch = rng.uniform(3, 24, 2)
    x, y = rng.uniform(-0.2 * W, 1.1 * W), rng.uniform(-0.2 * H, 1.1 * H)
    c, s = np.cos(angle), np.sin(angle)
    line = []
    for i in range(n):
        d = i * ((ch if vertical else cw) + rng.uniform(0, 4))
        ox, oy = (x - s * d, y + c * d) if vertical else (x + c * d, y + s * d)
        box = rect(ox, oy, cw, ch, angle) + rng.uniform(-1, 1, (4, 2)).astype(F32)
        kind = rng.random() if degenerate else 1.0
        if kind < 0.04 and line:
            box = line[-1][0].copy()  # duplicate
        elif kind < 0.07:
            box = np.array([[ox, oy], [ox + 5, oy + 2], [ox + 10, oy + 4], [ox + 2.5, oy + 1]], F32)  # collinear
        elif kind < 0.09:
            box = np.array([[ox, oy]] * 2 + [[ox + 3, oy + 1]] * 2, F32)  # zero area
        elif kind < 0.11:
            box = np.full((4, 2), [ox, oy], F32)  # a single point
        elif kind < 0.13:
            box = rect(ox - W, oy - H, 3 * W, 2.5 * H, angle)  # larger than the map
        line.append((box, LETTERS[int(rng.integers(0, len(LETTERS)))]))
    return line


def random_pages(rng, n_pages, H, W, n_lines):
    return [[random_line(rng, H, W) for _ in range(int(rng.integers(0, n_lines + 1)))] for _ in range(n_pages)]


def heatmaps():
    rng = np.random.default_rng(1)
    return {"512": ms.get_gaussian_heatmap(512, 1.5), "odd": ms.get_gaussian_heatmap(37, 2.0),
            "rand": rng.integers(0, 256, (21, 34), dtype=np.uint8)}


def assert_bits(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {np.argwhere(bad)[0]}"


def test_fixture_pages(ctx):
    g = dict(np.load(GOLDEN))
    i = 0
    while f"case{i}_hw" in g:
        H, W = (int(v) for v in g[f"case{i}_hw"])
        q, c, off = g[f"case{i}_quads"], g[f"case{i}_chars"], g[f"case{i}_offsets"]
        lines = [[(q[j], str(c[j])) for j in range(off[k], off[k + 1])] for k in range(len(off) - 1)]
        for k in range(2):
            got = ctx.compute_maps(g[f"heatmap{k}"], H, W, [lines, [], lines])
            for p in (0, 2):
                assert_bits(got[p], g[f"case{i}_maps{k}"], f"case {i} heatmap {k} page {p}")
            assert not got[1].any()
        i += 1
    assert i == 6


@pytest.mark.parametrize("H,W", [(256, 192), (130, 202), (96, 254)])
def test_random_pages(ctx, H, W):
    rng = np.random.default_rng(H * 1000 + W)
    pages = random_pages(rng, 4, H, W, 6)
    for name, hm in heatmaps().items():
        got = ctx.compute_maps(hm, H, W, pages)
        for p, lines in enumerate(pages):
            assert_bits(got[p], ms.compute_maps(hm, H, W, lines), f"{H}x{W} heatmap {name} page {p}")


@pytest.mark.parametrize("seed,n", ms.TIE_SEEDS)
def test_orientation_ties(ctx, seed, n):
    hm = ms.get_gaussian_heatmap(64, 1.5)
    lines = [ms.tie_line(seed, n)]
    assert_bits(ctx.compute_maps(hm, 160, 320, [lines])[0], ms.compute_maps(hm, 160, 320, lines), f"tie {seed}")


@pytest.mark.parametrize("seed,n", ms.LONG_TIE_SEEDS)
def test_long_tie_lines(ctx, seed, n):
    """lines longer than the 64 lanes of maps_line_kernel and than the 128 terms of one pairwise leaf, on which a sum in
    another order turns the line the other way (tests/test_maps_statement_cpu.py asserts that of every one)"""
    hm = ms.get_gaussian_heatmap(64, 1.5)
    H, W = ms.LONG_TIE_HW
    lines = [ms.long_tie_line(seed, n)]
    assert_bits(ctx.compute_maps(hm, H, W, [lines])[0], ms.compute_maps(hm, H, W, lines), f"long tie {seed}, {n} characters")


def test_long_scrambled_lines(ctx):
    """lines of 64, 65, 129 and 130 characters in a scrambled order: the rank sort, the tie by index and the link chain's
    reset across the kernel's strides; alone and as page 1 of a batch"""
    page, _ = ms.long_lines_page()
    H, W = ms.LONG_PAGE_HW
    for name in ("odd", "rand"):
        hm = heatmaps()[name]
        alone = ctx.compute_maps(hm, H, W, [page])[0]
        assert_bits(alone, ms.compute_maps(hm, H, W, page), f"long page, heatmap {name}")
        batch = ctx.compute_maps(hm, H, W, [[], page, page[:2]])
        assert_bits(batch[1], alone, f"long page inside a batch, heatmap {name}")
        assert not batch[0].any() and batch[2].any()


def test_pages_without_lines_and_errors(ctx):
    hm = ms.get_gaussian_heatmap(64, 1.5)
    out = ctx.compute_maps(hm, 10, 14, [[], []])
    assert out.shape == (2, 5, 7, 2) and out.dtype == np.float32 and not out.any()
    assert ctx.compute_maps(hm, 10, 14, []).shape == (0, 5, 7, 2)
    with pytest.raises(AssertionError):
        ctx.compute_maps(hm, 11, 14, [[]])
    with pytest.raises(AssertionError):
        ctx.compute_maps(hm, 10, 13, [[]])
    with pytest.raises(IndexError):
        ctx.compute_maps(hm, 10, 14, [[[]]])


def test_detection_compute_maps_default_context():
    from keras_ocr_amd import detection

    hm = detection.get_gaussian_heatmap(size=512, distanceRatio=1.5)
    lines = random_pages(np.random.default_rng(4), 1, 64, 80, 4)[0]
    assert_bits(detection.compute_maps(hm, 64, 80, lines), ms.compute_maps(hm, 64, 80, lines), "detection.compute_maps")
    with pytest.raises(AssertionError):
        detection.compute_maps(hm, 63, 80, lines)


def dense_page(rng, H=768, W=768, chars=1000, degenerate=True):
    """A page of about `chars` characters in horizontal and vertical lines of 1 to 40."""
    lines, n = [], 0
    while n < chars:
        line = random_line(rng, H, W, n_max=40, degenerate=degenerate)
        lines.append(line)
        n += len(line)
    return lines


def test_batch_of_32_dense_pages(ctx):
    rng = np.random.default_rng(32)
    pages = [dense_page(rng) for _ in range(32)]
    hm = ms.get_gaussian_heatmap(512, 1.5)
    batch = ctx.compute_maps(hm, 768, 768, pages)
    for p in (0, 7, 31):
        assert_bits(batch[p], ctx.compute_maps(hm, 768, 768, [pages[p]])[0], f"dense page {p}")
    assert_bits(batch[5], ms.compute_maps(hm, 768, 768, pages[5]), "dense page 5 against the statement")


def samples(rng, n, weights):
    for i in itertools.count():
        if i == n:
            return
        image = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
        lines = [random_line(rng, 48, 64, 6) for _ in range(2)]
        yield (image, lines, float(i + 1)) if weights else (image, lines)


def test_get_batch_generator(ctx, craft_weights):
    from keras_ocr_amd import detection

    det = detection.Detector(weights=craft_weights, ctx=ctx)
    hm = detection.get_gaussian_heatmap(size=512, distanceRatio=1.5)
    batches = list(det.get_batch_generator(samples(np.random.default_rng(8), 7, True), batch_size=3))
    assert [len(b) for b in batches] == [3, 3, 3]
    assert [b[0].shape[0] for b in batches] == [3, 3, 1]  # a short last batch, then the end
    want = list(samples(np.random.default_rng(8), 7, True))
    for k, (X, y, sw) in enumerate(batches):
        part = want[3 * k:3 * k + 3]
        assert X.dtype == np.float32 and X.shape == (len(part), 48, 64, 3)
        assert np.array_equal(X, detection.compute_input(np.array([s[0] for s in part])))
        assert y.dtype == np.float32 and y.shape == (len(part), 24, 32, 2)
        assert np.array_equal(sw, [s[2] for s in part])
        for j, s in enumerate(part):
            assert_bits(y[j], ms.compute_maps(hm, 48, 64, s[1]), f"generator batch {k} sample {j}")
    plain = list(det.get_batch_generator(samples(np.random.default_rng(8), 2, False), batch_size=8, heatmap_size=33,
                                         heatmap_distance_ratio=2.5))
    assert len(plain) == 1 and len(plain[0]) == 2 and plain[0][1].shape == (2, 24, 32, 2)
    assert list(det.get_batch_generator(iter([]))) == []


def _exact_sum(y_true, y_pred):
    """math.fsum of the per-pixel terms ((y0 - p0)^2 + (y1 - p1)^2) / 2, each evaluated in float64 from the float32 values:
    the correctly rounded sum of the terms as the kernel forms them (the differences are exact)"""
    d = y_true.astype(np.float64) - y_pred.astype(np.float64)
    terms = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) / 2.0
    return np.array([math.fsum(image.ravel().tolist()) for image in terms], np.float64)


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (16, 16), (17, 19), (32, 48)])
def test_heat_mse_sums(ctx, h, w):
    """pixel counts below the block's 256 threads, off its multiples and on them"""
    rng = np.random.default_rng(100 * h + w)
    N = 3
    # multiples of 1 / 16 in [0, 1]: every term is a multiple of 1 / 512 and every partial sum exact, in any order
    y = (rng.integers(0, 17, (N, h, w, 2)) / 16).astype(F32)
    p = (rng.integers(0, 17, (N, h, w, 2)) / 16).astype(F32)
    d = np.rint((y.astype(np.float64) - p) * 16).astype(np.int64)
    want = ((d * d).sum(axis=(1, 2, 3)) / 512.0).astype(np.float64)
    assert np.array_equal(want, _exact_sum(y, p)) and (want > 0).all()
    got = ctx.heat_mse(y, p)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
    # random float32 maps: each term carries at most three roundings (two squares, their sum; the halving is exact) and a
    # sum of h w non-negative terms in any order at most h w - 1 more, each relative 2^-53, to first order
    y, p = rng.random((N, h, w, 2), dtype=F32), rng.random((N, h, w, 2), dtype=F32)
    ref = _exact_sum(y, p)
    got = ctx.heat_mse(y, p)
    bound = (h * w + 4) * 2.0 ** -53 * ref
    print(f"heat_mse {h}x{w}: |got - ref| / ref = {np.abs(got - ref) / ref}, gate {(h * w + 4) * 2.0 ** -53:.3e}")
    assert (ref > 0).all() and (np.abs(got - ref) <= bound).all(), (got, ref, bound)
    # image k alone: the same bits as inside the batch
    for k in range(N):
        assert ctx.heat_mse(y[k:k + 1], p[k:k + 1]).view(np.uint64)[0] == got.view(np.uint64)[k]


def test_evaluate_mse(ctx, craft_weights):
    from keras_ocr_amd import detection

    det = detection.Detector(weights=craft_weights, ctx=ctx)
    rng = np.random.default_rng(12)
    x = detection.compute_input(rng.integers(0, 256, (5, 64, 96, 3), dtype=np.uint8))
    y = rng.random((5, 32, 48, 2)).astype(F32)
    sw = rng.uniform(0.5, 2.0, 5)
    pred = det.model.predict(x, batch_size=2)
    # the fused path keeps the heat-maps in HBM and equals the given-prediction path bit for bit
    fused = ctx.craft_mse(x, y, micro_batch=2)
    assert np.array_equal(fused.view(np.uint64), ctx.heat_mse(y, pred).view(np.uint64))
    # and at 25 x 35 = 875 pixels, no multiple of heat_mse_kernel's 256 threads
    x2 = detection.compute_input(rng.integers(0, 256, (3, 50, 70, 3), dtype=np.uint8))
    y2 = rng.random((3, 25, 35, 2)).astype(F32)
    fused2 = ctx.craft_mse(x2, y2, micro_batch=2)
    assert np.array_equal(fused2.view(np.uint64), ctx.heat_mse(y2, det.model.predict(x2, batch_size=2)).view(np.uint64))
    for bs, w in ((2, sw), (None, None)):
        got = det.model.evaluate(x, y, batch_size=bs, sample_weight=w)
        want = ms.mse_loss_f64(y, pred, w)
        ratio = abs(got - want) / want
        print(f"evaluate batch_size={bs}: {got!r} vs float64 statement {want!r}, relative difference {ratio:.2e}")
        assert ratio <= 1e-6
    with pytest.raises(NotImplementedError):
        det.model.fit(x, y)
    with pytest.raises(NotImplementedError):
        det.model.compile(loss="mse")
