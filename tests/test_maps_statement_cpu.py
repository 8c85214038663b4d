"""CPU: the detector-target statement (tests/maps_statement.py) against the reference's own code (maps_golden.npz, written
by tests/golden/make_golden_maps.py), and the host halves of keras_ocr_amd's compute_maps / fix_line / generator helpers."""
import inspect
import os

import numpy as np
import pytest

from oracle import tools as otools
from tests import maps_statement as ms

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "maps_golden.npz")
F32 = np.float32


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def golden_cases(g):
    """[(H, W, lines)] of the fixture"""
    out = []
    i = 0
    while f"case{i}_hw" in g:
        H, W = (int(v) for v in g[f"case{i}_hw"])
        q, c, off = g[f"case{i}_quads"], g[f"case{i}_chars"], g[f"case{i}_offsets"]
        lines = [[(q[j], str(c[j])) for j in range(off[k], off[k + 1])] for k in range(len(off) - 1)]
        out.append((H, W, lines))
        i += 1
    return out


def test_statement_equals_reference_compute_maps(golden):
    hms = [golden["heatmap0"], golden["heatmap1"]]
    cases = golden_cases(golden)
    assert len(cases) == 6
    for i, (H, W, lines) in enumerate(cases):
        for k, hm in enumerate(hms):
            got = ms.compute_maps(hm, H, W, lines)
            want = golden[f"case{i}_maps{k}"]
            assert got.dtype == np.float32 and want.dtype == np.float32
            assert got.shape == (H // 2, W // 2, 2)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (i, k)


def test_fixture_reaches_the_singular_path(golden):
    """A collinear character makes the perspective system singular: cv2 then samples heatmap[0, 0] on the whole map."""
    hm = golden["heatmap0"]
    line = [(np.array([[20, 20], [30, 20], [40, 20], [25, 20]], F32), "d")]
    got = ms.compute_maps(hm, 16, 20, [line])
    assert np.all(got[..., 0] == F32(hm[0, 0]) / F32(255)) and np.all(got[..., 1] == 0)
    assert hm[0, 0] == 26


def test_gaussian_heatmap(golden):
    from keras_ocr_amd import detection

    for k, (size, ratio) in enumerate(golden["heatmap_args"]):
        want = golden[f"heatmap{k}"]
        assert np.array_equal(ms.get_gaussian_heatmap(int(size), float(ratio)), want)
        assert np.array_equal(detection.get_gaussian_heatmap(size=int(size), distanceRatio=float(ratio)), want)


def test_fix_line_equals_reference(golden):
    from keras_ocr_amd import tools

    for i, (_, _, lines) in enumerate(golden_cases(golden)):
        fixed, vertical = [], []
        for line in lines:
            fl, o = tools.fix_line(line)
            sl, so = ms.fix_line(line)
            assert o == so
            assert [c for _, c in fl] == [c for _, c in sl]
            for (a, _), (b, _) in zip(fl, sl):
                assert np.array_equal(a, b) and a.dtype == np.float32
            fixed += [b for b, _ in fl]
            vertical.append(o == "vertical")
        assert np.array_equal(np.array(fixed, F32).reshape(-1, 4, 2), golden[f"case{i}_fixed"]), i
        assert np.array_equal(np.array(vertical, bool), golden[f"case{i}_vertical"]), i


def test_pairwise_sum_is_numpys():
    rng = np.random.default_rng(3)
    for _ in range(400):
        n = int(rng.integers(0, 300))
        a = (rng.standard_normal(n) * 10 ** rng.uniform(-3, 3, n)).astype(F32)
        assert ms.pairwise_sum_f32(a).tobytes() == a.sum().tobytes()


def _naive_sum(a):
    r = F32(a[0])
    for v in a[1:]:
        r = F32(r + v)
    return r


TIE_LINES = [(seed, n, False) for seed, n in ms.TIE_SEEDS] + [(seed, n, True) for seed, n in ms.LONG_TIE_SEEDS]


@pytest.mark.parametrize("seed,n,long", TIE_LINES, ids=[f"{seed}-{n}" for seed, n, _ in TIE_LINES])
def test_orientation_follows_the_pairwise_order(seed, n, long):
    from keras_ocr_amd import tools

    line = ms.long_tie_line(seed, n) if long else ms.tie_line(seed, n)
    c = np.array([ms.box_center(otools.get_rotated_box(b)[0]) for b, _ in line], F32)
    ddx = np.diff(c[np.argsort(c[:, 0], kind="stable")][:, 0])
    ddy = np.diff(c[np.argsort(c[:, 1], kind="stable")][:, 1])
    assert ms.pairwise_sum_f32(ddx).tobytes() == ddx.sum().tobytes() and ms.pairwise_sum_f32(ddy).tobytes() == ddy.sum().tobytes()
    pairwise = ms.pairwise_sum_f32(ddy) > ms.pairwise_sum_f32(ddx)
    assert pairwise != (_naive_sum(ddy) > _naive_sum(ddx)), "the line no longer separates the two orders"
    if n >= 130:  # more than 128 differences: a sum that never splits gets the orientation wrong
        assert len(ddx) > 128
        assert pairwise != (ms.one_leaf_sum_f32(ddy) > ms.one_leaf_sum_f32(ddx)), "the line no longer separates the split from one leaf"
    want = "vertical" if pairwise else "horizontal"
    assert ms.fix_line(line)[1] == want
    assert tools.fix_line(line)[1] == want


def test_long_tie_lines_cover_the_boundaries_and_fit_their_map():
    assert [n for _, n in ms.LONG_TIE_SEEDS] == [65, 129, 130, 258, 300]
    H, W = ms.LONG_TIE_HW
    assert H // 2 <= 170 and W // 2 <= 170
    for seed, n in ms.LONG_TIE_SEEDS:
        line = ms.long_tie_line(seed, n)
        c = np.array([ms.box_center(b) for b, _ in line], F32)
        assert len(line) == n and (np.diff(c[:, 0]) > 0).all() and (np.diff(c[:, 1]) > 0).all()  # it arrives sorted
        assert c[:, 0].max() < W + 16 and c[:, 1].max() < H + 16 and (c[:64] < [W, H]).all()
    a = np.random.default_rng(1).standard_normal(128).astype(F32)
    assert ms.one_leaf_sum_f32(a).tobytes() == a.sum().tobytes()
    assert len(ms.tie_line(11, 20)) == 20 and np.array_equal(ms.tie_line(11, 20)[3][0], ms.tie_line(11, 20, (3, 9), 0.3)[3][0])


def test_long_lines_page_is_what_it_says():
    """four scrambled lines of 64, 65, 129 and 130 characters: fix_line gives the constructed reading order and orientation"""
    lines, expected = ms.long_lines_page()
    H, W = ms.LONG_PAGE_HW
    assert [len(line) for line in lines] == [64, 65, 129, 130] and H // 2 <= 170 and W // 2 <= 170
    assert [o for _, o in expected] == ["horizontal", "vertical", "horizontal", "vertical"]
    at_the_stride, twins = 0, 0
    for line, (ordered, orientation) in zip(lines, expected):
        fixed, got = ms.fix_line(line)
        assert got == orientation
        assert [c for _, c in fixed] == [c for _, c in ordered]
        assert all(np.array_equal(a, otools.get_rotated_box(b)[0]) for (a, _), (b, _) in zip(fixed, ordered))
        centers = np.array([ms.box_center(otools.get_rotated_box(b)[0]) for b, _ in ordered], F32)
        assert centers.min() > 0 and (centers < [W, H]).all()
        if orientation == "vertical":  # truly vertical: at least 2 : 1
            assert np.ptp(centers[:, 1]) >= 2 * np.ptp(centers[:, 0])
        else:
            assert np.ptp(centers[:, 0]) >= 2 * np.ptp(centers[:, 1])
        # scrambled: no input stride of 64 holds a run of the reading order
        given = [next(k for k, (b, c) in enumerate(ordered) if b is box) for box, _ in line]
        assert sorted(given) == list(range(len(line))) and given != sorted(given)
        assert sum(1 for a, b in zip(given, given[1:]) if b == a + 1) < len(line) // 8
        spaces = [k for k, (_, c) in enumerate(ordered) if c == " "]
        assert spaces and 0 < spaces[0] and spaces[-1] < len(ordered) - 1
        at_the_stride += sum(1 for k in spaces if k in (63, 64))
        main = 1 if orientation == "vertical" else 0
        for k in np.flatnonzero(np.diff(centers[:, main]) == 0):  # two characters on one centre
            assert np.array_equal(centers[k], centers[k + 1])
            first, second = given.index(int(k)), given.index(int(k) + 1)
            assert first < 64 <= second, "the tie is not decided between two strides"
            assert (ordered[k][1] == " ") != (ordered[k + 1][1] == " ")  # the order decides which of them the links reach
            twins += 1
    assert at_the_stride >= 1 and twins == 2


def test_empty_line_and_odd_sizes():
    hm = ms.get_gaussian_heatmap(32, 1.5)
    with pytest.raises(IndexError):
        ms.compute_maps(hm, 16, 16, [[]])
    with pytest.raises(AssertionError):
        ms.compute_maps(hm, 15, 16, [])
    with pytest.raises(AssertionError):
        ms.compute_maps(hm, 16, 15, [])


def test_host_helpers_equal_reference(golden):
    from keras_ocr_amd import detection

    x = detection.compute_input(golden["input_img"])
    assert x.dtype == np.float32 and np.array_equal(x, golden["input_x"])
    inv = detection.invert_input(golden["input_x"])
    assert inv.dtype == np.uint8 and np.array_equal(inv, golden["input_inv"])
    rgb = detection.map_to_rgb(golden["rgb_in"])
    assert rgb.dtype == np.uint8 and np.array_equal(rgb, golden["rgb_out"])


def test_mse_statement_reduces_batches():
    """Keras' evaluate: batch losses (SUM_OVER_BATCH_SIZE over N_b h w elements) averaged with weights N_b equal
    sum_n w_n S_n / (N h w) for any batch size."""
    rng = np.random.default_rng(9)
    y, p = rng.random((7, 5, 6, 2)), rng.random((7, 5, 6, 2))
    sw = rng.random(7)
    whole = ms.mse_loss_f64(y, p, sw)
    for bs in (1, 2, 3, 7):
        losses, sizes = [], []
        for s in range(0, 7, bs):
            l = ((y[s:s + bs] - p[s:s + bs]) ** 2).mean(-1) * sw[s:s + bs, None, None]
            losses.append(l.sum() / l.size)
            sizes.append(len(l))
        assert abs(np.average(losses, weights=sizes) - whole) <= 1e-12 * whole


# The reference's signatures (detection.py, tools.py), written out: the public names keep them.
REFERENCE_SIGNATURES = {
    "compute_input": "(image)",
    "invert_input": "(X)",
    "get_gaussian_heatmap": "(size=512, distanceRatio=3.34)",
    "compute_maps": "(heatmap, image_height, image_width, lines)",
    "map_to_rgb": "(y)",
    "get_batch_generator": "(self, image_generator, batch_size=8, heatmap_size=512, heatmap_distance_ratio=1.5)",
    "fix_line": "(line)",
}


def test_signatures_follow_the_reference():
    from keras_ocr_amd import detection, tools

    got = {n: str(inspect.signature(getattr(detection, n))) for n in
           ("compute_input", "invert_input", "get_gaussian_heatmap", "compute_maps", "map_to_rgb")}
    got["get_batch_generator"] = str(inspect.signature(detection.Detector.get_batch_generator))
    got["fix_line"] = str(inspect.signature(tools.fix_line))
    assert got == REFERENCE_SIGNATURES
    assert str(inspect.signature(ms.compute_maps)) == REFERENCE_SIGNATURES["compute_maps"]
    assert str(inspect.signature(ms.fix_line)) == REFERENCE_SIGNATURES["fix_line"]


def test_compute_maps_refuses_other_heatmaps():
    from keras_ocr_amd import detection

    with pytest.raises(NotImplementedError, match="float32"):
        detection.compute_maps(np.zeros((8, 8), np.float32), 16, 16, [])
