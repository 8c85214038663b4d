"""CPU suite: the oracle's resize and warp statements (oracle/tools.py) at the edge shapes of tests/geometry_cases.py.

The oracle is a numpy restatement of OpenCV and is anchored to the real library only at the recorded golden shapes; the shapes
here are new classes (downscales, 1-pixel axes, boxes outside the image, perspective quads whose denominator vanishes), so each
gets the anchor tests/test_thirdparty_crosscheck_cpu.py uses: float64 interpolation written out independently.  The GPU kernels
are then held to the oracle bit for bit (tests/test_geometry_edges_gpu.py).  A coverage guard counts, in the reference
computation, the pixels that reach each branch a case is named for."""
import numpy as np
import pytest

from tests import geometry_cases as gc


# ---------------------------------------------------------------------------------------------------------------------
# resize
# ---------------------------------------------------------------------------------------------------------------------
def _bilinear_f64(img, dh, dw, weight_dtype=np.float64):
    """float64 bilinear interpolation, half-pixel centres: source coordinate (d + 0.5) * src / dst - 0.5, taps clamped to the
    image.  img: (H, W, C).  ``weight_dtype``: the format the fraction is stored in before the float64 arithmetic."""
    sh, sw = img.shape[:2]
    x = img.astype(np.float64)

    def axis(dst_n, src_n):
        f = (np.arange(dst_n) + 0.5) * src_n / dst_n - 0.5
        i0 = np.floor(f)
        t = (f - i0).astype(weight_dtype).astype(np.float64)
        return np.clip(i0, 0, src_n - 1).astype(int), np.clip(i0 + 1, 0, src_n - 1).astype(int), t

    x0, x1, tx = axis(dw, sw)
    y0, y1, ty = axis(dh, sh)
    tx, ty = tx[None, :, None], ty[:, None, None]
    rows = x[:, x0] * (1 - tx) + x[:, x1] * tx
    return rows[y0] * (1 - ty) + rows[y1] * ty


@pytest.mark.parametrize("case", gc.resize_cases_u8(), ids=gc.case_id)
def test_u8_resize_within_one_lsb_of_float64_bilinear(case):
    """the bar of test_thirdparty_crosscheck_cpu.py::test_resize_within_one_lsb_of_float_bilinear: 11-bit coefficients and two
    truncating shifts stay within 1 LSB of the exact bilinear value"""
    from oracle import tools as ot

    _, _, _, dh, dw, _, _, _, _ = case
    for im in gc.resize_source_u8(case):
        got = ot.cv_resize_linear_u8(im, (dw, dh))
        assert got.shape == (dh, dw, 3) and got.dtype == np.uint8
        err = np.abs(got.astype(np.float64) - _bilinear_f64(im, dh, dw)).max()
        assert err <= 1.0, err


def test_u8_resize_exact_half_is_the_rounded_mean_of_four():
    """OpenCV routes an exact 2:1 INTER_LINEAR to its area path, (a + b + c + d + 2) >> 2; the linear path agrees only because
    its 11-bit coefficients come out as 1024 / 1024 and the shifts lose nothing"""
    from oracle import tools as ot

    case = next(c for c in gc.resize_cases_u8() if c[0] == "half")
    im = gc.resize_source_u8(case)[0]
    assert (case[1], case[2]) == (2 * case[3], 2 * case[4])
    for i0, i1, c0, c1 in (ot._resize_axis_tables(case[2], case[4], True), ot._resize_axis_tables(case[1], case[3], False)):  # pylint: disable=protected-access
        assert (c0 == 1024).all() and (c1 == 1024).all() and np.array_equal(i0, 2 * np.arange(len(i0))) and np.array_equal(i1, i0 + 1)
    q = im.astype(np.int64)
    want = (q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2
    assert np.array_equal(ot.cv_resize_linear_u8(im, (case[4], case[3])), want)


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("case", gc.resize_cases_f32(), ids=gc.case_id)
def test_float_resize_within_rounding_of_float64_bilinear(case, channels):
    """Bound: 4 * 2^-24 * (bilinear interpolation of |x|).  The weight a of cv2.resize on a float image is a float32 (its
    coefficient format, like the 11 bits of the uint8 path), so the float64 side rounds its own fraction to float32 and does
    everything else in float64; an interpolation with the unrounded fraction is no reference for this bound, since a
    weight near 1 is off by up to 2^-25 ABSOLUTE and fl(1 - a) inherits that whatever the size of 1 - a (x0 = 1e4, x1 = 1,
    a = 0.999: 3e-4 against an interpolated |x| of 11).  With the weight given, one pass is fl(fl(x0 * fl(1 - a)) + fl(x1 * a)):
    fl(1 - a) is exact for a >= 0.5 and one relative rounding of 2^-24 below, each product one, the sum one -- at most three
    roundings along either term, a factor within (1 + 2^-24)^3 of the exact pass on |x|, and the same again for the second
    pass: 6 * 2^-24 if every rounding were at its worst with one sign, which no pixel comes near; the statement is held to
    4 * 2^-24."""
    from oracle import tools as ot

    _, _, _, dh, dw, _, _, _, _ = case
    for im in gc.resize_source_f32(case, channels):
        got = ot.resize_linear_float(im, (dw, dh))
        assert got.shape == (dh, dw, channels) and got.dtype == np.float32
        want, scale = _bilinear_f64(im, dh, dw, np.float32), _bilinear_f64(np.abs(im), dh, dw)
        excess = np.abs(got.astype(np.float64) - want) - 4 * 2.0 ** -24 * scale
        assert excess.max() <= 0, (excess.max(), np.abs(got - want).max())


@pytest.mark.parametrize("case", gc.resize_cases_f32(), ids=gc.case_id)
def test_float_resize_of_one_clamped_pixel_is_that_pixel(case):
    """Where both taps of an axis are the same clamped pixel (the right / bottom border, a 1-pixel axis) OpenCV sets the weight
    to 0, so the pass returns the pixel itself; v * (1 - a) + v * a with a != 0 can be an ulp off."""
    from oracle import tools as ot

    _, sh, sw, dh, dw, _, _, _, _ = case
    x0, x1, ax = ot.resize_float_taps(dw, sw)
    y0, y1, ay = ot.resize_float_taps(dh, sh)
    im = gc.resize_source_f32(case, 3)[0]
    got = ot.resize_linear_float(im, (dw, dh))
    ys, xs = np.nonzero(y0 == y1)[0], np.nonzero(x0 == x1)[0]
    if len(ys) and len(xs):  # both passes degenerate: the source pixel, bit for bit
        assert np.array_equal(got[np.ix_(ys, xs)].view(np.uint32), im[np.ix_(y0[ys], x0[xs])].view(np.uint32))
    if sh == 1:              # every row is the horizontal pass of the one source row
        assert all(np.array_equal(got[0].view(np.uint32), r.view(np.uint32)) for r in got)
    if sw == 1:
        assert all(np.array_equal(got[:, 0].view(np.uint32), got[:, k].view(np.uint32)) for k in range(dw))
    assert (ax[x0 == x1] == 0).all() and (ay[y0 == y1] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# warp
# ---------------------------------------------------------------------------------------------------------------------
INT_MIN, INT_MAX = -2147483648.0, 2147483647.0


def _coordinates(M, dw, dh):
    """The 1/32-pixel source coordinate of every crop pixel, pixel by pixel in Python floats (float64), following the oracle's
    rounding rule: (mi0 x + mi1 y) + mi2, 32 / W0 (0 where W0 == 0), clamp to int32, round half to even.  Returns X, Y and
    the branch counters of the coverage guard."""
    from oracle import tools as ot

    mi = ot.invert3(M)
    X = np.zeros((dh, dw), np.int64)
    Y = np.zeros((dh, dw), np.int64)
    zero_w = np.zeros((dh, dw), bool)
    clamped = np.zeros((dh, dw), bool)
    for y in range(dh):
        for x in range(dw):
            xd, yd = float(x), float(y)
            X0 = (mi[0][0] * xd + mi[0][1] * yd) + mi[0][2]
            Y0 = (mi[1][0] * xd + mi[1][1] * yd) + mi[1][2]
            W0 = (mi[2][0] * xd + mi[2][1] * yd) + mi[2][2]
            wi = 32.0 / W0 if W0 != 0.0 else 0.0
            fx, fy = X0 * wi, Y0 * wi
            zero_w[y, x] = W0 == 0.0
            clamped[y, x] = not (INT_MIN <= fx <= INT_MAX and INT_MIN <= fy <= INT_MAX)
            X[y, x] = round(max(INT_MIN, min(INT_MAX, fx)))  # Python's round(): half to even
            Y[y, x] = round(max(INT_MIN, min(INT_MAX, fy)))
    return X, Y, zero_w, clamped


def _sample_f64(gray, X, Y):
    """Bilinear interpolation of a 2-D image at (X / 32, Y / 32) in float64 with a constant-0 border: floor and fraction
    instead of shifts and masks, real weights instead of 15-bit integers.  Every product is exact for uint8 taps (weights are
    multiples of 1 / 1024), so round-half-up of the sum is what cv2.warpPerspective's fixed point returns."""
    H, W = gray.shape
    padded = np.zeros((H + 2, W + 2), np.float64)
    padded[1:-1, 1:-1] = gray
    x, y = X / 32.0, Y / 32.0
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0

    def tap(yy, xx):
        inside = (yy >= -1) & (yy <= H) & (xx >= -1) & (xx <= W)
        return np.where(inside, padded[np.clip(yy + 1, 0, H + 1).astype(int), np.clip(xx + 1, 0, W + 1).astype(int)], 0.0)

    parts = ((1 - fx) * (1 - fy) * tap(y0, x0), fx * (1 - fy) * tap(y0, x0 + 1), (1 - fx) * fy * tap(y0 + 1, x0),
             fx * fy * tap(y0 + 1, x0 + 1))
    return parts[0] + parts[1] + parts[2] + parts[3], sum(np.abs(p) for p in parts)


def _count(coverage, key, n):
    coverage[key] = coverage.get(key, 0) + int(n)


def _check_warp(grays, M, dsize, coverage, problems, name):
    """warp_perspective_u8 / warp_perspective_float of every page against the direct evaluation; mismatches go to ``problems``
    and the branch counters of the reference computation to ``coverage``.  Returns the uint8 crops."""
    from oracle import tools as ot

    dw, dh = dsize
    X, Y, zero_w, clamped = _coordinates(M, dw, dh)
    H, W = grays[0].shape
    sx, sy = X >> 5, Y >> 5
    _count(coverage, "W0 == 0", zero_w.sum())
    _count(coverage, "clamped high", (clamped & ((X == int(INT_MAX)) | (Y == int(INT_MAX)))).sum())
    _count(coverage, "clamped low", (clamped & ((X == int(INT_MIN)) | (Y == int(INT_MIN)))).sum())
    _count(coverage, "negative X with a fraction", ((X < 0) & (X & 31 != 0) & (X > -32 * 8)).sum())
    _count(coverage, "negative Y with a fraction", ((Y < 0) & (Y & 31 != 0) & (Y > -32 * 8)).sum())
    _count(coverage, "X in (-32, 0), row inside", ((X < 0) & (X > -32) & (sy >= 0) & (sy < H)).sum())
    _count(coverage, "last column, neighbour outside", ((sx == W - 1) & (sy >= 0) & (sy < H)).sum())
    _count(coverage, "last row, neighbour outside", ((sy == H - 1) & (sx >= 0) & (sx < W)).sum())
    _count(coverage, "all four taps outside", ((sx < -1) | (sx >= W) | (sy < -1) | (sy >= H)).sum())
    crops = []
    for k, gray in enumerate(grays):
        got = ot.warp_perspective_u8(gray, M, (dw, dh))
        value, _ = _sample_f64(gray, X, Y)
        if not np.array_equal(got, np.floor(value + 0.5).astype(np.uint8)):
            problems.append((name, k, "uint8 warp != round-half-up of the float64 interpolation"))
        if not (got[zero_w] == gray[0, 0]).all():      # Wi = 0: source pixel (0, 0) with both fractions 0
            problems.append((name, k, "a W0 == 0 pixel is not source pixel (0, 0)"))
        if got[clamped].any():                         # +-2^31 / 32 pixels away: outside
            problems.append((name, k, "a clamped pixel is not 0"))
        # the float statement samples at the same coordinates: its float32 weights are exact (multiples of 1 / 1024), each of
        # the four products rounds once and each of the three sums once: 4 * 2^-24 of the interpolation of |x|
        gf = gray.astype(np.float32) + np.float32(0.37)
        value, scale = _sample_f64(gf, X, Y)
        gotf = ot.warp_perspective_float(gf, M, (dw, dh))
        if not (np.abs(gotf.astype(np.float64) - value) <= 4 * 2.0 ** -24 * scale).all():
            problems.append((name, k, "float warp off the float64 interpolation by more than 4 * 2^-24"))
        crops.append(got)
    return crops


@pytest.fixture(scope="module")
def report():
    """Every box case at every target and every quad case, once: (problems, coverage).  coverage: branch -> number of pixels
    (or cases) of the REFERENCE computation that reached it."""
    from oracle import tools as ot

    grays = [ot.rgb2gray_u8(im) for im in gc.warp_images_u8()]
    problems, coverage = [], {}
    for th, tw in gc.TARGETS:
        for name, box, expect, _ in gc.box_cases():
            tag = (name, th, tw)
            if expect != "ok":
                try:
                    ot.warp_box_params(box, th, tw)
                    problems.append((tag, "no error"))
                except ZeroDivisionError as e:  # the oracle raises it for both: "division by zero" / "singular ..."
                    if ("singular" in str(e)) != (expect == "singular"):
                        problems.append((tag, f"expected {expect}, got {e}"))
                _count(coverage, "status 1" if expect == "zero" else "status 2 (box)", 1)
                continue
            try:
                ot.min_rotated_rect_f64(box)
            except AttributeError:
                _count(coverage, "rotated_box fallback, status 0", 1)
            _, (w, h), _, M, dsize, _ = ot.warp_box_params(box, th, tw)
            if (th, tw) == (31, 200) and gc.EXPECTED_DSIZE.get(name, dsize) != dsize:
                problems.append((tag, f"crop size {dsize}"))
            if name == "tall_40x3" and not th / h < tw / w:
                problems.append((tag, "scale not decided by the height"))
            crops = _check_warp(grays, M, dsize, coverage, problems, tag)
            if name == "outside" and any(c.any() for c in crops):
                problems.append((tag, "not all zero"))
            if name == "collinear_zero_inverse" and not all(c.size and (c == g[0, 0]).all() for c, g in zip(crops, grays)):
                problems.append((tag, "not source pixel (0, 0) everywhere"))
    th, tw = gc.QUAD_TARGET
    for name, src, dst, (cw, ch), _, expect, _ in gc.quad_cases():
        d = src[[1, 2, 3, 0]] - src
        if not (cw <= tw and ch <= th and np.abs(d[0] + d[2]).max() > 1e-3):  # opposite edges equal and opposite: a parallelogram
            problems.append((name, "not a perspective quad inside the target"))
        if expect == "singular":
            try:
                ot.get_perspective_transform(src, dst)
                problems.append((name, "no error"))
            except ZeroDivisionError as e:
                if "singular" not in str(e):
                    problems.append((name, str(e)))
            _count(coverage, "status 2 (quad)", 1)
            continue
        M = ot.get_perspective_transform(src, dst)
        before = coverage.get("W0 == 0", 0)
        _check_warp(grays, M, (cw, ch), coverage, problems, name)
        if name == "denominator_changes_sign":
            _count(coverage, "W0 == 0 on one crop column of a regular matrix", coverage.get("W0 == 0", 0) - before)
            mi = np.array(ot.invert3(M))
            if not np.array_equal(mi, [[2, 0, -8], [0, 2, -16], [1, 0, -3]]):
                problems.append((name, f"inverse {mi.tolist()}"))
            w0 = mi[2, 0] * np.arange(cw) + mi[2, 2]
            _count(coverage, "W0 < 0 and W0 > 0 in one crop", min((w0 < 0).sum(), (w0 > 0).sum()))
    return problems, coverage


def test_warps_equal_direct_float64_evaluation(report):
    """warp_perspective_u8 with the matrix the oracle computed == a direct float64 evaluation at the oracle's 1/32-pixel
    coordinates, exactly (with the coordinate fixed the rest is integer); a W0 == 0 pixel is source pixel (0, 0), a clamped
    pixel is 0; degenerate boxes raise what their case says."""
    problems, _ = report
    assert not problems, problems


BRANCHES = ["W0 == 0", "W0 == 0 on one crop column of a regular matrix", "clamped high", "clamped low", "negative X with a fraction", "negative Y with a fraction",
            "X in (-32, 0), row inside", "last column, neighbour outside", "last row, neighbour outside", "all four taps outside",
            "status 1", "status 2 (box)", "status 2 (quad)", "rotated_box fallback, status 0", "W0 < 0 and W0 > 0 in one crop"]


def test_every_named_branch_is_reached(report):
    """a later edit of a case must not quietly stop covering the branch it is named for"""
    _, coverage = report
    print("geometry edge coverage:", {k: coverage.get(k, 0) for k in BRANCHES})
    missing = [k for k in BRANCHES if coverage.get(k, 0) <= 0]
    assert not missing, missing
