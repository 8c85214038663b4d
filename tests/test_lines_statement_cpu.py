"""CPU suite: the float64 statement of line grouping (tests/lines_statement.py) on pages with known answers, at its
thresholds and on the random pages the GPU suite compares bit for bit; and the surface the feature adds."""
import inspect
import math

import numpy as np
import pytest

from tests import lines_cases as lc
from tests import lines_statement as ls


def _check_page(name, quads, lines, rule):
    got = ls.group_page(quads, **rule)
    assert got["lines"] == lines, (name, got["lines"])
    n = len(quads)
    assert sorted(got["order"].tolist()) == list(range(n)), name
    assert got["order"].tolist() == [j for line in lines for j in line], name
    assert got["line_of"].tolist() == [next(k for k, line in enumerate(lines) if j in line) for j in range(n)], name
    assert got["boxes"].shape == (len(lines), 4, 2) and got["boxes"].dtype == np.float32, name
    return got


@pytest.mark.parametrize("case", lc.hand_made(), ids=lambda c: c[0])
def test_hand_made_pages(case):
    _check_page(*case)


def test_hand_made_boxes():
    """the line box is the bounding rectangle along the line's axis"""
    cases = {c[0]: c for c in lc.hand_made()}
    got = _check_page(*cases["three lines scrambled"])
    assert np.array_equal(got["boxes"], lc.page([lc.box(5, 0, 147, 10), lc.box(60, 40, 35, 10), lc.box(0, 80, 217, 10)]))
    got = _check_page(*cases["degenerate"])
    assert got["boxes"][1:].tolist() == [[[70, 20], [70, 20], [70, 30], [70, 30]], [[75, 40], [90, 40], [90, 40], [75, 40]], [[3, 50]] * 4]
    # rotated by 30 degrees: the box of the unrotated line, rotated (not an axis-parallel rectangle around it)
    got = _check_page(*cases["rotated 30"])
    np.testing.assert_allclose(got["boxes"][0], lc.rotated([lc.box(0, 0, 177, 10)], 30.0)[0], rtol=0, atol=1e-3)
    # by 180 degrees: tl is the corner the line starts at, bottom right on the page
    got = _check_page(*cases["rotated 180"])
    np.testing.assert_allclose(got["boxes"][0], lc.rotated([lc.box(0, 0, 177, 10)], 180.0, (100.0, 50.0))[0], rtol=0, atol=1e-3)


@pytest.mark.parametrize("case", lc.exact_thresholds(), ids=lambda c: c[0])
def test_exact_thresholds(case):
    """a condition that holds with equality links; one float32 ulp beyond it does not.  The margin is exactly 0 where the
    case sits on its threshold."""
    name, quads, lines, rule = case
    got = _check_page(name, quads, lines, rule)
    assert (got["margin"] == 0.0) == (len(lines) == 1), (name, got["margin"])
    assert 0 < got["margin"] < 1e-6 or len(lines) == 1, (name, got["margin"])


def test_angle_with_a_margin():
    """cos is not exact, so no equality case: 14 degrees links under the default 15, 16 does not"""
    a = lc.page([lc.box(0, 0, 30, 10)])
    for degrees, lines in ((14.0, [[0, 1]]), (16.0, [[0], [1]]), (-14.0, [[0, 1]]), (-16.0, [[1], [0]])):
        b = lc.rotated([lc.box(38, 0, 30, 10)], degrees, (38.0, 5.0))
        assert ls.group_page(np.concatenate([a, b]))["lines"] == lines, degrees
    assert ls.group_page(np.concatenate([a, lc.rotated([lc.box(38, 0, 30, 10)], 16.0, (38.0, 5.0))]), max_angle=17)["lines"] == [[0, 1]]
    for bad in (90, -1, 120.5):
        with pytest.raises(ValueError, match="max_angle"):
            ls.cos_max_of(bad)


def test_linking_is_transitive_and_symmetric():
    """a slowly bending chain is one line although its ends differ by more than max_angle; the link matrix is symmetric"""
    quads, x, y = [], 0.0, 0.0
    for k in range(8):
        quads.append(lc.rotated([lc.box(x, y - 5, 30, 10)], 6.0 * k, (x, y))[0])
        x += 38 * math.cos(math.radians(6.0 * k))
        y += 38 * math.sin(math.radians(6.0 * k))
    got = ls.group_page(lc.page(quads))
    assert got["lines"] == [list(range(8))]
    rec = ls.word_records(lc.random_page(np.random.default_rng(0), 300))
    link, _ = ls.link_matrix(rec, ls.cos_max_of(15.0), 0.5, 0.5, 1.5)
    assert link.any() and (link == link.T).all() and not link.diagonal().any()


def test_chains():
    for broken in (False, True):
        quads, lines = lc.chain(512, broken)
        assert ls.group_page(quads)["lines"] == lines


@pytest.fixture(scope="module")
def batch():
    return lc.random_batch()


def test_random_pages_keep_their_distance_from_the_thresholds(batch):
    """the seeds of the pages the GPU is compared on: no tested condition within 1e-9 (relative) of its threshold, so the
    comparison never rests on a coin toss; and the pages are what they are meant to be"""
    assert sorted(len(p) for p in batch)[:4] == [0, 1, 2, 3] and set(lc.BATCH_SIZES) <= {len(p) for p in batch} and len(batch) == 64
    results = [ls.group_page(p) for p in batch]
    margin = min(r["margin"] for r in results)
    print("smallest margin of the batch:", margin)
    assert margin > 1e-9
    big = results[[len(p) for p in batch].index(2048)]
    sizes = [len(line) for line in big["lines"]]
    assert max(sizes) >= 20 and sizes.count(1) >= 10 and 50 < len(sizes) < 1500  # long lines, single words, many lines
    for rule in ({},) + lc.OTHER_RULES:
        results = [ls.group_page(p, **rule) for p in lc.small_pages()]
        assert min(r["margin"] for r in results) > 1e-9, rule
        assert len({len(r["lines"]) for r in results}) > 1
    default = [ls.group_page(p)["lines"] for p in lc.small_pages()]
    assert all([ls.group_page(p, **rule)["lines"] for p in lc.small_pages()] != default for rule in lc.OTHER_RULES), "a rule without effect"


def test_a_page_does_not_depend_on_word_order():
    """the lines and their boxes are a property of the set of words: permuting the input permutes the indices, nothing else
    -- except the axis sum, which is taken in index order and may move a box by an ulp"""
    rng = np.random.default_rng(5)
    quads = lc.random_page(rng, 90)
    perm = rng.permutation(90)
    a, b = ls.group_page(quads), ls.group_page(quads[perm])
    assert [[int(perm[j]) for j in line] for line in b["lines"]] == a["lines"]
    np.testing.assert_allclose(a["boxes"], b["boxes"], rtol=1e-6, atol=1e-3)


def test_refusals():
    with pytest.raises(ValueError, match="2049"):
        ls.group_page(np.zeros((2049, 4, 2), np.float32))
    bad = lc.page([lc.box(0, 0, 30, 10)])
    bad[0, 2, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        ls.group_page(bad)


def test_surface():
    """the names and defaults the feature adds; recognize() keeps the reference's signature"""
    import keras_ocr_amd as k

    sig = inspect.signature(k.Context.group_lines)
    assert list(sig.parameters)[1:] == ["quads", "offsets", "max_angle", "min_height_ratio", "max_offset", "max_gap", "return_boxes"]
    assert {n: p.default for n, p in sig.parameters.items() if n in ls.DEFAULTS} == ls.DEFAULTS
    assert sig.parameters["return_boxes"].default is True
    assert list(inspect.signature(k.layout.group_lines).parameters) == ["box_groups", "ctx", "rule"]
    assert k.layout.Line._fields == ("box", "words")
    sig = inspect.signature(k.pipeline.Pipeline.recognize_lines)
    assert list(sig.parameters)[1:] == ["images", "detection_kwargs", "recognition_kwargs", "rule"]
    assert list(inspect.signature(k.pipeline.Pipeline.recognize).parameters)[1:] == ["images", "detection_kwargs", "recognition_kwargs"]
    with pytest.raises(ValueError, match="beam_width"):
        k.pipeline.Pipeline(detector=object(), recognizer=object()).recognize_lines([], recognition_kwargs={"beam_width": 4})
    with pytest.raises(TypeError, match="max_gab"):
        k.layout.group_lines([], ctx=object(), max_gab=2)
