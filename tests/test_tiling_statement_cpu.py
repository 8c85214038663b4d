"""Tiled pages without a GPU: the tile plan by brute force, ``tools.tile_plan`` against the statement, the two copies'
statement, and what the fixtures of tests/test_tiling_gpu.py contain (so that the GPU tests cannot pass on an empty page)."""
import numpy as np
import pytest

from tests import tiling_statement as ts

PLANS = [(64, 16), (64, 0), (96, 32), (128, 48)]


@pytest.mark.parametrize("tile,overlap", PLANS)
def test_plan_by_brute_force(tile, overlap):
    for d in range(1, 4 * tile + 1):
        n, origins, cores = ts.axis_plan(d, tile, overlap)
        canvas = (n - 1) * (tile - 2 * overlap) + tile
        assert (n == 1) == (d <= tile)
        assert canvas >= d and origins[0] == 0
        # the cores partition [0, canvas): every pixel lies in exactly one
        owner = np.zeros(canvas, np.int64)
        for a, b in cores:
            owner[a:b] += 1
        assert (owner == 1).all() and cores[0][0] == 0 and cores[-1][1] == canvas
        for k, (o, (a, b)) in enumerate(zip(origins, cores)):
            assert o <= a < b <= o + tile                                     # inside its tile
            assert a == o if k == 0 else a - o >= overlap                      # an interior edge keeps the halo ...
            assert b == o + tile if k == n - 1 else o + tile - b >= overlap    # ... on both sides
            assert o % 16 == 0 and a % 16 == 0 and b % 16 == 0
        # no tile is superfluous: without the last one the page would not be covered
        assert n == 1 or origins[-2] + tile < d


@pytest.mark.parametrize("tile,overlap", PLANS)
def test_tools_tile_plan_equals_the_statement(tile, overlap):
    from keras_ocr_amd import tools

    for h, w in [(1, 1), (tile, tile), (tile + 1, tile), (tile, 4 * tile), (3 * tile - 7, 2 * tile + 33), (91, 136), (30, 40)]:
        got, want = tools.tile_plan(h, w, tile, overlap), ts.plan(h, w, tile, overlap)
        assert got.counts == want.counts and got.canvas == want.canvas and got.stride == want.stride
        assert got.origins == want.origins and got.cores == want.cores


@pytest.mark.parametrize("tile,overlap", [(72, 16), (32, 0), (64, 8), (64, -16), (64, 32), (96, 48), (128, 56)],
                         ids=["T=72", "T=32", "O=8", "O<0", "S=0", "S=0_T96", "S=16"])
def test_tools_tile_plan_refuses(tile, overlap):
    from keras_ocr_amd import tools

    with pytest.raises(ValueError):
        tools.tile_plan(100, 100, tile, overlap)


@pytest.mark.parametrize("tile,overlap,h,w", [(64, 16, 120, 180), (64, 0, 64, 65), (96, 32, 97, 33), (64, 16, 30, 40), (128, 48, 300, 129)])
def test_stitch_of_gather_is_the_identity(tile, overlap, h, w):
    p = ts.plan(h, w, tile, overlap)
    canvas = np.random.default_rng(h * w).integers(-2 ** 31, 2 ** 31, p.canvas + (2,), dtype=np.int64).astype(np.int32)
    tiles = ts.gather(canvas, p)
    assert tiles.shape == (p.counts[0] * p.counts[1], tile, tile, 2)
    assert np.array_equal(ts.stitch(tiles, p), canvas)
    # ... and at half resolution, as the heat-maps are stitched
    half = canvas[::2, ::2]
    assert np.array_equal(ts.stitch(np.stack([t[::2, ::2] for t in tiles]), p, shrink=2), half)


@pytest.mark.parametrize("name,tiles,canvas,boxes,crossing", [("A", 28, (160, 256), 11, 8), ("B", 6, (192, 256), 11, 7)])
def test_fixtures_are_not_vacuous(name, tiles, canvas, boxes, crossing):
    f = ts.fixture(name)
    assert len(f.plan.origins) == tiles and f.plan.canvas == canvas
    assert len(f.want) == boxes
    assert sum(ts.crosses_seam(np.asarray(box) * f.scale, f.plan) for _, box in f.want) == crossing
    assert sum(len(text) > 0 for text, _ in f.want) >= boxes - 1
    if name == "B":  # the canvas is the resized page: no pad
        assert f.canvas.shape[:2] == (f.page.shape[0] * f.scale, f.page.shape[1] * f.scale)
