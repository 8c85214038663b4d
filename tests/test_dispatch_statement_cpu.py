"""tests/dispatch_statement.py against every kernel row the suite already asserts somewhere, and against the reading
written next to the boundary shapes of tests/dispatch_cases.py.  No GPU: the statement is plain Python."""
import ast
import os

import pytest

from tests import dispatch_cases as dc
from tests.dispatch_statement import BF16X3, F16X1, F16X2, ragged_geo, row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _literal(path, name):
    """a module-level list of tuples, read without importing the module (the GPU test modules import torch and mark
    themselves gpu)"""
    with open(os.path.join(ROOT, path), encoding="utf-8") as f:
        tree = ast.parse(f.read())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(isinstance(t, ast.Name) and t.id == name for t in node.targets):
            return ast.literal_eval(node.value)
    raise AssertionError(f"{name} not found in {path}")


SPLIT_CASES = _literal("tests/test_conv_gpu.py", "SPLIT_CASES")
DSPLIT_CASES = _literal("tests/test_conv_gpu.py", "DSPLIT_CASES")
K5_CASES = _literal("tests/test_conv_gpu.py", "K5_CASES")


def _bf16x3_family(family):
    """what tests/test_conv_gpu.py::_expect_family asserts in bf16x3 mode; None where it asserts nothing (the ragged
    grids exist in the fp16 kernels only)"""
    if family.endswith("_rag"):
        return None
    return family.replace("conv_w4hr", "conv_w4s").replace("conv_w4hf", "conv_w4s").replace("conv_w4h", "conv_w4").replace("conv_hh", "conv_hs")


def test_lists_were_found():
    assert len(SPLIT_CASES) >= 37 and len(DSPLIT_CASES) >= 9 and len(K5_CASES) >= 4


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[str(c) for c in SPLIT_CASES])
def test_split_cases_name_the_statements_row(case):
    n, h, w, cin, cout, family = case
    assert row(n, h, w, cin, cout, 3, 1, F16X2) == family
    want = _bf16x3_family(family)
    if want is not None:
        assert row(n, h, w, cin, cout, 3, 1, BF16X3) == want
    else:  # what took these shapes before the ragged grids: F(2,3) for an even width, else the fp32 kernel
        assert row(n, h, w, cin, cout, 3, 1, BF16X3).startswith(("conv_ws_", "conv_mfma_", "conv_w4s_", "conv_w4v_", "conv_w4t_"))


@pytest.mark.parametrize("case", DSPLIT_CASES, ids=[str(c) for c in DSPLIT_CASES])
def test_dsplit_cases_name_the_statements_row(case):
    n, h, w, cin, cout, k, dil, family = case
    assert row(n, h, w, cin, cout, k, dil, F16X2) == family
    assert row(n, h, w, cin, cout, k, dil, BF16X3) == _bf16x3_family(family)


@pytest.mark.parametrize("case", K5_CASES, ids=[str(c) for c in K5_CASES])
def test_k5_cases_reach_conv_k5(case):
    n, h, w, cin = case
    for mode in (BF16X3, F16X2, F16X1):
        assert row(n, h, w, cin, 16, 5, 1, mode).startswith("conv_k5")


@pytest.mark.parametrize("name,cin,cout", [("fc_9", 512, 128), ("lstm_10_xproj", 128, 1024), ("lstm_11_xproj", 256, 1024),
                                           ("fc_12", 256, 37)])
def test_recogniser_1x1_switch_at_4096_pixels(name, cin, cout):
    """tests/test_crnn_layers_gpu.py: 81 crops x 50 steps = 4050 pixels on conv_mfma, 82 x 50 = 4100 on conv_ds.  Whatever
    the layers' exact widths, the rows asserted there need Cin % 16 == 0 and more than 32 couts."""
    for mode in (BF16X3, F16X2):
        assert row(81, 50, 1, cin, cout, 1, 1, mode).startswith("conv_mfma"), name
        assert row(82, 50, 1, cin, cout, 1, 1, mode).startswith("conv_ds"), name
        assert row(1, 81 * 50, 1, cin, cout, 1, 1, mode).startswith("conv_mfma"), name
        assert row(1, 82 * 50, 1, cin, cout, 1, 1, mode).startswith("conv_ds"), name


def _detector_rows(h, w, mode):
    """the 3 x 3 layers of the detector (VGG16-bn backbone, U-Net decoder, head) on an h x w page, through launch_conv_pool"""
    h2, w2, h4, w4, h8, w8, h16, w16 = h // 2, w // 2, h // 4, w // 4, h // 8, w // 8, h // 16, w // 16
    layers = [(h, w, 64, 64, True), (h2, w2, 64, 128, False), (h2, w2, 128, 128, True), (h4, w4, 128, 256, False),
              (h4, w4, 256, 256, False), (h4, w4, 256, 256, True), (h8, w8, 256, 512, False), (h8, w8, 512, 512, False),
              (h8, w8, 512, 512, True), (h16, w16, 512, 512, False), (h16, w16, 512, 512, False),
              (h16, w16, 512, 256, False), (h8, w8, 256, 128, False), (h4, w4, 128, 64, False), (h2, w2, 64, 32, False),
              (h2, w2, 32, 32, False), (h2, w2, 32, 32, False), (h2, w2, 32, 16, False)]
    return [row(1, lh, lw, cin, cout, 3, 1, mode, pool=pool) for lh, lw, cin, cout, pool in layers]


def test_ragged_detector_page_rows():
    """tests/test_craft_gpu.py::test_heatmap_ragged_page_on_the_fp16_kernels, 375 x 500: the same four assertions"""
    rows = _detector_rows(375, 500, F16X2)
    assert any(k.startswith("conv_w4hv_256x128") and k.endswith("_rag") for k in rows), rows
    assert any(k.startswith("conv_w4hr_256x64") and k.endswith("_rag") for k in rows), rows
    assert any(k.startswith("conv_w4hv_256x128_pool") and k.endswith("_rag") for k in rows), rows
    assert not any(k.startswith(("conv_ws_", "conv_wino", "conv_w4s_256x128", "conv_w4s_512x64")) for k in rows), rows
    assert rows[0] == "conv_w4hr_256x64_pool_rag" and rows[-1] == "conv_hs_256x16" and rows[-2] == "conv_hh_256x32", rows


@pytest.mark.parametrize("table,mode", [(dc.DEFAULT, F16X2), (dc.BF16X3, BF16X3), (dc.F16X1, F16X1)], ids=["default", "bf16x3", "f16x1"])
def test_boundary_cases_land_where_they_are_read_to(table, mode):
    wrong = {c: (row(*c, mode), want) for c, want in table if row(*c, mode) != want}
    assert not wrong, wrong
    assert len({c for c, _ in table}) == len(table), "a case is listed twice"


@pytest.mark.parametrize("label,a,b", dc.PAIRS, ids=[p[0] for p in dc.PAIRS])
def test_every_pair_straddles_its_predicate(label, a, b):
    assert a in dc.DEFAULT_CASES and b in dc.DEFAULT_CASES, label
    assert row(*a, F16X2) != row(*b, F16X2), (label, row(*a, F16X2))


def test_geometry_only_predicates():
    """where a predicate changes geometry and the row's suffix with it: the stated geometries"""
    n, h, w, cin, cout, k, dil = dc.GEO_4X64
    assert ragged_geo(h, w, cin, cout, dil, F16X2) == 1
    n, h, w, cin, cout, k, dil = dc.GEO_8X32
    assert ragged_geo(h, w, cin, cout, dil, F16X2) == 2
    # pooling and the 64-cout kernel know 4 x 64 only
    assert ragged_geo(h, w, cin, cout, dil, F16X2, pool=True) == 1 and ragged_geo(h, w, cin, 64, dil, F16X2) == 1
    # 256 and 272 pixels run the same kernel: one image per tile against two (a fact of the shapes, not of a predicate)
    assert 16 * 16 == 256 and (17 * 16) % 256 != 0
    for c, share_ok in ((dc.SHARE_52, True), (dc.SHARE_48, False), (dc.SHARE_104, True), (dc.SHARE_100, False)):
        n, h, w, cin, cout, k, dil = c
        assert (ragged_geo(h, w, cin, cout, dil, F16X2) > 0) == share_ok, c
        assert ragged_geo(h, w, cin, cout, dil, BF16X3) == -1


def test_negative_control_has_three_one_piece_rows():
    assert sum(1 for _, r in dc.F16X1 if r.startswith("conv_w4q")) >= 3
    assert {dc.PIXELS_256, dc.PIXELS_272}.issubset(dc.F16X1_CASES) and set(dc.TINY_RAGGED).issubset(dc.F16X1_CASES)


def test_statement_is_integer_only():
    """no float literal and no true division in the statement: the padding shares are cross-multiplied"""
    with open(os.path.join(ROOT, "tests", "dispatch_statement.py"), encoding="utf-8") as f:
        tree = ast.parse(f.read())
    for node in ast.walk(tree):
        assert not (isinstance(node, ast.Constant) and isinstance(node.value, float)), node.lineno
        assert not (isinstance(node, ast.BinOp) and isinstance(node.op, ast.Div)), node.lineno
