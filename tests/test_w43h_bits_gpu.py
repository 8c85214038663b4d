"""The fp16 F(4,3) kernels (csrc/conv_w43h.hip) write the bits they wrote before their input transform was rewritten per
component (scalar fp32 instructions instead of packed ones beside the MFMAs): outputs and per-image max-|x| slots of the
cases of tests/w43h_bits_cases.py against SHA-256 digests recorded with the earlier build (tests/golden/w43h_bits.json,
written by tests/golden/make_w43h_bits.py on the GPU).  One pass over the cases, shared by the tests."""
import json
import os

import pytest

from tests import w43h_bits_cases as wb

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "w43h_bits.json")


@pytest.fixture(scope="module")
def want():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got(ctx, craft_weights, crnn_weights):
    return wb.digests(ctx, craft_weights, crnn_weights)


def _rows(recs):
    return {r for rec in recs.values() for r in rec["kernel"].split("+") if r}


def _compare(got, want, label):
    assert sorted(got) == sorted(want), f"{label}: launches {sorted(set(got) ^ set(want))} differ from the recorded ones"
    wrong_row = {k: (got[k]["kernel"], want[k]["kernel"]) for k in want if got[k]["kernel"] != want[k]["kernel"]}
    assert not wrong_row, f"{label}: (kernel rows that ran, rows recorded) {wrong_row}"
    wrong = [f"{k}[{part}] ({want[k]['kernel']})" for k in want for part in ("out", "pool") if got[k].get(part) != want[k].get(part)]
    print(f"{label}: {len(want)} launches, rows {sorted(_rows(want))}, {len(wrong)} digests differ")
    assert not wrong, f"{label}: bits differ from the recorded build in {wrong}"


def test_fixture_reaches_every_loop_form(want):
    """the recorded rows cover the wide kernel on 4 x 64 (pooled and plain) and 8 x 32 tiles, exact, ragged and cells, the
    64-cout kernel pooled and plain, the flattened kernel plain and dilated (the dilated one as a single layer: at the
    8 x 8 level of a 128 x 128 page the composite is below its 256 pixels), and the one-piece rows"""
    single = _rows(want["single"])
    assert {"conv_w4hv_256x128", "conv_w4hv_256x128_rag", "conv_w4ht_256x128", "conv_w4ht_256x128_rag", "conv_w4hr_256x64",
            "conv_w4hr_256x64_rag", "conv_w4hf_256x128", "conv_w4hf_256x128_dil"} <= single, single
    assert {"conv_w4qv_256x128", "conv_w4qt_256x128", "conv_w4qr_256x64", "conv_w4qf_256x128"} <= _rows(want["single_f16x1"])
    craft = _rows(want["craft"]["2x128x128"])
    assert {"conv_w4hr_256x64_pool", "conv_w4hv_256x128_pool", "conv_w4hv_256x128", "conv_w4ht_256x128",
            "conv_w4hf_256x128"} <= craft, craft
    ragged = _rows(want["craft"]["1x100x140"])
    assert {"conv_w4hv_256x128_pool_rag", "conv_w4hv_256x128_rag", "conv_w4ht_256x128_rag", "conv_w4hr_256x64_rag"} <= ragged, ragged
    crnn = _rows(want["crnn"][str(wb.N_CROPS)])
    assert {"conv_w4hv_256x128_pool_cells", "conv_w4hv_256x128_cells", "conv_w4ht_256x128_cells"} <= crnn, crnn


def test_single_layers_keep_their_bits(got, want):
    _compare(got["single"], want["single"], "single layers, f16x2")


def test_single_layers_keep_their_bits_f16x1(got, want):
    _compare(got["single_f16x1"], want["single_f16x1"], "single layers, f16x1")


@pytest.mark.parametrize("key", list(wb.CRAFT_PAGES))
def test_craft_taps_keep_their_bits(got, want, key):
    _compare(got["craft"][key], want["craft"][key], f"CRAFT {key}")


def test_recogniser_taps_keep_their_bits(got, want):
    _compare(got["crnn"][str(wb.N_CROPS)], want["crnn"][str(wb.N_CROPS)], f"recogniser, {wb.N_CROPS} crops")
