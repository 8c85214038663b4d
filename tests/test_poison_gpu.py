"""No kernel reads workspace that its own call has not written: poison mode ("Poison mode").

Every buffer of a call comes from a bump arena or from the detector's lifetime pool, and both hand out bytes that were just used
for something else.  tests/test_workspace_gpu.py cannot see a missing initialisation: fresh device memory is in practice zero
and a region that nobody writes keeps its benign value, so cold, warm and "after the largest call" read the same.  With
kocr_debug_set_arena_poison every allocation is filled with one byte on the stream when it is made, and a call is run with the
mode off, under 0x00 and under 0xFF: a float, half or bf16 of 0xFF bytes is a NaN, an int32 / int64 is -1.  Results are compared
as bit patterns; there is no tolerance in this file.

  a  the mode is live   the box rows past counts[i] of a pipeline call (include/kocr.h: "rows >= counts[i] of an image
                        undefined") hold the byte, read back from the device: the proof that b and c can fail;
  b  the table          every row of tests/workspace_cases.py and tests/windows_cases.py (refusals excluded) from a cold
                        context: off, 0x00, 0xFF, 0xFF with arena guards -- the same bits four times, no guard damaged;
  c  inside one call    reuse that the table does not reach: the detector's pool at two sizes, under the four schedules and
                        the other two arithmetics, the KOCR_ECAPACITY rerun of the post-processing, ragged and pooled
                        convolutions, the recogniser on both sides of crnn_small_batch, 2 M oriented crops;
  d  off is off         after set_arena_poison(None) a pipeline call launches what a context that never saw the mode launches.

The rows of b are split by family (one test function each) so that a run can take the families one process at a time.

Limits.  fmax-style reductions and ordered comparisons swallow a NaN: a stale value that is read only into a maximum, or only
compared, is not seen under 0xFF unless it also differs from what 0x00 gives.  Positive finite poison words are left out on
purpose: as integers they are wild indices, while -1 stops a signed loop and an index of -1 stays next to its buffer."""
import ctypes

import numpy as np
import pytest

from tests import batch_edge_cases as bc
from tests import dispatch_cases as dc
from tests import windows_cases as winc
from tests import workspace_cases as wc
from tests.workspace_harness import _Contexts, _bits, _call, _prepare, _where

pytestmark = pytest.mark.gpu

MODES = (("off", None, False), ("0x00", 0x00, False), ("0xFF", 0xFF, False), ("0xFF+guards", 0xFF, True))
NETWORKS = dict(crnn=wc.DEFAULT_CRNN, craft=None, setup=[])  # what _prepare reads of a row


@pytest.fixture(scope="module")
def contexts():
    pool = _Contexts()
    yield pool
    pool.close()


def _under(c, byte, guards, call):
    """call() on the context made cold, in the given mode; (bits, damaged guards and where).  Both modes are off afterwards."""
    c.release_arenas()
    c.set_arena_poison(byte)
    c.set_arena_guards(guards)
    try:
        got = call()
        damage = c.check_arena_guards() if guards else (0, None, 0, 0)
    finally:
        c.set_arena_guards(False)
        c.set_arena_poison(None)
    return got, damage


def _same_in_every_mode(c, what, call, modes=MODES):
    want = None
    for label, byte, guards in modes:
        got, (damaged, arena, offset, at) = _under(c, byte, guards, call)
        assert damaged == 0, f"{what}: {label}: {damaged} damaged guards, the first in arena {arena} behind the buffer at offset {offset}: byte {at}"
        if want is None:
            want = got
        assert got == want, f"{what}: the call under {label} differs from the call with the mode off: {_where(got, want)}"
    c.release_arenas()


# ---- a. the mode is live ---------------------------------------------------------------------------------------------------
def test_unwritten_box_rows_hold_the_poison_byte(contexts):
    """cap above the box count: kocr_pipeline writes counts[i] box rows of image i and documents the rest of d_boxes
    [N][cap][4][2] as undefined.  Under 0xFF those rows are 0xFF bytes, then -- on the same, now warm, arena, so that the
    bytes are known to have been filled again -- 0x00 under 0x00; the written rows are the same in both."""
    r = wc.row("pipeline")
    c = _prepare(contexts.get(r["env"]), r)
    args, _ = wc.call_of(r)
    c.release_arenas()
    seen = {}
    try:
        for byte in (0xFF, 0x00):
            c.set_arena_poison(byte)
            out = c._pipeline(*args, 0.7, 0.4, 0.4, 10, 0, False, 256, None)  # pylint: disable=protected-access
            got = c.pipeline_device_results()
            counts = [len(b) for b in out.boxes]
            assert got["n"] == len(counts) == 2 and got["cap"] == 256 and 0 < max(counts) < got["cap"] and got["boxes"]
            dev = np.full((got["n"], got["cap"], 8), 0x5A5A5A5A, np.uint32)
            c._check(c._lib.kocr_memcpy_d2h(c._h, ctypes.c_void_p(dev.ctypes.data), ctypes.c_void_p(got["boxes"]), dev.nbytes))  # pylint: disable=protected-access
            for i, n in enumerate(counts):
                tail = dev[i, n:].view(np.uint8)
                assert tail.size and (tail == byte).all(), f"byte {byte:#04x}: image {i}: rows past {n} hold {np.unique(tail)[:8]}"
                assert dev[i, :n].tobytes() == np.ascontiguousarray(out.boxes[i], np.float32).tobytes()
            seen[byte] = _bits((out.boxes, out.labels))
    finally:
        c.set_arena_poison(None)
        c.release_arenas()
    assert seen[0xFF] == seen[0x00], _where(seen[0xFF], seen[0x00])


# ---- b. every row of the workspace tables ------------------------------------------------------------------------------------
def _family(family):
    return [r["name"] for r in wc.rows() if r["family"] == family and not r["raises"]]


def _table_row(contexts, name):
    r = wc.row(name)
    c = _prepare(contexts.get(r["env"]), r)
    _same_in_every_mode(c, name, lambda: _call(c, r))


@pytest.mark.parametrize("name", _family("other"))
def test_rows_other(contexts, name):
    _table_row(contexts, name)


@pytest.mark.parametrize("name", _family("detector"))
def test_rows_detector(contexts, name):
    _table_row(contexts, name)


@pytest.mark.parametrize("name", _family("recogniser"))
def test_rows_recogniser(contexts, name):
    _table_row(contexts, name)


@pytest.mark.parametrize("name", _family("pipeline"))
def test_rows_pipeline(contexts, name):
    _table_row(contexts, name)


@pytest.mark.parametrize("row", winc.workspace_rows(), ids=lambda r: r["name"])
def test_rows_windows(contexts, row):
    c = _prepare(contexts.get({}), NETWORKS)
    args = row["args"]()
    _same_in_every_mode(c, row["name"], lambda: _bits(getattr(c, row["method"])(*args)))


def test_the_table_is_run_whole():
    ran = [n for f in ("other", "detector", "recogniser", "pipeline") for n in _family(f)]
    assert sorted(ran) == sorted(r["name"] for r in wc.rows() if not r["raises"])
    assert set(wc.LARGEST) == {"other", "detector", "recogniser", "pipeline"}


# ---- c. reuse inside one call that the table does not reach ------------------------------------------------------------------
INSIDE = MODES[:3]


@pytest.fixture()
def detector(contexts):
    """the table's own detector context with the raw weights, schedule and arithmetic put back afterwards"""
    c = _prepare(contexts.get({}), dict(crnn=None, craft="raw", setup=[]))
    schedule, mode = c.get_schedule(), c.get_split_mode()
    yield c
    c.set_schedule(*schedule)
    c.set_split_mode(mode)


@pytest.mark.parametrize("hw", [(64, 96), (128, 192)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_craft_forward_pool_reuse(detector, hw):
    x = wc.detector_images(1, *hw)()
    _same_in_every_mode(detector, f"craft_forward 1x{hw[0]}x{hw[1]}", lambda: _bits(detector.craft_forward(x)), INSIDE)


@pytest.mark.parametrize("fold_linear_chain", [True, False], ids=["linfold", "no_linfold"])
@pytest.mark.parametrize("fold_upsample", [True, False], ids=["upfold", "no_upfold"])
def test_craft_forward_schedules(detector, fold_linear_chain, fold_upsample):
    x = wc.detector_images(2, 64, 96)()
    detector.set_schedule(fold_linear_chain, fold_upsample)
    assert detector.get_schedule() == (fold_linear_chain, fold_upsample)
    _same_in_every_mode(detector, f"craft_forward 2x64x96, schedule {(fold_linear_chain, fold_upsample)}",
                        lambda: _bits(detector.craft_forward(x)), INSIDE)


@pytest.mark.parametrize("mode", ["bf16x3", "f16x1"])
def test_craft_forward_arithmetics(detector, mode):
    x = wc.detector_images(1, 64, 96)()
    detector.set_split_mode(mode)
    _same_in_every_mode(detector, f"craft_forward 1x64x96, {mode}", lambda: _bits(detector.craft_forward(x)), INSIDE)


def test_pipeline_capacity_rerun(contexts):
    """cap = 1, max_crops = 1 (tests/test_chars_gpu.py): the post-processing runs again on the resident heat-maps with a box
    buffer of its own, KOCR_ECAPACITY, and everything is fetched from what stayed resident"""
    r = wc.row("pipeline")
    c = _prepare(contexts.get(r["env"]), r)
    args, _ = wc.call_of(r)
    plain = _bits(c.pipeline(*args))

    def call():
        out = c.pipeline(*args, cap=1, max_crops=1, return_scores=True, char_boxes=True)
        assert max(len(b) for b in out[0]) > 1 and _bits(out[:2]) == plain
        return _bits(out)
    _same_in_every_mode(c, "pipeline cap=1 max_crops=1", call, INSIDE)


@pytest.mark.parametrize("case", dc.TINY_RAGGED + [dc.PIXELS_272], ids=dc.case_id)
def test_conv2d_ragged(contexts, case):
    c = contexts.get({})["ctx"]
    p = dc.problem(case)
    _same_in_every_mode(c, f"conv2d_nhwc {dc.case_id(case)}",
                        lambda: _bits(c.conv2d_nhwc(p["x"], p["w"], dilation=case[6], pre_a=p["pre_a"], pre_b=p["pre_b"], relu=True)), INSIDE)


def test_conv2d_fused_pool_without_the_full_tensor(contexts):
    """conv + 2x2 max-pool in one launch, need_full=False: the full-resolution tensor is allocated and never written"""
    c = contexts.get({})["ctx"]
    x, w, pitch, wv = wc.conv_args((16, 104, 100, 8, 1, 128, 256))()

    def call():
        full, pooled, amax = c.conv2d_cells(x, w, pitch, wv, pool=True, need_full=False)
        assert full is None and pooled is not None
        return _bits((pooled, amax))
    _same_in_every_mode(c, "conv2d_cells pool, need_full=False", call, INSIDE)


@pytest.mark.parametrize("m", [82, 81])
def test_crnn_forward_at_the_small_batch_edge(contexts, m):
    """50 m pixels of the per-frame 1x1 layers: 4100 >= DSPLIT_MIN_PIXELS = 4096 > 4050 (csrc/common.h)"""
    c = _prepare(contexts.get({}), NETWORKS)
    x = bc.crops(m)
    _same_in_every_mode(c, f"crnn_forward M={m}", lambda: _bits(c.crnn_forward(x, return_probs=True)), INSIDE)


def test_recognize_boxes_oriented(contexts):
    """2 M candidate crops, the winners' rows compacted beside them"""
    r = wc.row("recognize_boxes-orientation")
    c = _prepare(contexts.get(r["env"]), r)
    _same_in_every_mode(c, r["name"], lambda: _call(c, r), INSIDE)


# ---- d. off is off -------------------------------------------------------------------------------------------------------
def _pipeline_launches(c, args):
    c.release_arenas()
    c.profile_enable(True)
    c.profile_reset()
    try:
        out = _bits(c.pipeline(*args))
        return out, {k: v["launches"] for k, v in c.profile_report().items()}
    finally:
        c.profile_enable(False)


def test_off_launches_what_an_untouched_context_launches(contexts):
    r = wc.row("pipeline")
    args, _ = wc.call_of(r)
    c = _prepare(contexts.get(r["env"]), r)
    c.set_arena_poison(0xFF)
    c.pipeline(*args)
    c.set_arena_poison(None)
    got, launches = _pipeline_launches(c, args)
    fresh = _Contexts()
    try:
        want, untouched = _pipeline_launches(_prepare(fresh.get(r["env"]), r), args)
    finally:
        fresh.close()
    assert launches == untouched and sum(launches.values()) > 20, (launches, untouched)
    assert got == want, _where(got, want)
