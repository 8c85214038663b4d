"""Every entry point's workspace plan on a COLD context, with guards ("Arena book-keeping").

The session's ``ctx`` has usually sized every arena for 1024 crops or a 28-tile page before a small shape runs, and the slack of
arena_reserve hides a plan that is short by up to an eighth; production's first call meets neither.  Every row of
tests/workspace_cases.py runs here on contexts of this module's own:

  1. cold    kocr_debug_release_arenas, the row's switches, the call: it succeeds (a refusal row raises what it documents);
  2. plan    every arena that was reserved: excess == 0 and peak <= requested; every arena that was touched was reserved, and
             the arenas the row is there for were;
  3. warm    the call again: the same bits; the family's largest call, then the row's call again: the same bits;
  4. guards  released again, guard mode on: the same bits, and no guard damaged (every batch is checked when its arena is emptied);
  5. kernel  the recogniser rows with the split-K dense kernel on: one ``dense_splitk`` launch per batch on the cold call
             (a short workspace used to select another kernel silently).

Integers and floats are compared as bit patterns; there is no tolerance in this file.  ``pytest -s`` prints, per row and
arena, peak / requested, and the last test prints the largest of each arena over the table."""
import collections
import ctypes

import numpy as np
import pytest

from tests import batch_edge_cases as bc
from tests import workspace_cases as wc
from tests.workspace_harness import _Contexts, _bits, _call, _prepare, _where

pytestmark = pytest.mark.gpu

# the Context methods that run the recogniser from crops (the others of its family start behind fc_12)
FORWARD_METHODS = {"crnn_forward", "crnn_forward_scores", "crnn_beam", "crnn_lexicon", "crnn_pattern", "crnn_ctc_loss", "crnn_features",
                   "recognize_boxes"}
TIGHTEST = collections.defaultdict(lambda: (0.0, None, 0, 0))  # arena -> (peak / requested, row, peak, requested)


@pytest.fixture(scope="module")
def contexts():
    pool = _Contexts()
    yield pool
    pool.close()


def _largest(c, r):
    """the family's largest call on the row's context as it stands: it sizes the arenas, its results do not matter"""
    name = wc.LARGEST[r["family"]]
    if name is None or name == r["name"]:
        return
    big = wc.row(name)
    if r["family"] == "recogniser" and not c.crnn_classes():
        return  # kocr_ctc_batch_cost needs no recogniser
    args, kwargs = wc.call_of(big)
    getattr(c, big["method"])(*args, **kwargs)


def _forward_batches(r):
    """the recogniser batches of a row that runs crnn_forward, or 0"""
    if r["method"] not in FORWARD_METHODS or r["raises"]:
        return 0
    args, kwargs = wc.call_of(r)
    m = sum(len(g) for g in args[1]) * (2 if kwargs.get("orientation") else 1) if r["method"] == "recognize_boxes" else len(args[0])
    return len(bc.pieces(m))


def _check_plan(c, r):
    stats = c.arena_stats()
    assert list(stats) == list(wc.ARENAS)
    for arena, s in stats.items():
        ratio = s["peak"] / s["requested"] if s["requested"] else 0.0
        if s["peak"] or s["requested"]:
            print(f"\n{r['name']}: {arena}: peak {s['peak']} / requested {s['requested']} = {ratio:.4f}, excess {s['excess']}, cap {s['cap']}")
        if ratio > TIGHTEST[arena][0]:
            TIGHTEST[arena] = (ratio, r["name"], s["peak"], s["requested"])
    for arena, s in stats.items():
        what = f"{r['name']}: arena {arena}: requested {s['requested']}, peak {s['peak']}, excess {s['excess']}"
        if s["requested"]:
            assert s["excess"] == 0 and s["peak"] <= s["requested"], f"{what}: the plan is short of what the call took"
        assert not s["peak"] or s["requested"], f"{what}: an allocation from an arena that this entry point never reserved"
    for arena in r["touches"]:
        assert stats[arena]["requested"] > 0, f"{r['name']}: arena {arena} was not reserved: the row does not take the path it is there for"


@pytest.mark.parametrize("name", wc.names())
def test_workspace_plan_cold_warm_and_guarded(contexts, name):
    r = wc.row(name)
    state = contexts.get(r["env"])
    c = _prepare(state, r)
    batches = _forward_batches(r)
    splitk = batches and r["crnn"][2] and r["env"].get("KOCR_DENSE_SPLITK") != "0"
    # 1. cold
    c.release_arenas()
    assert all(not any(s.values()) for s in c.arena_stats().values())
    if splitk:
        c.profile_enable(True)
        c.profile_reset()
    try:
        cold = _call(c, r)
        launches = {k: v["launches"] for k, v in c.profile_report().items()} if splitk else {}
    finally:
        c.profile_enable(False)
    # 2. plan
    _check_plan(c, r)
    # 3. warm equals cold
    warm = _call(c, r)
    assert warm == cold, f"{name}: the repeated call differs from the cold one: {_where(warm, cold)}"
    _largest(c, r)
    after = _call(c, r)
    assert after == cold, f"{name}: the call behind the family's largest differs from the cold one: {_where(after, cold)}"
    # 4. guards
    c.release_arenas()
    c.set_arena_guards(True)
    try:
        guarded = _call(c, r)
        damaged, arena, offset, byte = c.check_arena_guards()
    finally:
        c.set_arena_guards(False)
        c.release_arenas()
    assert guarded == cold, f"{name}: the call in guard mode differs from the cold one: {_where(guarded, cold)}"
    assert damaged == 0, f"{name}: {damaged} damaged guards, the first in arena {arena} behind the buffer at offset {offset}: byte {byte}"
    # 5. stn_dense_1 on the split-K kernel, once per batch
    if splitk:
        assert launches.get("dense_splitk") == batches, f"{name}: dense_splitk launches {launches.get('dense_splitk')} for {batches} batches"


# ---- the resident records ----------------------------------------------------------------------------------------------------
def _getters(c):
    lib, h, n = c._lib, c._h, None  # pylint: disable=protected-access
    return {
        "kocr_pipeline_device_results": lambda: lib.kocr_pipeline_device_results(h, n, n, n, n, n, n),
        "kocr_pipeline_results": lambda: lib.kocr_pipeline_results(h, n, 0, n, 0),
        "kocr_pipeline_results_shape": lambda: lib.kocr_pipeline_results_shape(h, n, n),
        "kocr_detection_scores": lambda: lib.kocr_detection_scores(h, n, 0),
        "kocr_recognition_scores": lambda: lib.kocr_recognition_scores(h, n, n, 0, n, n),
        "kocr_recognition_beams": lambda: lib.kocr_recognition_beams(h, n, n, 0, n, n, n),
        "kocr_recognition_lexicon": lambda: lib.kocr_recognition_lexicon(h, n, n, 0, n, n),
        "kocr_recognition_patterns": lambda: lib.kocr_recognition_patterns(h, n, n, n, 0, n),
        "kocr_recognition_orientation": lambda: lib.kocr_recognition_orientation(h, n, n, n, 0, n),
        "kocr_detection_char_boxes": lambda: lib.kocr_detection_char_boxes(h, n, n, n, 0, ctypes.c_int64(0), n),
    }


def _nothing_resident(c):
    from keras_ocr_amd._lib import KOCR_EINVAL

    for fn, get in _getters(c).items():
        rc = get()
        message = c._lib.kocr_last_error(c._h).decode()  # pylint: disable=protected-access
        assert rc == KOCR_EINVAL and fn in message and " no " in message and "resident" in message, (fn, rc, message)


def test_release_forgets_every_resident_result(contexts):
    from keras_ocr_amd.extras import Extras

    state = contexts.get({})
    c = _prepare(state, wc.row("pipeline-widest"))
    c.release_arenas()
    _nothing_resident(c)
    args, kwargs = wc.call_of(wc.row("pipeline-widest"))
    # the call's switches stay on for the getters
    with c._extras_scope(Extras(scores=True, lexicon_top=wc.TOP_WORDS, pattern=kwargs["pattern"], char_boxes=True)):  # pylint: disable=protected-access
        out = c._pipeline(*args, 0.7, 0.4, 0.4, 10, 0, False, 256, None)  # pylint: disable=protected-access
        counts = [len(b) for b in out.boxes]
        assert sum(counts) == len(out.labels) > 0
        got = c.pipeline_device_results()
        assert got["n"] == 2 and got["m"] == len(out.labels) and got["boxes"] and got["labels"]
        assert [len(s) for s in c.detection_scores(counts, 256)] == counts
        assert all(len(rows) == len(out.labels) for rows in c.recognition_scores() + c.recognition_beams() + c.recognition_lexicon() +
                   c.recognition_patterns())
        assert [len(words) for words in c.detection_char_boxes(counts, 256)] == counts
        c.release_arenas()
        _nothing_resident(c)
    c = _prepare(state, wc.row("pipeline-orientation"))
    args, kwargs = wc.call_of(wc.row("pipeline-orientation"))
    with c._extras_scope(Extras(orientation=(2, 1.5))):  # pylint: disable=protected-access
        out = c._pipeline(*args, 0.7, 0.4, 0.4, 10, 0, False, 256, None)  # pylint: disable=protected-access
        turns, quads, pairs = c.recognition_orientation()
        assert len(turns) == len(quads) == len(pairs) == len(out.labels) > 0
        c.release_arenas()
        _nothing_resident(c)


def test_a_changed_guard_byte_is_reported_with_its_place(contexts):
    """The guards are there and are compared on the device's memory: after a pipeline call in guard mode, ONE byte is copied
    from the host into the guard behind the resident label rows (kocr_memcpy_h2d into the context's own arena: no kernel
    writes anything).  The check names the io arena, and the byte is the first one behind that buffer; the next check is
    clean again.  (What a comparison sees of a damaged guard: scripts/host_arena_check.cpp.)"""
    state = contexts.get({})
    r = wc.row("pipeline")
    c = _prepare(state, r)
    args, _ = wc.call_of(r)
    c.release_arenas()
    c.set_arena_guards(True)
    try:
        out = c._pipeline(*args, 0.7, 0.4, 0.4, 10, 0, False, 256, None)  # pylint: disable=protected-access
        got = c.pipeline_device_results()
        rows_bytes = got["m"] * c.crnn_label_width() * 4
        assert got["m"] == len(out.labels) > 0 and got["labels"]
        byte = np.array([0x5A], np.uint8)
        c._check(c._lib.kocr_memcpy_h2d(c._h, ctypes.c_void_p(got["labels"] + rows_bytes), ctypes.c_void_p(byte.ctypes.data), 1))  # pylint: disable=protected-access
        damaged, arena, offset, at = c.check_arena_guards()
        assert (damaged, arena) == (1, "io") and at - offset == rows_bytes, (damaged, arena, offset, at, rows_bytes)
        assert c.check_arena_guards()[0] == 0
    finally:
        c.set_arena_guards(False)
        c.release_arenas()


def test_zz_the_tightest_plan_of_every_arena():
    """no assertion: the largest peak / requested per arena over the table, for the record (pytest -s)"""
    for arena in wc.ARENAS:
        ratio, name, peak, requested = TIGHTEST[arena]
        print(f"\narena {arena}: largest peak / requested {ratio:.4f} ({peak} / {requested}) in row {name}")
