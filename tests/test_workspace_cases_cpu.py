"""The case table of the workspace tests (tests/workspace_cases.py) against include/kocr.h, without a GPU: every ``kocr_``
function is the entry of a row or named as taking no arena, every row's arguments can be built and have the shapes its
Context method takes, and the edge cases the table is there for are in it -- decided, where a path depends on the inputs, by
the project's own CPU statements."""
import os
import re

import numpy as np
import pytest

from tests import lexicon_statement as ls
from tests import pattern_statement as ps
from tests import tiling_statement as ts
from tests import workspace_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "kocr.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)  # prototypes only
    return sorted(set(re.findall(r"\b(kocr_[a-z0-9_]+)\s*\(", src)))


def _arena_users():
    """the functions of csrc that reach an arena, read off the sources: an extern "C" definition whose body -- or a helper it
    calls, one level down -- names arena_reserve, ws_reserve or a Staging's reserve"""
    csrc = os.path.join(ROOT, "keras_ocr_amd", "csrc")
    bodies = {}
    for name in sorted(os.listdir(csrc)):
        if not name.endswith(".cpp"):
            continue
        text = open(os.path.join(csrc, name), encoding="utf-8").read()
        starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(?:extern \"C\" |static )?(?:int|long|void|size_t|const char\*) ([a-z_0-9:]+)\(", text, re.M)]
        for (a, fn), (b, _) in zip(starts, starts[1:] + [(len(text), None)]):
            bodies[fn] = text[a:b]
    direct = {fn for fn, body in bodies.items() if re.search(r"\b(arena_reserve|ws_reserve)\(|\.reserve\(", body) and fn != "arena_reserve"}
    direct -= {"kocr_ctx::ws_reserve", "taps_begin"}
    reach = set(direct)
    for _ in range(3):
        reach |= {fn for fn, body in bodies.items() if any(re.search(r"\b" + re.escape(d) + r"\(", body.split("{", 1)[-1]) for d in reach)}
    return {fn for fn in reach if fn.startswith("kocr_")}


def test_every_function_of_the_header_is_on_exactly_one_list():
    declared = _declared()
    entries = {r["entry"] for r in wc.rows()}
    assert len(set(wc.NO_ARENA)) == len(wc.NO_ARENA)
    both = sorted(entries & set(wc.NO_ARENA))
    assert not both, f"on both lists: {both}"
    neither = sorted(set(declared) - entries - set(wc.NO_ARENA))
    assert not neither, f"new entry points without a row in tests/workspace_cases.py (or a place on NO_ARENA): {neither}"
    unknown = sorted((entries | set(wc.NO_ARENA)) - set(declared))
    assert not unknown, f"not declared in include/kocr.h: {unknown}"


def test_the_lists_agree_with_the_sources():
    """what reaches arena_reserve / Staging::reserve / ws_reserve in csrc is what the table calls"""
    users = _arena_users()
    entries = {r["entry"] for r in wc.rows()}
    assert users == entries, (sorted(users - entries), sorted(entries - users))


def test_rows_are_well_formed():
    import keras_ocr_amd

    assert len(set(wc.names())) == len(wc.names())
    for r in wc.rows():
        method = getattr(keras_ocr_amd.Context, r["method"], None)
        assert callable(method), r["name"]
        assert r["family"] in wc.LARGEST and set(r["touches"]) <= set(wc.ARENAS), r["name"]
        assert set(r["env"]) <= {"KOCR_CELLS", "KOCR_W43", "KOCR_DENSE_SPLITK"}, r["name"]
        assert r["crnn"] is None or (r["crnn"][0] in (37, 96, 1000) and r["crnn"][1] in (0, 2, 5) and r["crnn"][2] in (True, False)), r["name"]
        assert r["craft"] in (None, "raw", "page", "A"), r["name"]
        for m, args in wc.setup_of(r):
            assert callable(getattr(keras_ocr_amd.Context, m, None)) and isinstance(args, tuple), (r["name"], m)
        if r["craft"] == "A" or "tiled" in r["name"] or r["name"] in ("detect", "detect-scores-char_boxes"):
            continue  # arguments that the oracle's resize builds: the GPU test builds them
        args, kwargs = wc.call_of(r)
        assert isinstance(args, tuple) and isinstance(kwargs, dict), r["name"]
        if r["method"].startswith("crnn_") and "decode_logits" not in r["method"] and r["method"] != "ctc_batch_cost":
            classes, discard, _ = r["crnn"]
            assert args[0].dtype == np.float32 and args[0].shape[1:] == (31, 200), r["name"]
        if "decode_logits" in r["method"]:
            assert args[0].dtype == np.float32 and args[0].shape[1:] == (50, r["crnn"][0]), r["name"]
        if r["method"] == "recognize_boxes":
            assert args[0].dtype == np.uint8 and args[0].ndim == 4 and len(args[1]) == len(args[0]), r["name"]
            m = sum(len(g) for g in args[1])
            for key in ("set_of", "pattern_of"):
                assert key not in kwargs or len(kwargs[key]) == m, r["name"]
        if r["method"] == "get_boxes":
            assert args[0].dtype == np.float32 and args[0].ndim == 4 and args[0].shape[3] == 2, r["name"]
    for family, name in wc.LARGEST.items():
        assert name is None or wc.row(name)["family"] == family


def _rows(entry, **where):
    return [r for r in wc.rows() if r["entry"] == entry and all(r[k] == v for k, v in where.items())]


def _crops_of(r):
    return len(wc.call_of(r)[0][0])


def test_the_recogniser_family_has_its_edges():
    for entry in ("kocr_crnn_forward", "kocr_crnn_forward_scores", "kocr_crnn_beam", "kocr_crnn_lexicon", "kocr_crnn_pattern",
                  "kocr_crnn_ctc_loss", "kocr_crnn_features"):
        sizes = {_crops_of(r) for r in _rows(entry, env={}, crnn=wc.DEFAULT_CRNN)}
        assert set(wc.CRNN_M) <= sizes, (entry, sizes)
    for env in (wc.DENSE_52, wc.DENSE_50):
        assert {_crops_of(r) for r in wc.rows() if r["env"] == env} >= set(wc.CRNN_M), env
    assert any(_crops_of(r) == 1025 for r in _rows("kocr_crnn_forward_scores"))
    assert any(sum(len(g) for g in wc.call_of(r)[0][1]) == 1025 for r in _rows("kocr_recognize_boxes"))
    builds = {r["crnn"] for r in wc.rows() if r["crnn"]}
    assert {(37, 2, True), (37, 2, False), (37, 0, True), (37, 5, True), (96, 2, True), (1000, 2, True)} <= builds
    beams = [wc.call_of(r)[0][1:] for r in _rows("kocr_crnn_beam")]
    assert beams and all(b == (64, 64) for b in beams)


def test_the_lexicon_rows_take_the_paths_they_name():
    labels, lengths = wc.lexicon(37)
    v = len(labels)
    assert max(ls.frames_needed(labels[i][:lengths[i]]) for i in range(v)) <= 48  # every word has an alignment
    for r in _rows("kocr_crnn_lexicon"):
        scratch = dict(wc.setup_of(r)).get("set_lexicon_scratch")
        m = _crops_of(r)
        if "one_crop_chunks" in r["name"]:
            assert max(1, min(m, scratch[0] // (4 * v))) == 1 and m > 1, r["name"]  # lexicon_chunk (csrc/crnn.cpp)
        else:
            assert scratch is None, r["name"]
    assert {bool(r["kwargs"].get("return_values")) for r in _rows("kocr_crnn_lexicon") if "one_crop_chunks" in r["name"]} == {False, True}
    # the table of a crop's log q: it stays in LDS at 37 and 96 classes and leaves it at 1000
    assert 48 * 96 * 4 <= wc.LDS_BYTES < 48 * 1000 * 4
    assert _rows("kocr_crnn_lexicon", crnn=(1000, 2, True))


def _pattern_extent(classes, used):
    from keras_ocr_amd import patterns as kp
    pats = wc.patterns(classes)
    return max(len(pats.delta[k]) + kp.label_nodes(pats.delta[k]) for k in used), max(len(pats.delta[k]) for k in used)


def _bp_leave_lds(classes, frames, nodes, states):
    """the LDS plan of the pattern launch (csrc/crnn_kernels.hip: pattern_lds), as tests/test_patterns_gpu.py states it"""
    fixed = (2 * nodes + 4 * states + 2 * 256) * 4
    table = frames * classes * 4
    fixed += table if fixed + table <= wc.LDS_BYTES else 0
    return fixed + frames * nodes * 2 > wc.LDS_BYTES


def test_the_pattern_rows_take_the_paths_they_name():
    rows = _rows("kocr_crnn_pattern")
    per_crop = [r for r in rows if "per_crop" in r["name"]]
    assert per_crop
    for r in per_crop:
        of = wc.call_of(r)[0][1]
        every = set(range(-1, len(wc.patterns(r["crnn"][0]))))
        assert -1 in of and len(set(of.tolist())) == min(len(of), len(every)) and set(of.tolist()) <= every, r["name"]
    assert any(len(set(wc.call_of(r)[0][1].tolist())) == len(wc.patterns(37)) + 1 for r in per_crop)  # every pattern and none
    none =[r for r in rows if "-none-" in r["name"]]
    assert {r["crnn"][0] for r in none} == {37, 1000} and all((wc.call_of(r)[0][1] == -1).all() for r in none)
    # `.{0,40}` at 96 classes: the statement accepts 40 characters and no 41, and its back-pointers leave LDS; `plate` stays
    pats = wc.patterns(96)
    k = pats.names.index("upto40")
    assert pats.accepts(k, [1] * 40) and not pats.accepts(k, [1] * 41)
    lq = np.log(np.full((48, 96), 1 / 96))
    assert ps.viterbi(lq, pats.delta[k], pats.accept[k])[1] is not None
    assert _bp_leave_lds(96, 48, *_pattern_extent(96, [k]))
    assert not _bp_leave_lds(37, 48, *_pattern_extent(37, [wc.patterns(37).names.index("plate")]))
    assert [r for r in rows if "upto40" in r["name"] and r["crnn"][0] == 96]
    # a batch of -1 rows runs with one node and one state: nothing leaves LDS but the 1000-class table
    assert not _bp_leave_lds(1000, 48, 1, 1) and 48 * 1000 * 4 > wc.LDS_BYTES


def test_the_stage_rows_cover_every_extra_alone_and_together():
    rows = _rows("kocr_recognize_boxes") + _rows("kocr_recognize_boxes_patterns") + _rows("kocr_recognize_boxes_charsets")
    alone = {frozenset(k for k in r["kwargs"]) for r in rows if len(r["kwargs"]) == 1}
    assert {frozenset([k]) for k in ("return_scores", "beam", "lexicon_top", "pattern", "pattern_of", "set_of", "orientation")} <= alone
    widest = wc.row("recognize_boxes-everything-refused")
    assert set(widest["kwargs"]) == {"return_scores", "beam", "lexicon_top", "pattern"} and ("set_charset", (1,)) in wc.setup_of(widest)
    assert widest["raises"] and widest["raises"][0] is ValueError
    assert wc.row("recognize_boxes-widest-pattern")["raises"] is None and wc.row("recognize_boxes-widest-charset")["raises"] is None


def test_the_detector_and_pipeline_rows_have_their_edges():
    shapes = {wc.call_of(r)[0][0].shape for r in _rows("kocr_craft_forward")}
    assert {(1, 16, 16, 3), (3, 16, 16, 3), (1, 64, 96, 3)} <= shapes
    boxes = _rows("kocr_get_boxes")
    assert not wc.call_of(wc.row("get_boxes-no_components"))[0][0].any()
    assert any(r["kwargs"].get("cap") == 1 for r in boxes)
    assert {r["kwargs"].get("min_area_rect") for r in boxes} >= {"exact", "opencv"}
    assert any(r["kwargs"].get("return_scores") for r in boxes) and any(r["kwargs"].get("char_boxes") for r in boxes)
    assert all({"chw", "chr"} <= set(r["touches"]) for r in wc.rows() if r["kwargs"].get("char_boxes"))
    # fixture A is a page of more than one tile in both directions
    (h, w, _, _), scale, tile, overlap = ts.FIXTURES["A"]
    plan = ts.plan(h * scale, w * scale, tile, overlap)
    assert plan.counts == (4, 7) and plan.canvas == (160, 256)
    for entry in ("kocr_pipeline", "kocr_pipeline_tiled"):
        assert {bool(r["kwargs"].get("orientation")) for r in _rows(entry)} == {False, True}, entry
    assert "bx" in wc.row("pipeline-cap1")["touches"]


@pytest.mark.parametrize("name", ["resize_pad-batch3", "resize_pad_f32-batch3", "warp_quads", "score_tables", "compute_maps", "conv2d_cells"])
def test_a_spliced_argument_list_fits_its_method(name):
    import inspect
    import keras_ocr_amd

    r = wc.row(name)
    args, kwargs = wc.call_of(r)
    inspect.signature(getattr(keras_ocr_amd.Context, r["method"])).bind(None, *args, **kwargs)
