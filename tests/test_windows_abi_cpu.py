"""include/kocr_windows.h held to what the suite holds include/kocr.h to (tests/test_abi_cpu.py, tests/test_workspace_cases_cpu.py),
without a GPU: every function it declares is exported by libkocr.so and has a ctypes signature of the declared length in
keras_ocr_amd/_lib.py; every one is the entry of a row of the workspace table in tests/windows_cases.py or named there as
taking no arena; and what reaches an arena reservation in csrc/windows.hip is what the table calls."""
import os
import re

import numpy as np
import pytest

from tests import windows_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = {"kocr_recognize_boxes_windowed", "kocr_windowed_results_shape", "kocr_windowed_results", "kocr_window_plan",
            "kocr_warp_crops_windowed", "kocr_ctc_stitch_decode"}


def _prototypes():
    """{name: number of parameters} of the header's declarations"""
    src = open(os.path.join(ROOT, "include", "kocr_windows.h"), encoding="utf-8").read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, params in re.findall(r"\bint\s+(kocr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        out[name] = len([p for p in params.split(",") if p.strip() and p.strip() != "void"])
    assert sorted(out) == sorted(set(re.findall(r"\b(kocr_[a-z0-9_]+)\s*\(", src)))  # nothing declared in another form
    return out


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__

    __graft_entry__.build()
    import keras_ocr_amd

    return keras_ocr_amd.load_library()


def test_the_header_declares_the_six_functions_and_kocr_h_none_of_them():
    assert set(_prototypes()) == EXPECTED
    main = open(os.path.join(ROOT, "include", "kocr.h"), encoding="utf-8").read()
    assert '"long words"' in open(os.path.join(ROOT, "include", "kocr_windows.h"), encoding="utf-8").read()
    assert "long words" in main and "kocr_windows.h" in main and "KOCR_WINDOW_FRAMES_MAX" in main  # the rule is stated there
    code = re.sub(r"/\*.*?\*/", "", main, flags=re.S)
    assert not EXPECTED & set(re.findall(r"\b(kocr_[a-z0-9_]+)\s*\(", code))


def test_every_declared_symbol_is_exported_with_a_ctypes_signature(lib):
    src = open(os.path.join(ROOT, "keras_ocr_amd", "_lib.py"), encoding="utf-8").read()
    for name, n_params in _prototypes().items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert f'"{name}"' in src, f"{name} has no ctypes signature"
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, (name, n_params, fn.argtypes)


def _arena_users():
    """the extern "C" functions of csrc/windows.hip whose body -- or a helper it calls, down to three levels -- names a Staging's
    reserve, arena_reserve or ws_reserve (tests/test_workspace_cases_cpu.py reads the .cpp files the same way)"""
    text = open(os.path.join(ROOT, "keras_ocr_amd", "csrc", "windows.hip"), encoding="utf-8").read()
    starts = [(m.start(), m.group(1)) for m in re.finditer(r"^(?:extern \"C\" |static )?(?:int|long|void) ([a-z_0-9]+)\(", text, re.M)]
    bodies = {fn: text[a:b] for (a, fn), (b, _) in zip(starts, starts[1:] + [(len(text), None)])}
    reach = {fn for fn, body in bodies.items() if re.search(r"\b(arena_reserve|ws_reserve)\(|\.reserve\(", body)}
    for _ in range(3):
        reach |= {fn for fn, body in bodies.items() if any(re.search(r"\b" + re.escape(d) + r"\(", body.split("{", 1)[-1]) for d in reach)}
    defined = {fn for fn in bodies if fn.startswith("kocr_")}
    return {fn for fn in reach if fn.startswith("kocr_")}, defined


def test_every_function_is_on_exactly_one_list_and_the_lists_agree_with_the_sources():
    declared = set(_prototypes())
    entries = {r["entry"] for r in wc.workspace_rows()}
    assert len(set(wc.NO_ARENA)) == len(wc.NO_ARENA) and not entries & set(wc.NO_ARENA)
    assert declared == entries | set(wc.NO_ARENA), (sorted(declared - entries - set(wc.NO_ARENA)), sorted((entries | set(wc.NO_ARENA)) - declared))
    users, defined = _arena_users()
    assert defined == declared, "csrc/windows.hip defines what the header declares"
    assert users == entries, (sorted(users - entries), sorted(entries - users))
    # ... and no .cpp file defines one of them, where tests/test_workspace_cases_cpu.py would look for it
    csrc = os.path.join(ROOT, "keras_ocr_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith(".cpp"):
            text = open(os.path.join(csrc, name), encoding="utf-8").read()
            assert not [fn for fn in declared if re.search(r"\b" + fn + r"\(", text)], name


def test_rows_are_well_formed():
    import keras_ocr_amd

    rows = wc.workspace_rows()
    assert len({r["name"] for r in rows}) == len(rows)
    for r in rows:
        assert callable(getattr(keras_ocr_amd.Context, r["method"], None)), r["name"]
        assert set(r["touches"]) <= {"ws", "pp", "pp2", "io", "pl", "bx", "chw", "chr"}, r["name"]
        args = r["args"]()
        assert isinstance(args, tuple), r["name"]
        if r["method"] in ("warp_crops_windowed", "recognize_boxes_windowed"):
            assert args[0].dtype == np.uint8 and args[0].ndim == 4 and len(args[1]) == len(args[0]), r["name"]
    # the edges the table is there for: a page without boxes, one crop, more than one recogniser batch, more boxes than a
    # workgroup of the plan kernels has lanes, a word of the longest kind beside words of one window
    from tests import windows_statement as ws
    assert any(any(len(g) == 0 for g in r["args"]()[1]) for r in rows if r["method"] == "warp_crops_windowed")
    totals = [int(ws.plan_boxes(np.concatenate([np.asarray(g).reshape(-1, 4, 2) for g in r["args"]()[1]]))[0].sum())
              for r in rows if r["method"] == "recognize_boxes_windowed"]
    assert 1 in totals and max(totals) > 1024
    assert any(len(r["args"]()[0]) > 256 for r in rows if r["method"] == "window_plan")
    assert any({1, 41} <= set(r["args"]()[1]) for r in rows if r["method"] == "ctc_stitch_decode")
