"""The moments when a context changes what it holds ("What a context owns and when it lets go";
include/kocr.h at kocr_load_craft): weight reloads, refused loads, tables replaced, and the device memory a context owns.

  (a) a reloaded context IS a fresh one     A -> B on one context == a context that only ever saw B: the same bits in every
                                            arithmetic mode, the same persistent allocations, the same arena capacities
  (b) reloads hold no more memory           five reloads of each network with a forward between them
  (c) a refused load changes nothing        one defect per case on a context that has loaded and run; on a fresh context every
                                            forward is then refused before any launch, and a good load equals a fresh context
  (d) tables                                lexicon, character sets, patterns: replaced, unloaded, refused, dropped by a class change
  (e) calls own nothing new                 every row of tests/workspace_cases.py three times; kocr_conv2d_nhwc as a first call
  (f) contexts                              create / load / run / close ten times: the process holds what it held before

Every context is the test's own (the rows of (e) run on the pool of tests/workspace_harness.py) and is closed in a ``finally``.
Every comparison is bit for bit or of exact integers; the memory figures are counted by the library where it allocates
(kocr_debug_memory_stats), never read from the device, whose free memory moves with other processes' work.
``pytest -s`` prints the seconds of every load."""
import contextlib
import ctypes
import re
import time

import numpy as np
import pytest

from tests import lifecycle_cases as lc
from tests import workspace_cases as wc
from tests.workspace_harness import _Contexts, _bits, _call, _prepare, _where

pytestmark = pytest.mark.gpu

ENOWEIGHTS = r"libkocr error -3"
EINVAL = r"libkocr error -1"


@contextlib.contextmanager
def _context():
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    try:
        yield c
    finally:
        c.close()


def _timed_load(c, which, weights):
    t0 = time.perf_counter()
    getattr(c, "load_" + which)(weights)
    print(f"\nload_{which}: {time.perf_counter() - t0:.2f} s")


def _mem(c):
    m = c.debug_memory()
    return {k: m[k] for k in ("persistent_count", "persistent_bytes", "arena_bytes")}


def _persistent(c):
    m = c.debug_memory()
    return m["persistent_count"], m["persistent_bytes"]


def _crnn_forwards(c, rows=None):
    """labels and probabilities of both batches in every mode, as bits; ``rows`` collects the profiler rows of the launches"""
    out = []
    for mode in lc.MODES:
        c.set_split_mode(mode)
        if rows is not None:
            c.profile_reset()
            c.profile_enable(True)
        for m in lc.CRNN_BATCHES:
            out.append(_bits(c.crnn_forward(lc.crops(m), return_probs=True)))
        if rows is not None:
            rows.update(c.profile_report())
            c.profile_enable(False)
    c.set_split_mode(lc.MODES[0])
    return tuple(out)


def _craft_forwards(c, pages=lc.DETECTOR_PAGES, rows=None):
    out = []
    for mode in lc.MODES:
        c.set_split_mode(mode)
        if rows is not None:
            c.profile_reset()
            c.profile_enable(True)
        for p in pages:
            out.append(_bits(c.craft_forward(lc.page(*p))))
        if rows is not None:
            rows.update(c.profile_report())
            c.profile_enable(False)
    c.set_split_mode(lc.MODES[0])
    return tuple(out)


# ---- the references: a context that only ever saw B, computed once per weight set and shared (read-only) -------------------------
_FRESH = {}


def _fresh(which, **kwargs):
    """(bits of the forwards, memory, profiler rows of those forwards) of a fresh context with the set"""
    key = (which, tuple(sorted(kwargs.items())))
    if key not in _FRESH:
        rows = {}
        with _context() as c:
            if which == "crnn":
                _timed_load(c, "crnn", lc.crnn_set(**kwargs))
                bits = _crnn_forwards(c, rows)
            else:
                _timed_load(c, "craft", lc.craft_set(**kwargs))
                bits = _craft_forwards(c, rows=rows)
            _FRESH[key] = (bits, _mem(c), frozenset(rows))
    return _FRESH[key]


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,a,b", lc.CRNN_TRANSITIONS, ids=[t[0] for t in lc.CRNN_TRANSITIONS])
def test_reloaded_recogniser_equals_a_fresh_one(name, a, b):
    want, want_mem, rows = _fresh("crnn", **b)
    with _context() as c:
        c.load_crnn(lc.crnn_set(**a))
        first = _crnn_forwards(c)
        c.load_crnn(lc.crnn_set(**b))
        assert c.crnn_classes() == b.get("classes", 37) and c.crnn_label_width() == 48
        got = _crnn_forwards(c)
        assert got == want, f"{name}: the reloaded context computes something else: {_where(got, want)}"
        assert _mem(c) == want_mem, f"{name}: the reloaded context holds {_mem(c)}, a fresh one {want_mem}"
    if a != b:
        assert first != want, f"{name}: A and B compute the same: the transition shows nothing"
    # the recogniser's own derived copy (lifecycle_cases.DETECTOR_UNREACHED): stn_conv_1 on the 5x5 kernel
    assert any(re.match(lc.DERIVED_COPIES["d_k5"], r) for r in rows) == b.get("stn", True), sorted(rows)


@pytest.mark.parametrize("name,a,b", lc.CRAFT_TRANSITIONS, ids=[t[0] for t in lc.CRAFT_TRANSITIONS])
def test_reloaded_detector_equals_a_fresh_one(name, a, b):
    want, want_mem, _ = _fresh("craft", **b)
    with _context() as c:
        _timed_load(c, "craft", lc.craft_set(**a))
        first = _craft_forwards(c)
        _timed_load(c, "craft", lc.craft_set(**b))
        got = _craft_forwards(c)
        assert got == want, f"{name}: the reloaded context computes something else: {_where(got, want)}"
        assert _mem(c) == want_mem, f"{name}: the reloaded context holds {_mem(c)}, a fresh one {want_mem}"
    if a != b:
        assert first != want, f"{name}: A and B compute the same: the transition shows nothing"


def test_the_compared_detector_forwards_read_every_derived_copy():
    """The coverage condition: over all modes and pages together, the compared detector forwards launch a kernel family that
    reads each derived pointer of release_layer's list -- or the pointer is in DETECTOR_UNREACHED with its reason."""
    rows = set()
    for _, _, b in lc.CRAFT_TRANSITIONS:  # the shapes and the modes decide the kernels, not the weights: the sets agree
        rows |= _fresh("craft", **b)[2]
    print("\nprofiler rows of the compared detector forwards:", sorted(rows))
    for pointer, pattern in lc.DERIVED_COPIES.items():
        reached = sorted(r for r in rows if re.match(pattern, r))
        if pointer in lc.DETECTOR_UNREACHED:
            assert not reached, f"{pointer} is listed as unreached, but {reached} read it: take it off the list"
        else:
            assert reached, f"no compared detector forward reads {pointer} (rows {pattern}): a stale copy of it could not show"
    # the uint8 page reads the normalisation table, the float32 page does not take the uint8 first layer
    assert any(r.startswith("conv_hs_first_") for r in rows)


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
def test_recogniser_reloads_hold_no_more_memory():
    sets = [lc.crnn_set(seed=4321), lc.crnn_set(seed=5)]
    with _context() as c:
        c.load_crnn(sets[0])
        c.crnn_forward(lc.crops(3))
        first = _persistent(c)
        for k in range(1, 6):
            c.load_crnn(sets[k % 2])
            c.crnn_forward(lc.crops(3))
            now = _persistent(c)
            print(f"\nreload {k}: persistent (count, bytes) {now}, after load 1 {first}")
            assert now == first, f"reload {k}: {now[0] - first[0]} allocations / {now[1] - first[1]} bytes more than after load 1"


def test_detector_reloads_hold_no_more_memory():
    sets = [lc.craft_set(seed=1234), lc.craft_set(seed=7)]
    with _context() as c:
        _timed_load(c, "craft", sets[0])
        c.craft_forward(lc.page(32, 48, "u8"))
        first = _persistent(c)
        for k in range(1, 6):
            _timed_load(c, "craft", sets[k % 2])
            c.craft_forward(lc.page(32, 48, "u8"))
            now = _persistent(c)
            print(f"\nreload {k}: persistent (count, bytes) {now}, after load 1 {first}")
            assert now == first, f"reload {k}: {now[0] - first[0]} allocations / {now[1] - first[1]} bytes more than after load 1"


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
def _load_tables(c, classes=37):
    c.set_lexicon(*lc.lexicon(classes, 50))
    c.set_charsets(lc.charsets(classes, 3))
    c.set_patterns(*lc.patterns(classes, lc.TWO_PATTERNS[classes]))


def _table_answers(c):
    """what the three tables answer for three crops, as bits"""
    x = lc.crops(3)
    lex = _bits(c.crnn_lexicon(x, 3))
    c.set_charset(1)
    try:
        sets = _bits(c.crnn_forward(x, return_probs=True))
    finally:
        c.set_charset(-1)
    return lex, sets, _bits(c.crnn_pattern(x, np.array([0, 1, -1], np.int32)))


@pytest.mark.parametrize("name,tensor,what,b,damage", lc.CRNN_DEFECTS, ids=[d[0] for d in lc.CRNN_DEFECTS])
def test_refused_recogniser_load_changes_nothing(name, tensor, what, b, damage):
    with _context() as c:
        c.crnn_set_rnn_steps_to_discard(5)
        c.load_crnn(lc.crnn_set(seed=4321))
        _load_tables(c)
        before, tables, mem = _crnn_forwards(c), _table_answers(c), c.debug_memory()
        with pytest.raises(Exception, match=f"{EINVAL}: kocr_load_crnn: .*{what}") as e:
            c.load_crnn(damage(lc.crnn_set(**b)))
        assert tensor in str(e.value) and what in str(e.value), str(e.value)
        assert c.debug_memory() == mem
        assert c.crnn_classes() == 37 and c.crnn_label_width() == 45
        assert (c.lexicon_size(), c.charset_count(), c.pattern_count()) == (50, 3, 2)
        after = _crnn_forwards(c)
        assert after == before, f"{name}: the forwards changed after the refused load: {_where(after, before)}"
        assert _table_answers(c) == tables
        assert _mem(c) == {k: mem[k] for k in _mem(c)}


@pytest.mark.parametrize("name,tensor,what,b,damage", lc.CRAFT_DEFECTS, ids=[d[0] for d in lc.CRAFT_DEFECTS])
def test_refused_detector_load_changes_nothing(name, tensor, what, b, damage):
    with _context() as c:
        _timed_load(c, "craft", lc.craft_set(seed=1234))
        before, mem = _craft_forwards(c, lc.SMALL_PAGES), c.debug_memory()
        with pytest.raises(Exception, match=f"{EINVAL}: kocr_load_craft: .*{what}") as e:
            c.load_craft(damage(lc.craft_set(**b)))
        assert tensor in str(e.value), str(e.value)
        assert c.debug_memory() == mem
        after = _craft_forwards(c, lc.SMALL_PAGES)
        assert after == before, f"{name}: the forwards changed after the refused load: {_where(after, before)}"
        assert _mem(c) == {k: mem[k] for k in _mem(c)}


def _pipeline_args():
    p = wc.page()
    return [p], [64], [96], [128], [192], 128, 192


def _refused_without_a_launch(c, calls):
    """every call raises KOCR_ENOWEIGHTS, and the profiler has seen no launch"""
    c.profile_reset()
    c.profile_enable(True)
    for what, call in calls:
        with pytest.raises(Exception, match=ENOWEIGHTS):
            call()
            pytest.fail(f"{what} was not refused")
    assert c.profile_report() == {}, f"launches before the refusal: {sorted(c.profile_report())}"
    c.profile_enable(False)


def test_refused_first_recogniser_load_leaves_no_recogniser():
    x, lab = lc.crops(3), wc.bc.ctc_inputs(3, 48, 37)
    boxes = wc.box_groups((5, 4))()
    with _context() as c:
        for _, tensor, what, b, damage in lc.CRNN_DEFECTS[:1] + lc.CRNN_DEFECTS[-1:]:
            with pytest.raises(Exception, match=f"{EINVAL}: kocr_load_crnn: {what} {tensor}"):
                c.load_crnn(damage(lc.crnn_set(**b)))
        assert c.crnn_classes() == 0 and _persistent(c) == (0, 0)
        _refused_without_a_launch(c, [
            ("crnn_forward", lambda: c.crnn_forward(x)),
            ("crnn_forward_scores", lambda: c.crnn_forward_scores(x)),
            ("crnn_beam", lambda: c.crnn_beam(x, 4, 2)),
            ("crnn_features", lambda: c.crnn_features(x)),
            ("crnn_ctc_loss", lambda: c.crnn_ctc_loss(x, *lab)),
            ("recognize_boxes", lambda: c.recognize_boxes(wc.box_pages(), boxes)),
            ("recognize_boxes_windowed", lambda: c.recognize_boxes_windowed(wc.box_pages(), boxes)),
            ("pipeline", lambda: c.pipeline(*_pipeline_args())),
            ("set_lexicon", lambda: c.set_lexicon(*lc.lexicon(37, 50))),
            ("set_charsets", lambda: c.set_charsets(lc.charsets(37, 3))),
            ("set_patterns", lambda: c.set_patterns(*lc.patterns(37, ("plate",)))),
        ])
        assert _persistent(c) == (0, 0)
        want, want_mem, _ = _fresh("crnn", seed=5)
        c.load_crnn(lc.crnn_set(seed=5))
        got = _crnn_forwards(c)
        assert got == want, _where(got, want)
        assert _mem(c) == want_mem


def test_refused_first_detector_load_leaves_no_detector():
    img = lc.page(32, 48, "u8")
    canvas = wc.tiled_canvas()
    with _context() as c:
        for _, tensor, what, b, damage in lc.CRAFT_DEFECTS[:1] + lc.CRAFT_DEFECTS[-1:]:
            with pytest.raises(Exception, match=f"{EINVAL}: kocr_load_craft: .*{what}") as e:
                c.load_craft(damage(lc.craft_set(**b)))
            assert tensor in str(e.value)
        assert _persistent(c) == (0, 0)
        c.load_crnn(lc.crnn_set(seed=4321))  # the pipeline's refusal is then the detector's
        held = _persistent(c)
        _refused_without_a_launch(c, [
            ("craft_forward", lambda: c.craft_forward(img)),
            ("detect", lambda: c.detect(img)),
            ("craft_mse", lambda: c.craft_mse(img, np.zeros((1, 16, 24, 2), np.float32))),
            ("craft_forward_tiled", lambda: c.craft_forward_tiled(canvas, 64, 16)),
            ("detect_tiled", lambda: c._detect_tiled(canvas, 64, 16, 0.7, 0.4, 0.4, 10, 0, None)),
            ("pipeline", lambda: c.pipeline(*_pipeline_args())),
            ("pipeline_tiled", lambda: c.pipeline_tiled(*wc.tiled_args())),
        ])
        assert _persistent(c) == held
    with _context() as c:
        with pytest.raises(Exception, match=EINVAL):
            c.load_craft(lc.CRAFT_DEFECTS[1][4](lc.craft_set(seed=7)))
        want, want_mem, _ = _fresh("craft", seed=1234)
        _timed_load(c, "craft", lc.craft_set(seed=1234))
        got = _craft_forwards(c)
        assert got == want, _where(got, want)
        assert _mem(c) == want_mem


def test_refused_recognizer_keeps_the_shared_contexts_label_width():
    """Recognizer.__init__ sets rnn_steps_to_discard only once its weights are loaded"""
    import keras_ocr_amd

    with _context() as shared:
        serving = keras_ocr_amd.recognition.Recognizer(weights=lc.crnn_set(seed=4321), ctx=shared)
        assert shared.crnn_label_width() == 48
        before = _bits(shared.crnn_forward(lc.crops(3)))
        defective = lc.CRNN_DEFECTS[0][4](lc.crnn_set(seed=5))
        with pytest.raises(Exception, match="missing tensor conv_1/kernel"):
            keras_ocr_amd.recognition.Recognizer(weights=defective, build_params={"rnn_steps_to_discard": 0}, ctx=shared)
        assert shared.crnn_label_width() == 48
        assert _bits(shared.crnn_forward(lc.crops(3))) == before
        del serving


# ---- (d) ------------------------------------------------------------------------------------------------------------------------
def test_tables_give_back_what_they_take():
    with _context() as c:
        c.load_crnn(lc.crnn_set(seed=4321))
        c.crnn_forward(lc.crops(3))
        base = _persistent(c)
        steps = {
            "lexicon": [lambda: c.set_lexicon(*lc.lexicon(37, 50)), lambda: c.set_lexicon(*lc.lexicon(37, 200)),
                        lambda: c.set_lexicon(*lc.lexicon(37, 7)), lambda: c.set_lexicon(None)],
            "charsets": [lambda: c.set_charsets(lc.charsets(37, 3)), lambda: c.set_charsets(lc.charsets(37, 9)),
                         lambda: c.set_charsets(lc.charsets(37, 1)), lambda: c.set_charsets(None)],
            "patterns": [lambda: c.set_patterns(*lc.patterns(37, ("plate", "digits"))),
                         lambda: c.set_patterns(*lc.patterns(37, ("plate", "digits", "shape", "any", "code"))),
                         lambda: c.set_patterns(*lc.patterns(37, ("digits",))), lambda: c.set_patterns(None)],
        }
        for table, (load, larger, smaller, unload) in steps.items():
            load()
            one = _persistent(c)
            assert one[0] > base[0] and one[1] > base[1], table
            larger()
            two = _persistent(c)
            assert two[0] == one[0] and two[1] > one[1], f"{table}: the larger table: {two} after {one}"
            smaller()
            three = _persistent(c)
            assert three[0] == one[0] and three[1] < one[1], f"{table}: the smaller table: {three} after {one}"
            c.crnn_forward(lc.crops(3))
            unload()
            assert _persistent(c) == base, f"{table}: unloaded, the context holds {_persistent(c)}, before the first load {base}"


def test_refused_table_leaves_the_previous_one_answering():
    with _context() as c:
        c.load_crnn(lc.crnn_set(seed=4321))
        _load_tables(c)
        before, mem = _table_answers(c), c.debug_memory()
        labels, lengths = lc.lexicon(37, 50)
        bad = labels.copy()
        bad[3, 0] = 37  # a label >= classes
        with pytest.raises(ValueError, match="word 3: label 37"):
            c.set_lexicon(bad, lengths)
        sets = lc.charsets(37, 3).copy()
        sets[2] = 0  # an empty set
        with pytest.raises(ValueError, match="set 2 is empty"):
            c.set_charsets(sets)
        with pytest.raises(ValueError, match="more than KOCR_PATTERN_MAX_NODES"):
            c.set_patterns(*lc.too_many_nodes(37))
        assert c.debug_memory() == mem
        assert (c.lexicon_size(), c.charset_count(), c.pattern_count()) == (50, 3, 2)
        assert _table_answers(c) == before


def test_another_class_count_unloads_the_tables():
    want, want_mem, _ = _fresh("crnn", seed=5, classes=96)
    with _context() as c:
        c.load_crnn(lc.crnn_set(seed=4321))
        _load_tables(c)
        _table_answers(c)
        c.load_crnn(lc.crnn_set(seed=5, classes=96))
        assert (c.lexicon_size(), c.charset_count(), c.pattern_count()) == (0, 0, 0)
        assert (c.get_charset(), c.get_pattern(), c.get_lexicon_match()) == (-1, -1, 0)
        got = _crnn_forwards(c)
        assert got == want, _where(got, want)
        assert _mem(c) == want_mem, f"after the class change the context holds {_mem(c)}, a fresh one {want_mem}"
        # the same class count keeps them
        _load_tables(c, 96)
        c.load_crnn(lc.crnn_set(seed=4321, classes=96))
        assert (c.lexicon_size(), c.charset_count(), c.pattern_count()) == (50, 3, 2)


# ---- (e) ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def contexts():
    pool = _Contexts()
    yield pool
    pool.close()


def _allowed_first_call_growth():
    """the (allocations, bytes) a first call may add: any subset of the lazily allocated buffers that a call allocates"""
    sums = {(0, 0)}
    for name in lc.FIRST_CALL_ADDS:
        sums |= {(n + 1, b + lc.LAZY_BUFFERS[name][0]) for n, b in sums}
    return sums


@pytest.mark.parametrize("name", wc.names())
def test_calls_own_nothing_new(contexts, name):
    r = wc.row(name)
    c = _prepare(contexts.get(r["env"]), r)
    before = _persistent(c)
    seen = []
    for _ in range(3):
        _call(c, r)
        seen.append(_persistent(c))
    grown = (seen[0][0] - before[0], seen[0][1] - before[1])
    assert grown in _allowed_first_call_growth(), f"{name}: the first call added {grown}: not a sum of {lc.FIRST_CALL_ADDS}"
    assert seen[1] == seen[0] and seen[2] == seen[0], f"{name}: persistent (count, bytes) after three calls: {seen}"


@pytest.mark.parametrize("shape", [((2, 5, 7, 32), (3, 3, 32, 96)), ((1, 16, 16, 16), (3, 3, 16, 32))], ids=["cout96", "cout32"])
def test_conv2d_as_a_first_call_keeps_the_lazy_buffers_only(shape):
    """The temporary layer of kocr_conv2d_nhwc frees what the call added behind its mark: a lazily allocated buffer that is to
    outlive the call must be there before the mark (csrc/abi.h, TempLayer)."""
    rng = np.random.default_rng(31)
    x, w = rng.normal(0, 1, shape[0]).astype(np.float32), rng.normal(0, 0.1, shape[1]).astype(np.float32)
    lazy = [lc.LAZY_BUFFERS["range_block"][0], lc.LAZY_BUFFERS["amax_pool"][0]]
    with _context() as c:
        assert _persistent(c) == (0, 0)
        c.range_stats_enable(True)
        assert _persistent(c) == (1, lazy[0])
        c.profile_enable(True)
        first = _bits(c.conv2d_nhwc(x, w))
        assert _persistent(c) == (2, sum(lazy)), f"the first call left {_persistent(c)}, the lazy buffers are {lazy}"
        again = _bits(c.conv2d_nhwc(x, w))
        assert _persistent(c) == (2, sum(lazy))
        assert again == first
        for mode in lc.MODES[1:]:
            c.set_split_mode(mode)
            c.conv2d_nhwc(x, w)
            assert _persistent(c) == (2, sum(lazy)), mode


# ---- (f) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", range(5))
def test_contexts_give_everything_back(pair):
    """ten contexts in all, two per case (a detector load folds its linear chain on the host: a second and more of each case)"""
    import keras_ocr_amd
    from keras_ocr_amd import _lib

    before = _lib.debug_process_memory()
    craft, crnn = lc.craft_set(seed=1234, calibrated=True), lc.crnn_set(seed=4321)
    for k in range(2):
        c = keras_ocr_amd.Context(0)
        try:
            c.load_craft(craft)
            c.load_crnn(crnn)
            c.pipeline(*_pipeline_args())
            held = c.debug_memory()
            assert held["persistent_count"] > 200 and held["arena_bytes"] > 0
            assert held["process_count"] >= before["process_count"] + held["persistent_count"]
            assert held["process_bytes"] >= before["process_bytes"] + held["persistent_bytes"] + held["arena_bytes"]
        finally:
            c.close()
        now = _lib.debug_process_memory()
        assert now == before, f"after close {2 * pair + k + 1}: the process holds {now}, before the first create {before}"


def test_device_alloc_and_free_are_counted():
    from keras_ocr_amd import _lib

    before = _lib.debug_process_memory()
    with _context() as c:
        base = c.debug_memory()
        a, b = ctypes.c_void_p(), ctypes.c_void_p()
        assert c._lib.kocr_device_alloc(c._h, ctypes.byref(a), 1 << 20) == 0 and c._lib.kocr_device_alloc(c._h, ctypes.byref(b), 0) == 0
        now = c.debug_memory()
        assert (now["process_count"], now["process_bytes"]) == (base["process_count"] + 2, base["process_bytes"] + (1 << 20) + 4)
        assert _persistent(c) == (0, 0)  # the caller's buffers are the caller's
        assert c._lib.kocr_device_free(c._h, a) == 0 and c._lib.kocr_device_free(c._h, b) == 0
        assert c.debug_memory() == base
    assert _lib.debug_process_memory() == before
