"""The case table of tests/test_workspace_gpu.py: one row per call of an entry point that takes memory from the context's bump
arenas ("Arena book-keeping"), at the smallest shapes that take each allocation path.  Pure numpy,
seeded; nothing here touches a GPU.  tests/test_workspace_cases_cpu.py holds the table against include/kocr.h: every
``kocr_`` function is either the ``entry`` of a row or named in NO_ARENA.

A row:
  name      the test id
  entry     the extern "C" function the call is about (it reaches arena_reserve, Staging::reserve or ws_reserve)
  family    which LARGEST row re-sizes the arenas in the warm-equals-cold step
  env       the context's kernel switches (read from the environment when a context is created; tests/test_fallback_paths_gpu.py)
  crnn      None, or (classes, rnn_steps_to_discard, stn): the recogniser that must be loaded (a row's networks are also what its
            family's LARGEST call needs)
  craft     None, "raw" (synthetic weights), "page" (calibrated on PAGE as __graft_entry__.smoke does) or "A" (fixture A of
            tests/tiling_statement.py)
  setup     [(Context method, args)] run in order after every switch is back at its default; an argument may be a
            zero-argument callable, evaluated once
  method    the Context method; ``args`` / ``kwargs`` its arguments (callables as above)
  raises    None, or (exception, pattern): the row is a documented refusal
  touches   arenas that the call must have reserved (the edge the row is there for)
"""
import functools

import numpy as np

from tests import batch_edge_cases as bc
from tests import synth

F32 = np.float32
ARENAS = ("ws", "pp", "pp2", "io", "pl", "bx", "chw", "chr")

# Every kocr_ function that never reaches an arena: the context, memory copies, loaders (persistent allocations), switches and
# their getters, the resident-result getters (copies out of what a row's call left), taps, profiler, statistics, and the
# debug calls of the book-keeping itself.
NO_ARENA = """
kocr_create kocr_destroy kocr_last_error kocr_set_stream kocr_synchronize kocr_device_alloc kocr_device_free kocr_memcpy_h2d
kocr_memcpy_d2h kocr_load_craft kocr_load_crnn kocr_craft_set_taps kocr_craft_tap_count kocr_craft_tap_info kocr_craft_get_tap
kocr_crnn_set_taps kocr_crnn_classes kocr_crnn_set_rnn_steps_to_discard kocr_crnn_label_width kocr_set_char_boxes
kocr_get_char_boxes kocr_detection_char_boxes kocr_pipeline_results kocr_pipeline_device_results kocr_tile_plan
kocr_set_split_mode kocr_get_split_mode kocr_set_schedule kocr_get_schedule kocr_set_min_area_rect kocr_get_min_area_rect
kocr_set_scores kocr_get_scores kocr_detection_scores kocr_recognition_scores kocr_set_beam kocr_get_beam kocr_recognition_beams
kocr_set_lexicon kocr_lexicon_size kocr_set_lexicon_match kocr_get_lexicon_match kocr_recognition_lexicon kocr_set_lexicon_scratch
kocr_set_charsets kocr_charset_count kocr_set_charset kocr_get_charset kocr_set_patterns kocr_pattern_count kocr_set_pattern
kocr_get_pattern kocr_recognition_patterns kocr_set_orientation kocr_get_orientation kocr_recognition_orientation
kocr_profile_enable kocr_profile_reset kocr_profile_report kocr_range_stats_enable kocr_range_stats_report
kocr_debug_arena_count kocr_debug_arena_name kocr_debug_arena_stats kocr_debug_release_arenas kocr_debug_set_arena_guards
kocr_debug_check_arena_guards kocr_debug_set_arena_poison kocr_debug_memory_stats kocr_pipeline_results_shape
""".split()

DEFAULT_CRNN = (37, 2, True)
CELLS = {}                        # the cell-grid schedule (the default)
DENSE_52 = {"KOCR_CELLS": "0"}    # the dense schedule, conv_6 / conv_7 through the 52-wide padded layout
DENSE_50 = {"KOCR_W43": "0"}      # the dense schedule without F(4,3) kernels: 50-wide tensors
CRNN_M = (1, 8, 9, 17)            # 8 | 9: the two sides of cells_per_row; 17: a second row of cells with a ragged end
BEAM = (64, 64)                   # the launcher's limits
TOP_WORDS = 3
LDS_BYTES = 65536                 # the budget of the pattern and lexicon launches (crnn_kernels.hip)


# ---- inputs (built once, read-only) ----------------------------------------------------------------------------------------
def crops(m):
    return lambda: bc.crops(m)


@functools.lru_cache(maxsize=None)
def lexicon(classes):
    return bc.lexicon(classes)


def one_crop_scratch(classes):
    """kocr_set_lexicon_scratch such that a chunk of the lexicon launches is one crop: room for one row of V values"""
    return 4 * len(lexicon(classes)[0]) + 8


@functools.lru_cache(maxsize=None)
def patterns(classes):
    """keras_ocr_amd.patterns.Patterns: tests/pattern_cases.py's at 37 and 96 classes, ``.*`` over 999 characters at 1000"""
    from keras_ocr_amd import patterns as kp
    from tests import pattern_cases as pc

    if classes in pc.ALPHABETS:
        return pc.compiled(classes)
    return kp.Patterns("".join(chr(0x4E00 + i) for i in range(classes - 1)), {"any": r".*"})


def pattern_tables(classes):
    return lambda: patterns(classes).tables()


def pattern_index(classes, name):
    return lambda: patterns(classes).names.index(name)


def pattern_per_crop(classes, m):
    """crop k under pattern k % (P + 1) - 1: every pattern and -1 in turn"""
    return lambda: (np.arange(m) % (len(patterns(classes)) + 1) - 1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def charsets(classes):
    """three sets over the non-blank classes: the first ten, every other one, all"""
    allowed = np.zeros((3, classes - 1), np.uint8)
    allowed[0, :10] = 1
    allowed[1, ::2] = 1
    allowed[2, :] = 1
    return allowed


@functools.lru_cache(maxsize=None)
def logits(m, classes, seed=3):
    x = np.random.default_rng(seed).normal(0, 3, (m, 50, classes)).astype(F32)
    x.flags.writeable = False
    return x


def ctc_args(m, lw=48, classes=37):
    return lambda: bc.ctc_inputs(m, lw, classes)


@functools.lru_cache(maxsize=None)
def page():
    """the 64 x 96 synthetic page of __graft_entry__.smoke and tests/test_lines_gpu.py::test_layout_and_pipeline"""
    rng = np.random.default_rng(0)
    img = np.full((64, 96, 3), 255, np.uint8)
    for _ in range(4):
        x, y = int(rng.integers(0, 60)), int(rng.integers(0, 50))
        img[y:y + 10, x:x + 30] = rng.integers(0, 120, (10, 30, 3), dtype=np.uint8)
    img.flags.writeable = False
    return img


def pipeline_args():
    """two copies of PAGE resized 2x into a 128 x 192 batch"""
    return [page(), page()], [64, 64], [96, 96], [128, 128], [192, 192], 128, 192


@functools.lru_cache(maxsize=None)
def page_detector_input():
    from oracle import tools as otools

    return np.ascontiguousarray(otools.resize_image(page(), 2, 2048)[0][None])


def tiled_args():
    """fixture A of tests/tiling_statement.py: (80, 120) page, scale 2, tile 64, overlap 16 -> 28 tiles"""
    from tests import tiling_statement as ts

    (h, w, words, seed), scale, tile, overlap = ts.FIXTURES["A"]
    img = synth.text_page(h, w, words, seed=seed)
    return [img], [h], [w], [h * scale], [w * scale], tile, overlap


def tiled_canvas():
    from tests import tiling_statement as ts

    (h, w, words, seed), scale, tile, overlap = ts.FIXTURES["A"]
    resized = ts.resize(synth.text_page(h, w, words, seed=seed), scale)
    p = ts.plan(resized.shape[0], resized.shape[1], tile, overlap)
    return np.ascontiguousarray(ts.canvas_of(resized, p)[None])


def tiled_tile_heat():
    from tests import tiling_statement as ts

    (h, w, _, _), scale, tile, overlap = ts.FIXTURES["A"]
    p = ts.plan(h * scale, w * scale, tile, overlap)
    n = p.counts[0] * p.counts[1]
    return np.random.default_rng(12).random((n, tile // 2, tile // 2, 2)).astype(F32)


def detector_images(n, h, w, dtype=np.uint8):
    def build():
        x = np.random.default_rng(100 * h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        return x if dtype == np.uint8 else (x.astype(F32) / F32(255) - F32(0.5))
    return build


BOX_PAGE_H, BOX_PAGE_W = 64, 256


@functools.lru_cache(maxsize=None)
def box_pages():
    return np.stack([bc.page(BOX_PAGE_H, BOX_PAGE_W, 31), bc.page(BOX_PAGE_H, BOX_PAGE_W, 32)])


def box_groups(counts):
    return lambda: bc.boxes(tuple(counts), BOX_PAGE_H, BOX_PAGE_W)


def heat_case(name):
    def build():
        from tests import postproc_cases as pc
        return pc.case(name)["heat"]
    return build


def empty_heat():
    return np.zeros((1, 24, 40, 2), F32)


def heat_batch():
    return synth.heatmap_batch()


def chars_batch():
    from tests import chars_cases as cc
    heat, pages, _ = cc.batch()
    return heat, pages


def resize_case(name, f32=False):
    def build():
        from tests import geometry_cases as gc
        case = next(c for c in (gc.resize_cases_f32() if f32 else gc.resize_cases_u8()) if c[0] == name)
        _, _, _, dh, dw, hmax, wmax, _, cval = case
        src = gc.resize_source_f32(case, 3) if f32 else gc.resize_source_u8(case)
        return (src, (dw, dh)), {"out_hw": (hmax, wmax), "cval": cval}
    return build


def warp_case(f32=False):
    def build():
        from tests import geometry_cases as gc
        groups = next(g for n, g, failing in gc.group_layouts() if n == "3_0")
        return (gc.warp_images_f32(3) if f32 else gc.warp_images_u8()), groups
    return build


def quad_case():
    from tests import geometry_cases as gc
    name, src, dst, wh, img, _, _ = gc.quad_cases()[0]
    th, tw = gc.QUAD_TARGET
    return gc.warp_images_u8(), src[None], dst[None], [img], [wh], th, tw


def orient_rows(m=5, width=48):
    rng = np.random.default_rng(9)
    labels = rng.integers(-1, 36, (m, 2, width)).astype(np.int32)
    return labels, rng.normal(-5, 2, (m, 2)).astype(F32), rng.random((m, 2, width)).astype(F32)


def lines_pages():
    from tests import lines_cases as lc
    return lc.flatten(lc.small_pages())


def eval_tables(score):
    def build():
        from tests import evaluation_cases as ec
        true, pred, kw = ec.scenario_bookkeeping()
        ids, t = ec.tables_input(true, pred, kw.get("translator"))

        def flat(groups):
            quads = np.array([q for g in groups for q in g], np.int32).reshape(-1, 4, 2)
            return quads, np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
        tq, toff = flat(t["truth_quads"])
        pq, poff = flat(t["pred_quads"])
        if not score:
            return tq, toff, pq, poff
        texts = []
        for groups in (t["truth_texts"], t["pred_texts"]):
            rows = [r for g in groups for r in g]
            texts += [np.array([c for r in rows for c in r], np.int32), np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)]
        return (tq, toff, pq, poff, np.array([v for g in t["truth_ignore"] for v in g], np.uint8), *texts)
    return build


def maps_args():
    from tests import maps_statement as ms

    def rect(x, y, w, h):
        return np.array([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], F32)
    line = [(rect(6 + 9 * k, 8 + k, 8, 11), ch) for k, ch in enumerate("ab cd")]
    return ms.get_gaussian_heatmap(37, 2.0), 40, 64, [[line], [], [line[:2], line[2:]]]


def mse_maps():
    rng = np.random.default_rng(21)
    return rng.random((3, 17, 23, 2)).astype(F32), rng.random((3, 17, 23, 2)).astype(F32)


def mse_detector():
    x = detector_images(2, 32, 48)()
    return x, np.random.default_rng(22).random((2, 16, 24, 2)).astype(F32)


def conv_args(cells):
    def build():
        rng = np.random.default_rng(31)
        if cells:  # a level of tests/test_cells_gpu.py: n_img images of cn cells of hc x pitch holding (hc - 1) x wv crops
            hc, pitch, wv, cn, n_img, cin, cout = cells
            x = np.zeros((n_img, hc, cn * pitch, cin), F32)
            for j in range(cn):  # row 0 and the columns behind wv stay the zero gutters
                x[:, 1:, j * pitch:j * pitch + wv] = np.maximum(rng.standard_normal((n_img, hc - 1, wv, cin)), 0)
            return x, (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (cin * 9))).astype(F32), pitch, wv
        return rng.normal(0, 1, (2, 5, 7, 32)).astype(F32), rng.normal(0, 0.1, (3, 3, 32, 96)).astype(F32)
    return build


def ctc_cost_args():
    rng = np.random.default_rng(41)
    y = rng.random((5, 12, 9)).astype(F32) + F32(0.01)
    y /= y.sum(-1, keepdims=True)
    return y, rng.integers(0, 8, (5, 4)).astype(np.int32), np.array([4, 0, 1, 3, 2], np.int32), np.array([12, 1, 5, 9, 12], np.int32)


# ---- the table ---------------------------------------------------------------------------------------------------------
def _row(name, entry, family, method, args=(), kwargs=None, env=None, crnn=None, craft=None, setup=(), raises=None, touches=()):
    return dict(name=name, entry=entry, family=family, method=method, args=args, kwargs=kwargs or {}, env=dict(env or {}), crnn=crnn,
                craft=craft, setup=list(setup), raises=raises, touches=tuple(touches))


def _lexicon_setup(classes=37, scratch=None):
    out = [("set_lexicon", lambda: lexicon(classes))]
    if scratch:
        out.append(("set_lexicon_scratch", (scratch,)))
    return out


def _recogniser_rows():
    rows = []
    rec = functools.partial(_row, family="recogniser", crnn=DEFAULT_CRNN, touches=("ws",))
    for m in CRNN_M:
        rows += [
            rec(f"crnn_forward-M{m}", "kocr_crnn_forward", method="crnn_forward", args=(crops(m),)),
            rec(f"crnn_forward-probs-M{m}", "kocr_crnn_forward", method="crnn_forward", args=(crops(m),), kwargs={"return_probs": True}),
            rec(f"crnn_forward_scores-probs-M{m}", "kocr_crnn_forward_scores", method="crnn_forward_scores", args=(crops(m),),
                kwargs={"return_probs": True}),
            rec(f"crnn_beam-M{m}", "kocr_crnn_beam", method="crnn_beam", args=(crops(m),) + BEAM),
            rec(f"crnn_lexicon-M{m}", "kocr_crnn_lexicon", method="crnn_lexicon", args=(crops(m), TOP_WORDS), setup=_lexicon_setup()),
            rec(f"crnn_pattern-uniform-M{m}", "kocr_crnn_pattern", method="crnn_pattern", args=(crops(m),),
                setup=[("set_patterns", pattern_tables(37)), ("set_pattern", (pattern_index(37, "plate"),))]),
            rec(f"crnn_ctc_loss-M{m}", "kocr_crnn_ctc_loss", method="crnn_ctc_loss", args=(crops(m), ctc_args(m))),
            rec(f"crnn_features-M{m}", "kocr_crnn_features", method="crnn_features", args=(crops(m),)),
            # the two dense schedules
            rec(f"crnn_forward_scores-probs-dense52-M{m}", "kocr_crnn_forward_scores", method="crnn_forward_scores", args=(crops(m),),
                kwargs={"return_probs": True}, env=DENSE_52),
            rec(f"crnn_forward_scores-probs-dense50-M{m}", "kocr_crnn_forward_scores", method="crnn_forward_scores", args=(crops(m),),
                kwargs={"return_probs": True}, env=DENSE_50),
        ]
    # other builds of the recogniser
    for m in (1, 17):
        rows.append(rec(f"crnn_forward-probs-no_stn-M{m}", "kocr_crnn_forward", method="crnn_forward", args=(crops(m),),
                        kwargs={"return_probs": True}, crnn=(37, 2, False)))
    for discard in (0, 5):
        rows.append(rec(f"crnn_forward_scores-probs-discard{discard}-M9", "kocr_crnn_forward_scores", method="crnn_forward_scores",
                        args=(crops(9),), kwargs={"return_probs": True}, crnn=(37, discard, True)))
    for classes in (96, 1000):
        rows.append(rec(f"crnn_forward-probs-C{classes}-M9", "kocr_crnn_forward", method="crnn_forward", args=(crops(9),),
                        kwargs={"return_probs": True}, crnn=(classes, 2, True)))
    # lexicon: the scoring kernel's own values, chunks of one crop, the table that leaves LDS
    rows += [
        rec("crnn_lexicon-all_values-M9", "kocr_crnn_lexicon", method="crnn_lexicon", args=(crops(9), TOP_WORDS),
            kwargs={"return_values": True}, setup=_lexicon_setup()),
        rec("crnn_lexicon-one_crop_chunks-M9", "kocr_crnn_lexicon", method="crnn_lexicon", args=(crops(9), TOP_WORDS),
            setup=_lexicon_setup(scratch=one_crop_scratch(37))),
        rec("crnn_lexicon-one_crop_chunks-all_values-M17", "kocr_crnn_lexicon", method="crnn_lexicon", args=(crops(17), TOP_WORDS),
            kwargs={"return_values": True}, setup=_lexicon_setup(scratch=one_crop_scratch(37))),
        rec("crnn_lexicon-C1000-M9", "kocr_crnn_lexicon", method="crnn_lexicon", args=(crops(9), TOP_WORDS), crnn=(1000, 2, True),
            setup=_lexicon_setup(1000)),
    ]
    # patterns: one per crop, every crop -1, back-pointers that leave LDS, the -1 batch whose table leaves LDS
    rows += [
        rec("crnn_pattern-per_crop-M9", "kocr_crnn_pattern", method="crnn_pattern", args=(crops(9), pattern_per_crop(37, 9)),
            setup=[("set_patterns", pattern_tables(37))]),
        rec("crnn_pattern-per_crop-M17", "kocr_crnn_pattern", method="crnn_pattern", args=(crops(17), pattern_per_crop(37, 17)),
            setup=[("set_patterns", pattern_tables(37))]),
        rec("crnn_pattern-none-M9", "kocr_crnn_pattern", method="crnn_pattern", args=(crops(9), lambda: np.full(9, -1, np.int32)),
            setup=[("set_patterns", pattern_tables(37))]),
        rec("crnn_pattern-upto40-C96-M9", "kocr_crnn_pattern", method="crnn_pattern", args=(crops(9),), crnn=(96, 2, True),
            setup=[("set_patterns", pattern_tables(96)), ("set_pattern", (pattern_index(96, "upto40"),))]),
        rec("crnn_pattern-upto40-one_crop_chunks-C96-M9", "kocr_crnn_pattern", method="crnn_pattern", args=(crops(9),), crnn=(96, 2, True),
            setup=[("set_patterns", pattern_tables(96)), ("set_pattern", (pattern_index(96, "upto40"),)), ("set_lexicon_scratch", (1,))]),
        rec("crnn_pattern-none-C1000-M9", "kocr_crnn_pattern", method="crnn_pattern", args=(crops(9), lambda: np.full(9, -1, np.int32)),
            crnn=(1000, 2, True), setup=[("set_patterns", pattern_tables(1000))]),
    ]
    # the launches behind fc_12 on given logits
    for m in (1, 17):
        rows += [
            rec(f"decode_logits-M{m}", "kocr_crnn_decode_logits", method="crnn_decode_logits", args=(lambda m=m: logits(m, 37),),
                kwargs={"return_probs": True}),
            rec(f"decode_logits-everything-M{m}", "kocr_crnn_decode_logits", method="crnn_decode_logits", args=(lambda m=m: logits(m, 37),),
                kwargs={"return_probs": True, "scores": True, "beam": BEAM, "top_words": TOP_WORDS, "return_values": True,
                        "loss_labels": ctc_args(m)}, setup=_lexicon_setup()),
            rec(f"decode_logits-own_values-M{m}", "kocr_crnn_decode_logits", method="crnn_decode_logits", args=(lambda m=m: logits(m, 37),),
                kwargs={"top_words": TOP_WORDS}, setup=_lexicon_setup(scratch=one_crop_scratch(37))),
            rec(f"decode_logits_charsets-M{m}", "kocr_crnn_decode_logits_charsets", method="crnn_decode_logits",
                args=(lambda m=m: logits(m, 37),), kwargs={"scores": True, "beam": BEAM, "set_of": lambda m=m: np.arange(m) % 4 - 1},
                setup=[("set_charsets", (lambda: charsets(37),))]),
            rec(f"decode_logits_patterns-M{m}", "kocr_crnn_decode_logits_patterns", method="crnn_decode_logits_patterns",
                args=(lambda m=m: logits(m, 37), pattern_per_crop(37, m)), setup=[("set_patterns", pattern_tables(37))]),
        ]
    rows.append(rec("decode_logits_patterns-upto40-C96-M9", "kocr_crnn_decode_logits_patterns", method="crnn_decode_logits_patterns",
                    args=(lambda: logits(9, 96),), crnn=(96, 2, True),
                    setup=[("set_patterns", pattern_tables(96)), ("set_pattern", (pattern_index(96, "upto40"),))]))
    rows.append(rec("ctc_batch_cost", "kocr_ctc_batch_cost", method="ctc_batch_cost", args=(ctc_cost_args,), crnn=None))
    # across the batch edge: the workspace sized for 1024 crops, then reused by a tail of one
    rows.append(rec("crnn_forward_scores-probs-M1025", "kocr_crnn_forward_scores", method="crnn_forward_scores", args=(crops(1025),),
                    kwargs={"return_probs": True}))
    return rows


WIDEST_SETUP = [("set_lexicon", lambda: lexicon(37)), ("set_patterns", pattern_tables(37)), ("set_charsets", (lambda: charsets(37),))]


def _stage_rows():
    """kocr_recognize_boxes and its twins: the recogniser stage (RecStage, csrc/abi.h) with each extra alone and all together"""
    rec = functools.partial(_row, family="recogniser", crnn=DEFAULT_CRNN, method="recognize_boxes", touches=("ws", "io"))
    small = (box_pages, box_groups((5, 4)))
    rows = [
        rec("recognize_boxes", "kocr_recognize_boxes", args=small),
        rec("recognize_boxes-scores", "kocr_recognize_boxes", args=small, kwargs={"return_scores": True}),
        rec("recognize_boxes-beam", "kocr_recognize_boxes", args=small, kwargs={"beam": BEAM}),
        rec("recognize_boxes-lexicon", "kocr_recognize_boxes", args=small, kwargs={"lexicon_top": TOP_WORDS}, setup=_lexicon_setup()),
        rec("recognize_boxes-lexicon-one_crop_chunks", "kocr_recognize_boxes", args=small, kwargs={"lexicon_top": TOP_WORDS},
            setup=_lexicon_setup(scratch=one_crop_scratch(37))),
        rec("recognize_boxes-pattern", "kocr_recognize_boxes", args=small, kwargs={"pattern": pattern_index(37, "plate")},
            setup=[("set_patterns", pattern_tables(37))]),
        rec("recognize_boxes_patterns", "kocr_recognize_boxes_patterns", args=small, kwargs={"pattern_of": pattern_per_crop(37, 9)},
            setup=[("set_patterns", pattern_tables(37))]),
        rec("recognize_boxes_charsets", "kocr_recognize_boxes_charsets", args=small, kwargs={"set_of": lambda: np.arange(9) % 4 - 1},
            setup=[("set_charsets", (lambda: charsets(37),))]),
        rec("recognize_boxes-orientation", "kocr_recognize_boxes", args=small, kwargs={"orientation": ("any", 1.5)}),
        # the widest stage that the library accepts: scores + beam + lexicon + pattern, and scores + beam + lexicon + a character set
        rec("recognize_boxes-widest-pattern", "kocr_recognize_boxes", args=small,
            kwargs={"return_scores": True, "beam": BEAM, "lexicon_top": TOP_WORDS, "pattern": pattern_index(37, "plate")}, setup=WIDEST_SETUP),
        rec("recognize_boxes-widest-charset", "kocr_recognize_boxes", args=small,
            kwargs={"return_scores": True, "beam": BEAM, "lexicon_top": TOP_WORDS}, setup=WIDEST_SETUP + [("set_charset", (1,))]),
        # ... and all of them on: a pattern states its characters itself, so the library refuses it under an active character set
        rec("recognize_boxes-everything-refused", "kocr_recognize_boxes", args=small,
            kwargs={"return_scores": True, "beam": BEAM, "lexicon_top": TOP_WORDS, "pattern": pattern_index(37, "plate")},
            setup=WIDEST_SETUP + [("set_charset", (1,))], raises=(ValueError, "character set"), touches=()),
        rec("recognize_boxes-widest-M1025", "kocr_recognize_boxes", args=(box_pages, box_groups((600, 425))),
            kwargs={"return_scores": True, "beam": (4, 2), "lexicon_top": TOP_WORDS, "pattern": pattern_index(37, "plate")}, setup=WIDEST_SETUP),
    ]
    return rows


def _detector_rows():
    det = functools.partial(_row, family="detector", craft="raw", touches=("ws",))
    rows = [
        det("craft_forward-1x16x16", "kocr_craft_forward", method="craft_forward", args=(detector_images(1, 16, 16),)),
        det("craft_forward-3x16x16", "kocr_craft_forward", method="craft_forward", args=(detector_images(3, 16, 16),)),
        det("craft_forward-1x17x19", "kocr_craft_forward", method="craft_forward", args=(detector_images(1, 17, 19),)),
        det("craft_forward-3x17x19-micro2", "kocr_craft_forward", method="craft_forward", args=(detector_images(3, 17, 19),),
            kwargs={"micro_batch": 2}),
        det("craft_forward-1x64x96", "kocr_craft_forward", method="craft_forward", args=(detector_images(1, 64, 96),)),
        det("craft_forward-3x64x96-f32", "kocr_craft_forward", method="craft_forward", args=(detector_images(3, 64, 96, F32),)),
        det("craft_mse-2x32x48", "kocr_craft_mse", method="craft_mse", args=(mse_detector,)),
        det("craft_forward_tiled-A", "kocr_craft_forward_tiled", method="craft_forward_tiled", args=(tiled_canvas, 64, 16)),
        det("gather_tiles-A", "kocr_gather_tiles", method="gather_tiles", args=(tiled_canvas, 64, 16), touches=("io",)),
        det("stitch_heat-A", "kocr_stitch_heat", method="stitch_heat", args=(tiled_tile_heat, (160, 256), 64, 16), touches=("io",)),
    ]
    box = functools.partial(_row, entry="kocr_get_boxes", family="detector", method="get_boxes", craft="raw", touches=("pp",))
    rows += [
        box("get_boxes-no_components", args=(empty_heat,)),
        box("get_boxes-one_component", args=(heat_case("all_foreground_2x2"),), kwargs={"size_threshold": 1}, touches=("pp", "pp2")),
        box("get_boxes-crowded", args=(heat_case("square_grid"),), touches=("pp", "pp2")),
        box("get_boxes-crowded-cap1", args=(heat_case("square_grid"),), kwargs={"cap": 1}, touches=("pp", "pp2")),
        box("get_boxes-batch-opencv", args=(heat_batch,), kwargs={"min_area_rect": "opencv"}, touches=("pp", "pp2")),
        box("get_boxes-batch-exact-scores", args=(heat_batch,), kwargs={"min_area_rect": "exact", "return_scores": True}, touches=("pp", "pp2")),
        box("get_boxes-batch-char_boxes", args=(heat_batch,), kwargs={"char_boxes": True}, touches=("pp", "pp2", "chw", "chr")),
        box("get_boxes-batch-opencv-scores-char_boxes-cap1", args=(heat_batch,),
            kwargs={"min_area_rect": "opencv", "return_scores": True, "char_boxes": True, "cap": 1}, touches=("pp", "pp2", "chw", "chr")),
    ]
    return rows


def _pipeline_rows():
    pipe = functools.partial(_row, family="pipeline", crnn=DEFAULT_CRNN, craft="page", touches=("ws", "io", "pl", "pp", "pp2"))
    tiled = functools.partial(pipe, craft="A")
    return [
        pipe("pipeline", "kocr_pipeline", method="pipeline", args=(pipeline_args,)),
        pipe("pipeline-orientation", "kocr_pipeline", method="pipeline", args=(pipeline_args,), kwargs={"orientation": ("any", 1.5)}),
        pipe("pipeline-cap1", "kocr_pipeline", method="pipeline", args=(pipeline_args,), kwargs={"cap": 1},
             touches=("ws", "io", "pl", "pp", "pp2", "bx")),
        pipe("pipeline-widest", "kocr_pipeline", method="pipeline", args=(pipeline_args,),
             kwargs={"return_scores": True, "lexicon_top": TOP_WORDS, "pattern": pattern_index(37, "plate"), "char_boxes": True,
                     "min_area_rect": "opencv"}, setup=WIDEST_SETUP + [("set_beam", BEAM)],
             touches=("ws", "io", "pl", "pp", "pp2", "chw", "chr")),
        pipe("detect", "kocr_detect", method="detect", args=(page_detector_input,), touches=("ws", "pl", "pp", "pp2")),
        pipe("detect-scores-char_boxes", "kocr_detect", method="detect", args=(page_detector_input,),
             kwargs={"return_scores": True, "char_boxes": True}, touches=("ws", "pl", "pp", "pp2", "chw", "chr")),
        tiled("detect_tiled-A", "kocr_detect_tiled", method="_detect_tiled", args=(tiled_canvas, 64, 16, 0.7, 0.4, 0.4, 10, 0, None),
              touches=("ws", "pl", "pp", "pp2")),
        tiled("pipeline_tiled-A", "kocr_pipeline_tiled", method="pipeline_tiled", args=(tiled_args,)),
        tiled("pipeline_tiled-A-orientation", "kocr_pipeline_tiled", method="pipeline_tiled", args=(tiled_args,),
              kwargs={"orientation": ("any", 1.5)}),
    ]


def _other_rows():
    other = functools.partial(_row, family="other", touches=("io",))
    return [
        other("resize_pad-batch3", "kocr_resize_pad", method="resize_pad", args=(resize_case("batch3_cval7"),)),
        other("resize_pad-to_1x1", "kocr_resize_pad", method="resize_pad", args=(resize_case("to_1x1"),)),
        other("resize_pad_f32-batch3", "kocr_resize_pad_f32", method="resize_pad_f32", args=(resize_case("batch3_cval-1.5", True),)),
        other("resize_pad_f32-to_1x1", "kocr_resize_pad_f32", method="resize_pad_f32", args=(resize_case("to_1x1", True),)),
        other("warp_crops", "kocr_warp_crops", method="warp_crops", args=(warp_case(),)),
        other("warp_crops_f32", "kocr_warp_crops_f32", method="warp_crops_f32", args=(warp_case(True),)),
        other("warp_quads", "kocr_warp_quads", method="warp_quads", args=(quad_case,), kwargs={"return_transforms": True}),
        other("warp_crops_turned", "kocr_warp_crops_turned", method="warp_crops_turned", args=(warp_case(),)),
        other("orient_select", "kocr_orient_select", method="orient_select", args=(orient_rows,)),
        other("group_lines", "kocr_group_lines", method="group_lines", args=(lines_pages,)),
        other("group_lines-no_boxes", "kocr_group_lines", method="group_lines", args=(lines_pages,), kwargs={"return_boxes": False}),
        other("char_boxes", "kocr_char_boxes", method="char_boxes", args=(chars_batch,), touches=("io", "chw", "chr")),
        other("iou_table", "kocr_iou_table", method="iou_table", args=(eval_tables(False),)),
        other("score_tables", "kocr_score", method="score_tables", args=(eval_tables(True),), kwargs={"return_iou": True}),
        other("compute_maps", "kocr_compute_maps", method="compute_maps", args=(maps_args,)),
        other("heat_mse", "kocr_heat_mse", method="heat_mse", args=(mse_maps,)),
        other("conv2d_nhwc", "kocr_conv2d_nhwc", method="conv2d_nhwc", args=(conv_args(None),), touches=("ws",)),
        # the conv_6 class (ragged couts; 52-column cells are not pooled) and the conv_4 class with the fused pooling
        other("conv2d_cells", "kocr_conv2d_cells", method="conv2d_cells", args=(conv_args((8, 52, 50, 16, 2, 64, 130)),), touches=("ws",)),
        other("conv2d_cells-pool", "kocr_conv2d_cells", method="conv2d_cells", args=(conv_args((16, 104, 100, 8, 1, 128, 256)),),
              kwargs={"pool": True, "need_full": False}, touches=("ws",)),
    ]


@functools.lru_cache(maxsize=None)
def rows():
    out = _recogniser_rows() + _stage_rows() + _detector_rows() + _pipeline_rows() + _other_rows()
    assert len({r["name"] for r in out}) == len(out)
    return tuple(out)


def names():
    return [r["name"] for r in rows()]


def row(name):
    return next(r for r in rows() if r["name"] == name)


# the row that sizes a family's arenas for its largest shapes in the warm-equals-cold step (None: the step repeats the call alone)
LARGEST = {"recogniser": "crnn_forward_scores-probs-M1025", "pipeline": "pipeline_tiled-A", "detector": "craft_forward_tiled-A",
           "other": None}


@functools.lru_cache(maxsize=None)
def _value(thing):
    return thing()


def resolve(thing):
    """a table entry as the call takes it: zero-argument callables evaluated (once), containers walked"""
    if callable(thing):
        return resolve(_value(thing))
    if isinstance(thing, tuple):
        return tuple(resolve(v) for v in thing)
    if isinstance(thing, dict):
        return {k: resolve(v) for k, v in thing.items()}
    return thing


def call_of(r):
    """(args, kwargs) of the row's call.  A builder that returns ``(args tuple, kwargs dict)`` (resize_case) or a tuple of
    arguments (the *_args builders) is spliced in when it is the row's only argument."""
    args, kwargs = resolve(tuple(r["args"])), resolve(dict(r["kwargs"]))
    if len(args) == 1 and isinstance(args[0], tuple):
        inner = args[0]
        if len(inner) == 2 and isinstance(inner[1], dict) and isinstance(inner[0], tuple):
            return inner[0], dict(inner[1], **kwargs)
        return inner, kwargs
    flat = []
    for a in args:  # crnn_ctc_loss(crops, *ctc_inputs): a tuple argument among others is spliced in as well
        flat += list(a) if isinstance(a, tuple) and all(isinstance(v, np.ndarray) for v in a) and r["method"] == "crnn_ctc_loss" else [a]
    return tuple(flat), kwargs


def setup_of(r):
    """[(method, args tuple)] with the arguments resolved; a bare callable stands for the whole argument tuple"""
    out = []
    for method, args in r["setup"]:
        a = resolve(args)
        out.append((method, a if isinstance(a, tuple) else (a,)))
    return out
