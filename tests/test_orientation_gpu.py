"""Word orientation on the GPU ("Orientation") against its statement tests/orientation_statement.py.

Every comparison is bit for bit: each side is either integer / float64 arithmetic with contraction off (the crop stage and
the oracle's restatement of it), or the same kernels on the same bits (the recogniser's two runs), or a copy (the choice).
  1. crop stage    Context.warp_crops_turned == the statement's crops, turns and quads on chosen boxes;
  2. choice        Context.orient_select == the statement's select on chosen rows (ties, empties, NaN, -inf);
  3. recogniser    Context.recognize_boxes(orientation=) == the composition of calls that exist without it: the statement's
                   quads through Context.warp_quads, crnn_forward_scores on each candidate set, the statement's select;
  4. pipeline      Context.pipeline(orientation=) == the off run's boxes and path 3 on the padded batch with those boxes, also
                   over a capacity overflow, with a page without boxes and from device pointers; off again == before;
  5. public        Pipeline / Recognizer return the winners; the refusals.
The weights are the synthetic ones with fc_12 doubled (as tests/test_beam_gpu.py sharpens them): nothing here shows that the
RIGHT reading wins, only that the stated rule is computed exactly."""
import numpy as np
import pytest

from tests import orientation_statement as st
from tests import synth

pytestmark = pytest.mark.gpu

SHARPEN = 2.0
ANY = ("any", 1.5)


def _rect(x0, y0, w, h):
    return np.array([[x0, y0], [x0 + w, y0], [x0 + w, y0 + h], [x0, y0 + h]], np.float32)


def _rotated(cx, cy, w, h, degrees):
    a = np.radians(degrees)
    r = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    return (np.array([[-w / 2, -h / 2], [w / 2, -h / 2], [w / 2, h / 2], [-w / 2, h / 2]]) @ r.T + [cx, cy]).astype(np.float32)


# wide, tall, exactly at the ratio (20 x 30), rotated 30 degrees (a wide one, and a tall one, which get_rotated_box orders as a
# wide box on a steep slope: its two leftmost corners span a long side), a tall one tilted by 10 degrees (still tall), partly
# outside the image (two ways), one pixel high, one pixel wide, and a (2, 172)-sized sliver as the detector gives for a page edge
BOXES = np.stack([_rect(10, 20, 60, 20), _rect(30, 5, 12, 80), _rect(70, 40, 20, 30), _rotated(64, 48, 60, 20, 30),
                  _rotated(64, 48, 16, 70, 30), _rotated(64, 48, 16, 70, 10), _rect(100, 70, 60, 40), _rect(-10, -5, 40, 20),
                  _rect(5, 50, 40, 1), _rect(50, 5, 1, 40), _rect(60, -40, 2, 172)])
TALL = [False, True, True, False, False, True, False, False, False, True, True]  # by hand: h >= 1.5 w of the ordered box


@pytest.fixture(scope="module")
def page():
    return synth.text_page(96, 128, 5, seed=21)


def _sharpened(weights):
    w = dict(weights)
    w["fc_12/kernel"] = w["fc_12/kernel"] * np.float32(SHARPEN)
    w["fc_12/bias"] = w["fc_12/bias"] * np.float32(SHARPEN)
    return w


@pytest.fixture(scope="module")
def crnn_ctx(ctx, crnn_weights):
    ctx.crnn_set_rnn_steps_to_discard(2)
    ctx.load_crnn(_sharpened(crnn_weights))
    yield ctx
    ctx.set_orientation(0)
    ctx.set_scores(False)
    ctx.load_crnn(crnn_weights)


# ---- 1. crop stage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", st.MODES)
def test_crop_stage_equals_the_statement(ctx, page, mode):
    want_crops, want_turns, want_quads = st.crops(page, BOXES, mode)
    crops, turns, quads = ctx.warp_crops_turned(page[None], [BOXES], mode)
    assert turns.tolist() == want_turns.tolist()
    assert np.array_equal(quads, want_quads)
    assert np.array_equal(crops, want_crops)
    base = [int(t and mode == "any") for t in TALL]
    assert turns.reshape(-1, 2).tolist() == [[b, b + 2] for b in base]
    # a turn of 0 is the crop stage of today
    plain = ctx.warp_crops(page[None], [BOXES])
    for m, b in enumerate(base):
        if b == 0:
            assert np.array_equal(crops[2 * m], plain[m])
    assert sum(b == 0 for b in base) >= 5


def test_crop_stage_over_two_images_and_other_ratios(ctx, page):
    """boxes of the second image read the second image; the ratio moves the border"""
    other = np.ascontiguousarray(page[::-1])
    groups = [BOXES[:3], BOXES[3:]]
    crops, turns, quads = ctx.warp_crops_turned(np.stack([page, other]), groups, "any", 3.0)
    w0 = st.crops(page, groups[0], "any", 3.0)
    w1 = st.crops(other, groups[1], "any", 3.0)
    for got, a, b in zip((crops, turns, quads), w0, w1):
        assert np.array_equal(got, np.concatenate([a, b]))
    assert turns.reshape(-1, 2)[2].tolist() == [0, 2]  # 20 x 30 is not tall at ratio 3
    empty = ctx.warp_crops_turned(page[None], [np.zeros((0, 4, 2), np.float32)], "flip")
    assert [a.shape for a in empty] == [(0, 31, 200), (0,), (0, 4, 2)]


def test_zero_size_box_is_the_reference_error(ctx, page):
    with pytest.raises(ZeroDivisionError):
        ctx.warp_crops_turned(page[None], [np.stack([BOXES[0], _rect(5, 5, 0.5, 40)])], "any")
    with pytest.raises(ValueError, match="orientation"):
        ctx.warp_crops_turned(page[None], [BOXES[:1]], "sideways")


# ---- 2. the choice ---------------------------------------------------------------------------------------------------
def _rows(m, width, seed):
    rng = np.random.default_rng(seed)
    labels = np.full((m, 2, width), -1, np.int32)
    n = rng.integers(0, 4, (m, 2)) * rng.integers(0, width // 3 + 1, (m, 2))  # about a quarter of the rows are empty
    for i in range(m):
        for c in range(2):
            labels[i, c, :n[i, c]] = rng.integers(0, 37, n[i, c])
    special = np.array([-np.inf, np.nan, -1.5, -1.5, -0.25, 0.0], np.float32)
    log_word = np.where(rng.random((m, 2)) < 0.5, special[rng.integers(0, len(special), (m, 2))],
                        -rng.random((m, 2)).astype(np.float32) * 20).astype(np.float32)
    chars = rng.random((m, 2, width)).astype(np.float32)
    turns = np.stack([rng.integers(0, 2, m), np.zeros(m, np.int64)], 1).astype(np.int32)
    turns[:, 1] = turns[:, 0] + 2
    quads = rng.random((m, 2, 4, 2)).astype(np.float32) * 100
    return labels, log_word, chars, turns, quads


@pytest.mark.parametrize("m,width", [(1, 48), (63, 48), (64, 48), (65, 48), (1025, 48), (5, 70), (3, 1)])
def test_select_equals_the_statement(ctx, m, width):
    labels, log_word, chars, turns, quads = _rows(m, width, seed=m)
    if m >= 63:  # the cases by hand in front: one side empty (both ways), both empty, a tie, NaN (both sides), -inf (both ways)
        labels[:8] = -1
        labels[0, 1, :2] = labels[1, 0, :2] = 5
        labels[3:8, :, 0] = 7
        log_word[:8] = [(-0.1, -9), (-9, -0.1), (-3, -1), (-2, -2), (-2, np.nan), (np.nan, -2), (-np.inf, -50), (-np.inf, -np.inf)]
        assert st.select(labels[:8], log_word[:8]).tolist() == [1, 0, 1, 0, 0, 0, 1, 0]
    win = st.select(labels, log_word)
    if m >= 63:
        assert 0 < win.sum() < m
    pick = np.arange(m)
    got = ctx.orient_select(labels, log_word, chars, turns, quads)
    want = (labels[pick, win], log_word[pick, win], chars[pick, win], turns[pick, win], quads[pick, win], log_word)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.int32), w.view(np.int32))  # bits: NaN and -inf included
    # the defaults: turns (0, 2), so the winner is turn / 2
    assert (ctx.orient_select(labels, log_word, chars)[3] // 2).tolist() == win.tolist()


# ---- 3. the recogniser path ------------------------------------------------------------------------------------------
def _composition(c, images, box_groups, mode, tall_ratio):
    """What recognize_boxes(orientation=) must return, from calls that exist without it and the statement"""
    src, dst, idx, wh, turns = [], [], [], [], []
    for i, boxes in enumerate(box_groups):
        for box in boxes:
            t, q = st.candidates(box, mode, tall_ratio)
            for k in range(2):
                _, _, d, _, dsize = st.quad_params(q[k])
                src.append(q[k])
                dst.append(d)
                idx.append(i)
                wh.append(dsize)
                turns.append(int(t[k]))
    src, turns = np.array(src, np.float32), np.array(turns, np.int32)
    crops = c.warp_quads(images, src, np.array(dst, np.float32), idx, wh, 31, 200)
    read = [c.crnn_forward_scores(crops[k::2]) for k in range(2)]  # each candidate set on its own
    labels, log_word, chars = (np.stack([read[0][j], read[1][j]], 1) for j in range(3))
    win = st.select(labels, log_word)
    pick = np.arange(len(win))
    return labels[pick, win], log_word[pick, win], chars[pick, win], turns.reshape(-1, 2)[pick, win], src.reshape(-1, 2, 4, 2)[pick, win], \
        log_word, win


def _same(got, want):
    assert len(got) == 6
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert np.array_equal(g.view(np.int32), w.view(np.int32))


def _word_boxes(rng, n):
    """n boxes on a 96 x 128 page: wide, tall and tilted ones"""
    out = []
    for k in range(n):
        w, h = (int(rng.integers(30, 80)), int(rng.integers(10, 20))) if k % 3 else (int(rng.integers(10, 18)), int(rng.integers(30, 70)))
        x, y = int(rng.integers(0, 128 - w)), int(rng.integers(0, 96 - h))
        out.append(_rect(x, y, w, h) if k % 4 else _rotated(x + w / 2, y + h / 2, w, h, int(rng.integers(-40, 40))))
    return np.stack(out)


@pytest.mark.parametrize("m", [1, 7, 600])
def test_recognize_boxes_equals_the_composition(crnn_ctx, m):
    c = crnn_ctx
    rng = np.random.default_rng(5)
    pages = np.stack([synth.text_page(96, 128, 5, seed=21), synth.text_page(96, 128, 6, seed=24)])
    distinct = _word_boxes(rng, min(m, 24))
    boxes = np.concatenate([distinct] * (m // len(distinct)))  # 600 = 24 x 25: 2 M = 1200 crops, past one recogniser batch of 1024
    assert len(boxes) == m
    groups = [boxes[: m // 2], boxes[m // 2:]]
    for mode, ratio in (ANY, ("flip", 1.5)) if m == 7 else (ANY,):
        *want, win = _composition(c, pages, groups, mode, ratio)
        _same(c.recognize_boxes(pages, groups, return_scores=True, orientation=(mode, ratio)), want)
        if m == 600:
            assert 0 < win.sum() < m, "both outcomes of the choice must occur"
            assert {0, 1, 2, 3} == set(want[3].tolist())
    if m == 7:
        # without scores: the same winners; the box buffers are the caller's; the switch is restored
        labels, turns, quads, pairs = c.recognize_boxes(pages, groups, orientation=ANY)
        assert c.get_orientation() == (0, 1.5)
        with pytest.raises(ValueError, match="scores off"):
            c.recognition_scores()
        *want, _ = _composition(c, pages, groups, *ANY)
        _same((labels, want[1], want[2], turns, quads, pairs), want)
        # and off again: today's results, and nothing of the orientation resident
        off = c.recognize_boxes(pages, groups, return_scores=True)
        with pytest.raises(ValueError, match="orientation off"):
            c.recognition_orientation()
        plain = c.crnn_forward_scores(c.warp_crops(pages, groups))  # sizes the arenas: nothing is resident after it
        for g, w in zip(off, plain):
            assert np.array_equal(g, w)
        with pytest.raises(ValueError, match="no orientation is resident"):
            c.recognition_orientation()


def test_sizing_an_arena_forgets_the_orientation_with_the_scores(crnn_ctx, page):
    """The resident rows lie in the io arena: a call that sizes it may overwrite them, so every resident result is forgotten
    there, the orientation together with the scores"""
    c = crnn_ctx
    c.recognize_boxes(page[None], [BOXES[:3]], return_scores=True, orientation=ANY)
    turns, quads, pairs = c.recognition_orientation()
    assert turns.shape == (3,) and quads.shape == (3, 4, 2) and pairs.shape == (3, 2)
    assert c.recognition_scores()[0].shape == (3,)
    maps = np.zeros((1, 1, 1, 2), np.float32)
    assert c.heat_mse(maps, maps).tolist() == [0.0]  # unrelated, and sizes the io arena
    with pytest.raises(ValueError, match="no orientation is resident"):
        c.recognition_orientation()
    with pytest.raises(ValueError, match="no recognition scores are resident"):
        c.recognition_scores()


def test_recognizer_returns_the_winners(crnn_ctx, crnn_weights):
    import keras_ocr_amd
    from keras_ocr_amd import layout

    c = crnn_ctx
    rec = keras_ocr_amd.recognition.Recognizer(weights=_sharpened(crnn_weights), ctx=c)
    rng = np.random.default_rng(6)
    pages = [synth.text_page(96, 128, 5, seed=21), synth.text_page(96, 128, 6, seed=24)]
    groups = [_word_boxes(rng, 4), _word_boxes(rng, 3)]
    labels, log_word, chars, turns, quads, pairs, _ = _composition(c, np.stack(pages), groups, "any", 2.0)
    texts = rec._decode(labels)  # pylint: disable=protected-access
    assert rec.recognize_from_boxes(pages, groups, orientation="any", tall_ratio=2.0) == [texts[:4], texts[4:]]
    out = rec.recognize_from_boxes(pages, groups, orientation="any", tall_ratio=2.0, return_orientation=True, return_scores=True)
    flat = [w for group in out for w in group]
    assert [len(g) for g in out] == [4, 3] and [w[0] for w in flat] == texts
    for k, (_, score, how) in enumerate(flat):
        assert isinstance(how, layout.Orientation) and how.turns == turns[k] and np.array_equal(how.box, quads[k])
        assert how.log_words == (float(pairs[k, 0]), float(pairs[k, 1])) and score.log_word == float(log_word[k])
    # pages of two sizes: one call per image, the same words
    small = pages[1][:90, :120]
    inside = [b for b in groups[1] if b[:, 0].max() < 120 and b[:, 1].max() < 90 and b.min() >= 0]
    if inside:
        one = rec.recognize_from_boxes([pages[0], small], [groups[0], np.stack(inside)], orientation="any", tall_ratio=2.0,
                                       return_orientation=True)
        assert [w[0] for w in one[0]] == texts[:4] and len(one[1]) == len(inside)
    with pytest.raises(ValueError, match="orientation and beam_width"):
        rec.recognize_from_boxes(pages, groups, orientation="any", beam_width=4)


# ---- 4. the pipeline -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def calibrated(craft_weights):
    import keras_ocr_amd
    from oracle import craft as ocraft

    page = synth.text_page(96, 128, 5, seed=21)[None]
    from oracle import tools as otools
    big = np.stack([otools.resize_image(p, 2, 2048)[0] for p in page])
    heat = ocraft.detector_predict(craft_weights, big)
    return keras_ocr_amd.weights.calibrate_craft_head(craft_weights, heat, text_frac=0.10, link_frac=0.04)


@pytest.fixture(scope="module")
def pipe(crnn_ctx, calibrated, crnn_weights):
    import keras_ocr_amd

    det = keras_ocr_amd.detection.Detector(weights=calibrated, ctx=crnn_ctx)
    rec = keras_ocr_amd.recognition.Recognizer(weights=_sharpened(crnn_weights), ctx=crnn_ctx)
    return keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)


def _pages():
    return [synth.text_page(96, 128, 5, seed=21), np.ascontiguousarray(np.rot90(synth.text_page(128, 96, 5, seed=23))),
            np.ascontiguousarray(np.rot90(synth.text_page(96, 128, 5, seed=21)))]


def _run(pipe, c, pages, **kw):
    """Context.pipeline on host pages or device pointers as Pipeline calls it: boxes in detector-input pixels"""
    shapes = [p.shape for p in kw.pop("shapes", pages)]
    _, dhs, dws, hmax, wmax = pipe._plan(shapes)  # pylint: disable=protected-access
    return c.pipeline(pages, [s[0] for s in shapes], [s[1] for s in shapes], dhs, dws, hmax, wmax, **kw), (hmax, wmax)


def _padded(c, pages, hmax, wmax):
    from oracle import tools as otools

    return np.stack([otools.pad(c.resize_pad(p[None], (p.shape[1] * 2, p.shape[0] * 2))[0], width=wmax, height=hmax) for p in pages])


def _tall_and_not(box_groups, ratio=1.5):
    from oracle import tools as otools

    tall = [h >= ratio * w for boxes in box_groups for w, h in (otools.get_rotated_width_height(otools.get_rotated_box(b)[0]) for b in boxes)]
    return any(tall) and not all(tall)


def _check_against_path_3(c, out, batch, mode=ANY):
    boxes, labels, scores, how = out
    *want, _ = _composition(c, batch, boxes, *mode)
    _same((labels, scores[1], scores[2], *how), want)


def test_pipeline_equals_off_boxes_and_the_recogniser_path(pipe, crnn_ctx):
    c = crnn_ctx
    pages = _pages()
    c.profile_enable(True)
    c.profile_reset()
    (b0, l0, s0), (hmax, wmax) = _run(pipe, c, pages, return_scores=True)
    rows_before = {k: v["launches"] for k, v in c.profile_report().items()}
    assert _tall_and_not(b0), "the batch needs tall and non-tall boxes"
    print("boxes per page:", [len(b) for b in b0])
    batch = _padded(c, pages, hmax, wmax)
    c.profile_reset()
    on, _ = _run(pipe, c, pages, return_scores=True, orientation=ANY)
    rows_on = {k: v["launches"] for k, v in c.profile_report().items()}
    assert len(on) == 4 and all(np.array_equal(a, b) for a, b in zip(on[0], b0)), "the boxes are the off run's bits"
    assert all(np.array_equal(a, b) for a, b in zip(on[2][0], s0[0]))
    _check_against_path_3(c, on, batch)
    assert rows_on["warp_prepare_turned"] == 1 and rows_on["orient_select"] == 1 and "warp_prepare" not in rows_on
    assert len(set(on[3][0].tolist())) >= 2
    # mode flip on the same boxes
    flip, _ = _run(pipe, c, pages, return_scores=True, orientation=("flip", 1.5))
    _check_against_path_3(c, flip, batch, ("flip", 1.5))
    assert set(flip[3][0].tolist()) <= {0, 2}
    # capacity overflow, then fetch: the same results
    small, _ = _run(pipe, c, pages, return_scores=True, orientation=ANY, cap=2, max_crops=2)
    assert max(len(b) for b in b0) > 2
    for a, b in zip(small[0], on[0]):
        assert np.array_equal(a, b)
    _same((small[1], small[2][1], small[2][2], *small[3]), (on[1], on[2][1], on[2][2], *on[3]))
    # without scores the winners are the same
    bare, _ = _run(pipe, c, pages, orientation=ANY)
    assert len(bare) == 3 and np.array_equal(bare[1], on[1]) and all(np.array_equal(a, b) for a, b in zip(bare[2], on[3]))
    # off again: the run before, bit for bit, and exactly its launches
    c.profile_reset()
    (b1, l1, s1), _ = _run(pipe, c, pages, return_scores=True)
    rows_after = {k: v["launches"] for k, v in c.profile_report().items()}
    c.profile_enable(False)
    assert rows_after == rows_before and "warp_prepare_turned" not in rows_after and "orient_select" not in rows_after
    assert all(np.array_equal(a, b) for a, b in zip(b1, b0)) and np.array_equal(l1, l0)
    assert np.array_equal(s1[1], s0[1]) and np.array_equal(s1[2], s0[2])
    with pytest.raises(ValueError, match="orientation off"):
        c.recognition_orientation()


def test_pipeline_with_a_page_without_boxes_and_from_device_pointers(pipe, crnn_ctx):
    import torch

    c = crnn_ctx
    # a page on which this detector finds nothing: the first of a few flat pages (the head is calibrated on a text page, and a
    # flat page's border can still give a sliver)
    flat = [np.full((96, 128, 3), v, np.uint8) for v in (255, 0, 128, 64, 192, 32, 224, 160, 96)]
    blank = next((p for p in flat if not len(_run(pipe, c, [p])[0][0][0])), None)
    assert blank is not None, "no flat page without boxes"
    pages = _pages()[:1] + [blank] + _pages()[1:2]
    on, (hmax, wmax) = _run(pipe, c, pages, return_scores=True, orientation=ANY)
    assert len(on[0][1]) == 0 and len(on[0][0]) and len(on[0][2]), "a page without boxes between two with boxes"
    assert _tall_and_not(on[0])
    _check_against_path_3(c, on, _padded(c, pages, hmax, wmax))
    # the device-resident route
    dev = [torch.from_numpy(p).cuda() for p in pages]
    torch.cuda.synchronize()
    there, _ = _run(pipe, c, [t.data_ptr() for t in dev], shapes=pages, return_scores=True, orientation=ANY, on_device=True)
    for a, b in zip(there[0], on[0]):
        assert np.array_equal(a, b)
    _same((there[1], there[2][1], there[2][2], *there[3]), (on[1], on[2][1], on[2][2], *on[3]))
    res = c.pipeline_device_results()
    assert res["m"] == len(on[1]) and res["labels"]
    # zero images
    none = c.pipeline([], [], [], [], [], 32, 32, orientation=ANY)
    assert len(none) == 3 and [a.shape for a in none[2]] == [(0,), (0, 4, 2), (0, 2)]


# ---- 5. the public surface -------------------------------------------------------------------------------------------
def test_public_surface(pipe, crnn_ctx):
    c = crnn_ctx
    pages = _pages()
    before = pipe.recognize_with_scores(pages)
    (boxes, labels, how), _ = _run(pipe, c, pages, orientation=ANY)
    scales = pipe._plan([p.shape for p in pages])[0]  # pylint: disable=protected-access
    ends = np.cumsum([len(b) for b in boxes])
    want_boxes = pipe._adjust([how[1][e - len(b):e] for b, e in zip(boxes, ends)], scales)  # pylint: disable=protected-access
    want_texts = pipe.recognizer._decode(labels)  # pylint: disable=protected-access
    kwargs = {"orientation": "any"}
    out = pipe.recognize(pages, recognition_kwargs=kwargs)
    assert [t for group in out for t, _ in group] == want_texts
    for group, quads in zip(out, want_boxes):
        assert len(group) == len(quads) and all(np.array_equal(b, q) for (_, b), q in zip(group, quads))
    scored = pipe.recognize_with_scores(pages, recognition_kwargs=kwargs)
    assert [[t for t, _, _ in g] for g in scored] == [[t for t, _ in g] for g in out]
    raw = pipe.recognize_raw(pages, recognition_kwargs={"orientation": "any", "tall_ratio": 1.5})
    assert len(raw) == 3 and np.array_equal(raw[1], labels) and np.array_equal(raw[2][0], how[0]) and np.array_equal(raw[2][2], how[2])
    assert np.array_equal(raw[2][1], np.concatenate(want_boxes))
    lines = pipe.recognize_lines(pages, recognition_kwargs=kwargs)
    assert sum(len(words) for page in lines for _, _, words in page) == len(want_texts)
    true = [[{"text": t, "vertices": b} for t, b in group] for group in out]
    predictions, _, (precision, recall) = pipe.evaluate(pages, true, recognition_kwargs=kwargs)
    assert [[t for t, _ in g] for g in predictions] == [[t for t, _ in g] for g in out] and 0 <= precision <= 1 and 0 <= recall <= 1
    # refusals
    with pytest.raises(ValueError, match="orientation and beam_width"):
        pipe.recognize(pages, recognition_kwargs={"orientation": "any", "beam_width": 4})
    with pytest.raises(ValueError, match="orientation and char_boxes"):
        pipe.recognize_characters(pages, recognition_kwargs=kwargs)
    with pytest.raises(NotImplementedError, match="orientation"):
        pipe.recognize([p.astype(np.float32) for p in pages], recognition_kwargs=kwargs)
    with pytest.raises(ValueError, match="orientation and beam"):
        _run(pipe, c, pages, orientation=ANY, beam=(4, 2))
    with pytest.raises(ValueError, match="orientation and char_boxes"):
        _run(pipe, c, pages, orientation=ANY, char_boxes=True)
    for mode, ratio in ((3, 1.5), (-1, 1.5), (1, 0.0), (2, float("nan")), (2, float("inf")), ("up", 1.5)):
        with pytest.raises(ValueError):
            c.set_orientation(mode, ratio)
    c.set_beam(4, 2)
    try:
        with pytest.raises(ValueError, match="beam"):
            c.set_orientation("flip")
    finally:
        c.set_beam(0)
    c.set_char_boxes(True)
    try:
        with pytest.raises(ValueError, match="character boxes"):
            c.set_orientation("any", 1.5)
    finally:
        c.set_char_boxes(False)
    c.set_orientation("any", 2.5)
    assert c.get_orientation() == (2, 2.5)
    c.set_beam(4, 2)
    try:
        with pytest.raises(Exception, match="beam"):  # the combination is refused where the call is made, too
            c.recognize_boxes(np.stack(pages[:1]), [BOXES[:1]])
    finally:
        c.set_beam(0)
        c.set_orientation(0)
    assert c.get_orientation() == (0, 1.5)
    # a following default call is the one made before, bit for bit
    after = pipe.recognize_with_scores(pages)
    assert len(after) == len(before)
    for g0, g1 in zip(before, after):
        assert [t for t, _, _ in g0] == [t for t, _, _ in g1]
        assert all(np.array_equal(a[1], b[1]) and a[2].log_word == b[2].log_word and a[2].detection == b[2].detection for a, b in zip(g0, g1))
