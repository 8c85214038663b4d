"""Lexicon-constrained recognition on the GPU (kocr_set_lexicon, kocr_crnn_lexicon; lexicon_logq / lexicon_score / lexicon_select
kernels; DESIGN.md section 4, "Lexicon") against the float64 statement tests/lexicon_statement.py, run on the GPU's own fc_12
logits (the "ctc" tap's input, as tests/test_beam_gpu.py takes them): only the match is under test here.

Values: the scoring kernel's own value of every (crop, word) pair must lie within the project's CTC gate of the statement,
|err| <= GATE * T * max(1, |value|) with GATE = 1e-6 (tests/test_ctc_loss_gpu.py), and be -inf exactly where the statement is.
Indices must equal the statement's top_words EXACTLY on every crop whose decision margin (lexicon_statement.top_words: the
smallest gap among ranks 1 .. K + 1 over max(1, |value at rank K + 1|)) exceeds twice that gate -- a decision compares two
values.  At least max(1, M // 2) crops must be compared (the rule of tests/test_crnn_gpu.py / test_beam_gpu.py); the compared
share and the largest fraction of the gate are printed (pytest -s).  log_prob must equal -crnn_ctc_loss of the crop with the
word bit for bit.

Inputs: synth.text_page crops of seeds 1000 .., the synthetic weights with fc_12 doubled (the beam test's sharpening), a
lexicon of 3000 random words (lengths 1 .. 12, labels 0 .. 35, np.random.default_rng(7)) merged as keras_ocr_amd.lexicon merges
duplicates.  On the CPU oracle's logits the statement alone leaves 24 / 19 / 17 of the first 24 crops above the margin at
K = 1 / 3 / 5 before the merge (the zero margins were duplicate one-letter words)."""
import numpy as np
import pytest

from tests import ctc_statement as cs
from tests import lexicon_statement as ls
from tests import synth

pytestmark = pytest.mark.gpu

GATE = 1e-6  # tests/test_ctc_loss_gpu.py
T = 50
SHARPEN = 2.0


def _crops(n, seed=1000):
    return np.stack([synth.text_page(31, 200, 3, seed=s)[..., 0] / np.float32(255) for s in range(seed, seed + n)])


def _sharpened(weights):
    w = dict(weights)
    w["fc_12/kernel"] = w["fc_12/kernel"] * np.float32(SHARPEN)
    w["fc_12/bias"] = w["fc_12/bias"] * np.float32(SHARPEN)
    return w


def _random_words(v, classes, seed=7, longest=12):
    """v random words, duplicates merged (first kept): labels (V', longest) int32 -1 padded, lengths (V',)"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, longest + 1, v)
    body = rng.integers(0, classes - 1, (v, longest))
    seen, rows = set(), []
    for n, row in zip(lengths, body):
        word = tuple(int(c) for c in row[:n])
        if word not in seen:
            seen.add(word)
            rows.append(word)
    return _rows(rows, longest)


def _rows(words, width=None):
    width = width or max(len(w) for w in words)
    labels = np.full((len(words), width), -1, np.int32)
    for i, w in enumerate(words):
        labels[i, :len(w)] = w
    return labels, np.array([len(w) for w in words], np.int32)


@pytest.fixture(scope="module")
def crnn_ctx(ctx, crnn_weights):
    ctx.crnn_set_rnn_steps_to_discard(2)
    ctx.load_crnn(_sharpened(crnn_weights))
    assert ctx.crnn_classes() == 37
    yield ctx
    ctx.set_lexicon(None)
    ctx.set_lexicon_scratch(0)
    ctx.load_crnn(crnn_weights)


def _logits(c, x):
    """fc_12's output (M, 50, C) of the crops, as the decode's launch read it"""
    c.crnn_set_taps(["ctc"])
    try:
        c.crnn_forward(x)
        taps = c.crnn_taps()
    finally:
        c.crnn_set_taps([])
    return taps["ctc"]["in"][0].reshape(len(x), T, -1)


def _statement(c, x, labels, lengths):
    from oracle import crnn as ocrnn

    lg = _logits(c, x)[:, T - c.crnn_label_width():].astype(np.float64)
    return ls.values(cs.log_q(ocrnn.softmax_f64(lg)), labels, lengths)


def _check_rows(c, x, labels, lengths, index, log_prob, values):
    """the rescoring contract: log_prob is -crnn_ctc_loss of crop and word, bit for bit; rows sorted (ties: the smaller index);
    the -1 / -inf tail only where fewer than K words are feasible; no word twice"""
    m, k = index.shape
    lw = c.crnn_label_width()
    assert index.dtype == np.int32 and log_prob.dtype == np.float32 and log_prob.shape == (m, k)
    assert index.max(initial=-1) < len(labels)
    feasible = np.isfinite(values).sum(-1)
    assert np.array_equal((index >= 0).sum(-1), np.minimum(feasible, k))
    for j in range(k):
        there = index[:, j] >= 0
        assert (log_prob[~there, j] == -np.inf).all() and np.isfinite(log_prob[there, j]).all()
        if j:
            assert (there <= (index[:, j - 1] >= 0)).all()  # the tail is a tail
            both = there
            ordered = (log_prob[both, j] < log_prob[both, j - 1]) | ((log_prob[both, j] == log_prob[both, j - 1]) & (index[both, j] > index[both, j - 1]))
            assert ordered.all()
        if there.any():
            words = index[there, j]
            loss = c.crnn_ctc_loss(x[there], labels[words], lengths[words], np.full(int(there.sum()), lw))
            assert np.array_equal(log_prob[there, j].view(np.uint32), (-loss).view(np.uint32))


def _check(c, x, labels, lengths, k, what):
    lw = c.crnn_label_width()
    c.set_lexicon(labels, lengths)
    assert c.lexicon_size() == len(labels)
    index, log_prob, values = c.crnn_lexicon(x, k, return_values=True)
    assert values.shape == (len(x), len(labels)) and values.dtype == np.float32
    plain = c.crnn_lexicon(x, k)
    assert np.array_equal(plain[0], index) and np.array_equal(plain[1].view(np.uint32), log_prob.view(np.uint32))
    want = _statement(c, x, labels, lengths)
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(values), fin) and (values[~fin] == -np.inf).all(), what
    gate = GATE * lw * np.maximum(1.0, np.abs(want[fin]))
    frac = float((np.abs(values[fin] - want[fin]) / gate).max()) if fin.any() else 0.0
    want_i, want_p, margin = ls.top_words(want, k)
    safe = margin > 2 * GATE * lw
    print(f"\n{what}: compared {int(safe.sum())} of {len(x)} crops; largest |value - statement| = {frac:.3f} of the gate")
    assert frac <= 1.0, what
    assert np.array_equal(index[safe], want_i[safe]), what
    assert safe.sum() >= max(1, len(x) // 2), what
    there = want_i[safe] >= 0
    err = np.abs(log_prob[safe][there] - want_p[safe][there])
    assert (err <= GATE * lw * np.maximum(1.0, np.abs(want_p[safe][there]))).all(), what
    _check_rows(c, x, labels, lengths, index, log_prob, values)
    return index, log_prob, values


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("v", [2, 64, 3000])
@pytest.mark.parametrize("m", [1, 5, 40])
def test_values_and_indices_equal_the_statement(crnn_ctx, m, v, k):
    labels, lengths = _random_words(v, 37)
    _check(crnn_ctx, _crops(m), labels, lengths, k, f"m={m} V={len(labels)} K={k}")


def test_tail_and_infeasible_words(crnn_ctx):
    """two words, K = 3: the third entry is -1 / -inf; a 32-letter word of one character needs 63 frames, has no alignment in
    48, is -inf in all_values and never returned; a lexicon of infeasible words only returns nothing, cleanly; M = 0 too"""
    x = _crops(5)
    labels, lengths = _rows([(3, 1, 4), (7,) * 32, (2, 7)])
    index, log_prob, values = _check(crnn_ctx, x, labels, lengths, 3, "two feasible words of three")
    assert (values[:, 1] == -np.inf).all() and (index[:, 2] == -1).all() and (log_prob[:, 2] == -np.inf).all()
    assert (np.sort(index[:, :2], axis=1) == [0, 2]).all()
    crnn_ctx.set_lexicon(*_rows([(7,) * 32, (5, 5) * 13]))
    index, log_prob, values = crnn_ctx.crnn_lexicon(x, 2, return_values=True)
    assert (index == -1).all() and (log_prob == -np.inf).all() and (values == -np.inf).all()
    empty = crnn_ctx.crnn_lexicon(x[:0], 4, return_values=True)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 4) and empty[2].shape == (0, 2)
    # equal words: the smaller index first, the same value
    crnn_ctx.set_lexicon(*_rows([(3, 1), (2, 7), (3, 1)]))
    index, log_prob = crnn_ctx.crnn_lexicon(x, 3)
    for row, vals in zip(index.tolist(), log_prob):
        assert row.index(0) + 1 == row.index(2) and vals[row.index(0)] == vals[row.index(2)]


def test_the_greedy_decode_in_the_lexicon(crnn_ctx):
    """each crop's own greedy decode joins the lexicon: where it is returned its log_prob is log_word of the scores, bit for
    bit, and only words of a higher rescored value (or an equal one and a smaller index) precede it; where it is not, every
    returned word beats it"""
    x = _crops(40)
    greedy, log_word, _ = crnn_ctx.crnn_forward_scores(x)
    labels, lengths = _random_words(3000, 37)
    words = [tuple(r[:n]) for r, n in zip(labels.tolist(), lengths)]
    where = {w: i for i, w in enumerate(words)}
    own = []
    for row in greedy:
        w = tuple(int(c) for c in row[row >= 0])
        if 1 <= len(w) <= 32 and w not in where:
            where[w] = len(words)
            words.append(w)
        own.append(where.get(w, -1))
    own = np.array(own)
    assert (own >= 0).sum() >= 20
    labels, lengths = _rows(words)
    index, log_prob, _ = _check(crnn_ctx, x, labels, lengths, 3, "greedy decodes in the lexicon")
    found = 0
    for i in np.flatnonzero(own >= 0):
        row = index[i].tolist()
        if own[i] in row:
            j = row.index(own[i])
            found += 1
            assert log_prob[i, j].view(np.uint32) == log_word[i].view(np.uint32)
            assert all(log_prob[i, a] > log_word[i] or (log_prob[i, a] == log_word[i] and row[a] < own[i]) for a in range(j))
        else:
            assert (log_prob[i] >= log_word[i]).all()
    print(f"\nthe greedy decode is among the 3 best of {len(words)} words on {found} of {int((own >= 0).sum())} crops")
    assert found >= 1


@pytest.mark.parametrize("discard", [0, 5])
@pytest.mark.parametrize("classes", [96, 1000])
def test_wide_alphabet_and_other_discards(ctx, crnn_weights, classes, discard):
    """96 classes (the table still fits LDS) and 1000 (it does not: the gather reads global memory); rnn_steps_to_discard 0 / 5"""
    import keras_ocr_amd

    try:
        ctx.crnn_set_rnn_steps_to_discard(discard)
        ctx.load_crnn(_sharpened(keras_ocr_amd.weights.synthetic_crnn_weights(4321, n_classes=classes)))
        assert ctx.crnn_classes() == classes and ctx.crnn_label_width() == T - discard
        labels, lengths = _random_words(300, classes, seed=11)
        assert labels.max() > 64
        for k in (1, 3):
            _check(ctx, _crops(9, seed=300), labels, lengths, k, f"{classes} classes, discard {discard}, K={k}")
    finally:
        ctx.set_lexicon(None)
        ctx.crnn_set_rnn_steps_to_discard(2)
        ctx.load_crnn(crnn_weights)


def test_invariance(crnn_ctx):
    """a crop's result is the same bits alone, in a batch of 40, at another position and under another scratch chunking;
    a permuted lexicon gives the same values and, where no two values of a crop are equal, the same words"""
    x = _crops(40)
    labels, lengths = _random_words(3000, 37)
    v = len(labels)
    bits = lambda a: a.view(np.uint32)
    crnn_ctx.set_lexicon(labels, lengths)
    index, log_prob, values = crnn_ctx.crnn_lexicon(x, 5, return_values=True)
    for i in (0, 7, 39):
        a = crnn_ctx.crnn_lexicon(x[i:i + 1], 5, return_values=True)
        assert np.array_equal(a[0][0], index[i]) and np.array_equal(bits(a[1][0]), bits(log_prob[i])) and np.array_equal(bits(a[2][0]), bits(values[i]))
    perm = np.roll(np.arange(40), 11)
    a = crnn_ctx.crnn_lexicon(x[perm], 5, return_values=True)
    assert np.array_equal(a[0], index[perm]) and np.array_equal(bits(a[1]), bits(log_prob[perm])) and np.array_equal(bits(a[2]), bits(values[perm]))
    try:
        crnn_ctx.set_lexicon_scratch(3 * 4 * v + 8)  # chunks of 3 crops
        a = crnn_ctx.crnn_lexicon(x, 5, return_values=True)
        b = crnn_ctx.crnn_lexicon(x, 5)
        crnn_ctx.set_lexicon_scratch(1)  # chunks of 1
        c = crnn_ctx.crnn_lexicon(x[:7], 5)
    finally:
        crnn_ctx.set_lexicon_scratch(0)
    assert np.array_equal(a[0], index) and np.array_equal(bits(a[1]), bits(log_prob)) and np.array_equal(bits(a[2]), bits(values))
    assert np.array_equal(b[0], index) and np.array_equal(bits(b[1]), bits(log_prob))
    assert np.array_equal(c[0], index[:7]) and np.array_equal(bits(c[1]), bits(log_prob[:7]))
    shuffle = np.random.default_rng(3).permutation(v)
    crnn_ctx.set_lexicon(labels[shuffle], lengths[shuffle])
    a = crnn_ctx.crnn_lexicon(x, 5, return_values=True)
    assert np.array_equal(bits(a[2]), bits(values[:, shuffle]))
    distinct = np.array([len(set(row.tolist())) == v for row in values])
    assert distinct.sum() >= 20
    assert np.array_equal(shuffle[a[0][distinct]], index[distinct]) and np.array_equal(bits(a[1][distinct]), bits(log_prob[distinct]))


def test_refusals_name_the_argument(crnn_ctx, crnn_weights):
    import keras_ocr_amd

    x = _crops(1)
    labels, lengths = _random_words(64, 37)
    crnn_ctx.set_lexicon(None)
    assert crnn_ctx.lexicon_size() == 0 and crnn_ctx.get_lexicon_match() == 0
    with pytest.raises(ValueError, match="no lexicon"):
        crnn_ctx.crnn_lexicon(x, 3)
    with pytest.raises(ValueError, match="no lexicon"):
        crnn_ctx.set_lexicon_match(3)
    crnn_ctx.set_lexicon(labels, lengths)
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="top_words"):
            crnn_ctx.crnn_lexicon(x, k)
        if k:
            with pytest.raises(ValueError, match="top_words"):
                crnn_ctx.set_lexicon_match(k)
    bad = labels.copy()
    bad[5, 0] = 36  # the blank
    with pytest.raises(ValueError, match=r"words: word 5: label 36"):
        crnn_ctx.set_lexicon(bad, lengths)
    assert crnn_ctx.lexicon_size() == 64  # a refused call changes nothing
    wide = np.zeros((3, 40), np.int32)
    with pytest.raises(ValueError, match=r"lengths: word 1 has length 33"):
        crnn_ctx.set_lexicon(wide, [4, 33, 2])
    with pytest.raises(ValueError, match=r"lengths: word 2 has length 0"):
        crnn_ctx.set_lexicon(wide, [4, 32, 0])
    # another recogniser with another class count unloads the lexicon and switches the match off
    crnn_ctx.set_lexicon(labels, lengths)
    crnn_ctx.set_lexicon_match(2)
    try:
        crnn_ctx.load_crnn(_sharpened(crnn_weights))  # the same class count: the lexicon stays
        assert crnn_ctx.lexicon_size() == len(labels) and crnn_ctx.get_lexicon_match() == 2
        crnn_ctx.load_crnn(keras_ocr_amd.weights.synthetic_crnn_weights(4321, n_classes=96))
        assert crnn_ctx.lexicon_size() == 0 and crnn_ctx.get_lexicon_match() == 0
        with pytest.raises(ValueError, match="37 classes.*96 classes"):
            crnn_ctx.crnn_lexicon(x, 3)
    finally:
        crnn_ctx.load_crnn(_sharpened(crnn_weights))
    # the fetch without anything resident / with the match off
    crnn_ctx.recognize_boxes(np.full((1, 40, 220, 3), 200, np.uint8), [np.array([[[2, 2], [210, 2], [210, 33], [2, 33]]], np.float32)])
    with pytest.raises(ValueError, match="match off"):
        crnn_ctx.recognition_lexicon()


# ---- end to end -----------------------------------------------------------------------------------------------------------

WORDS = ["the", "quick", "brown", "fox", "l1g", "1l1w", "al1tg", "a", "1", "11", "w1", "lig", "allg", "gtla", "tg", "zebra", "0"]


@pytest.fixture(scope="module")
def pipe(craft_weights, crnn_weights):
    import keras_ocr_amd
    from oracle import craft as ocraft, tools as otools

    page = synth.text_page(96, 128, 5, seed=21)[None]
    big = np.stack([otools.resize_image(p, 2, 2048)[0] for p in page])
    calibrated = keras_ocr_amd.weights.calibrate_craft_head(craft_weights, ocraft.detector_predict(craft_weights, big),
                                                            text_frac=0.10, link_frac=0.04)
    c = keras_ocr_amd.Context(0)
    det = keras_ocr_amd.detection.Detector(weights=calibrated, ctx=c)
    rec = keras_ocr_amd.recognition.Recognizer(weights=crnn_weights, ctx=c)
    yield keras_ocr_amd.pipeline.Pipeline(detector=det, recognizer=rec)
    c.close()


def _padded(pages):
    from oracle import tools as otools

    resized = [otools.resize_image(p, 2, 2048)[0] for p in pages]
    hmax, wmax = max(r.shape[0] for r in resized), max(r.shape[1] for r in resized)
    return np.stack([otools.pad(r, width=wmax, height=hmax) for r in resized])


def test_pipeline_equals_the_stages(pipe):
    import keras_ocr_amd

    ctx = pipe.detector._ctx  # pylint: disable=protected-access
    rec = pipe.recognizer
    pages = [synth.text_page(96, 128, 5, seed=21), synth.text_page(80, 100, 4, seed=22)]
    kwargs = {"lexicon_top": 3, "batch_size": 7}
    plain = pipe.recognize(pages)
    assert sum(len(g) for g in plain) >= 4
    with pytest.raises(ValueError, match="loaded lexicon"):
        pipe.recognize(pages, recognition_kwargs=kwargs)
    with pytest.raises(ValueError, match="loaded lexicon"):
        rec.recognize(_padded(pages)[0][:31, :200], lexicon_top=3)
    rec.set_lexicon(WORDS + ["The", "QUICK"], lowercase=True)
    assert rec.lexicon.words == WORDS and ctx.lexicon_size() == len(WORDS)
    matched = pipe.recognize(pages, recognition_kwargs=kwargs)
    assert ctx.get_lexicon_match() == 0
    assert all(np.array_equal(a[1], b[1]) for g, h in zip(plain, matched) for a, b in zip(g, h))
    assert [t for g in pipe.recognize(pages) for t, _ in g] == [t for g in plain for t, _ in g]
    batch = _padded(pages)
    boxes = pipe.detector.detect(batch)
    stages = rec.recognize_from_boxes(batch, boxes, lexicon_top=3)
    assert [[m for m, _ in g] for g in matched] == stages
    for matches in (m for g in stages for m in g):
        assert len(matches) == 3 and all(w in WORDS and isinstance(v, float) for w, v in matches)
        assert [v for _, v in matches] == sorted((v for _, v in matches), reverse=True)
        assert len({w for w, _ in matches}) == 3
    # one size, mixed sizes and float images take three branches of recognize_from_boxes
    taller = np.pad(batch[1], ((0, 2), (0, 0), (0, 0)))
    mixed = rec.recognize_from_boxes([batch[0], taller], boxes, lexicon_top=3)
    assert mixed[0] == stages[0]
    assert mixed[1:] == rec.recognize_from_boxes([taller], boxes[1:], lexicon_top=3)
    as_float = rec.recognize_from_boxes(list(batch.astype(np.float32)), boxes, lexicon_top=3)
    assert [[len(a) for a in g] for g in as_float] == [[len(a) for a in g] for g in stages]
    assert all(len(a) == 1 for g in rec.recognize_from_boxes(batch, boxes, lexicon_top=1) for a in g)
    assert all(len(a) == len(WORDS) for g in rec.recognize_from_boxes(batch, boxes, lexicon_top=64) for a in g)
    # the stage-wise pipeline (float pages) returns the same structure, and what its own stages return
    floats = pipe.recognize([p.astype(np.float32) for p in pages], recognition_kwargs=kwargs)
    plain_floats = pipe.recognize([p.astype(np.float32) for p in pages])
    assert [len(g) for g in floats] == [len(g) for g in plain_floats] and sum(len(g) for g in floats) >= 4
    assert all(np.array_equal(a[1], b[1]) for g, h in zip(plain_floats, floats) for a, b in zip(g, h))
    assert all(isinstance(m, list) and len(m) == 3 for g in floats for m, _ in g)
    # a duck-typed detector takes the stage-wise path on uint8 pages: the fused path's result

    class Detect:
        def detect(self, images, **kwargs):
            return pipe.detector.detect(images, **kwargs)

    staged = keras_ocr_amd.pipeline.Pipeline(detector=Detect(), recognizer=rec).recognize(pages, recognition_kwargs=kwargs)
    assert [[m for m, _ in g] for g in staged] == [[m for m, _ in g] for g in matched]
    # with scores: the score is the greedy decode's
    scored = pipe.recognize_with_scores(pages, recognition_kwargs=kwargs)
    greedy = pipe.recognize_with_scores(pages)
    for g, h, b in zip(scored, greedy, matched):
        assert [m for m, _, _ in g] == [m for m, _ in b]
        assert all(a[2].log_word == c[2].log_word and a[2].detection == c[2].detection and np.array_equal(a[2].characters, c[2].characters)
                   for a, c in zip(g, h))
        for (matches, _, score), (text, _, _) in zip(g, h):
            hit = [v for w, v in matches if w == text]
            assert not hit or np.float32(hit[0]) == np.float32(score.log_word)
    # a single crop
    crop = batch[0][:31, :200]
    one = rec.recognize(crop, lexicon_top=3)
    assert isinstance(one, list) and len(one) == 3 and isinstance(rec.recognize(crop), str)
    matches, score = rec.recognize(crop, return_scores=True, lexicon_top=3)
    assert matches == one and score.detection is None
    # refusals of the Python surface
    for bad in (0, 65):
        with pytest.raises(ValueError, match="lexicon_top"):
            pipe.recognize(pages, recognition_kwargs={"lexicon_top": bad})
        with pytest.raises(ValueError, match="lexicon_top"):
            rec.recognize(crop, lexicon_top=bad)
    with pytest.raises(ValueError, match="beam_width"):
        pipe.recognize(pages, recognition_kwargs={"lexicon_top": 3, "beam_width": 8})
    with pytest.raises(ValueError, match="beam_width"):
        rec.recognize_from_boxes(batch, boxes, lexicon_top=3, beam_width=8)
    with pytest.raises(ValueError, match="class count"):
        rec.set_lexicon(keras_ocr_amd.lexicon.Lexicon(["ab"], "abc"))
    with pytest.raises(ValueError, match="'café'"):
        rec.set_lexicon(["tea", "café"])
    with pytest.raises(NotImplementedError, match="lexicon"):
        keras_ocr_amd.dist.ShardedPipeline(pipeline=pipe).recognize(pages, recognition_kwargs=kwargs)
    rec.set_lexicon(None)
    assert ctx.lexicon_size() == 0 and rec.lexicon is None
    with pytest.raises(ValueError, match="loaded lexicon"):
        pipe.recognize(pages, recognition_kwargs=kwargs)


def test_lexicon_off_launches_what_it_always_launched(pipe):
    """off -- lexicon loaded or not -- the profiler rows of a pipeline call are the plain call's; on: three more rows, once
    per recogniser batch each"""
    ctx = pipe.detector._ctx  # pylint: disable=protected-access
    pages = [synth.text_page(96, 128, 5, seed=21), synth.text_page(80, 100, 4, seed=22)]

    def rows(kwargs):
        ctx.profile_enable(True)
        ctx.profile_reset()
        try:
            pipe.recognize(pages, recognition_kwargs=kwargs)
            return {name: row["launches"] for name, row in ctx.profile_report().items()}
        finally:
            ctx.profile_enable(False)

    unloaded = rows(None)
    pipe.recognizer.set_lexicon(WORDS)
    try:
        off, on = rows(None), rows({"lexicon_top": 3})
    finally:
        pipe.recognizer.set_lexicon(None)
    new = {"lexicon_logq", "lexicon_score", "lexicon_select"}
    assert not new & set(off) and off["ctc_greedy"] >= 1
    assert all(on.pop(name) == off["ctc_greedy"] for name in sorted(new))
    assert on == off == unloaded == rows({"batch_size": 4})
