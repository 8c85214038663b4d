"""The CTC kernels behind fc_12 (csrc/crnn_kernels.hip: ctc_kernel, ctc_scores_kernel, ctc_beam_kernel, ctc_loss_kernel<true>, the
three lexicon kernels) on the chosen logits of tests/decode_cases.py -- saturated frames, the 1e-7 floor, exact ties -- through
kocr_crnn_decode_logits, against the float64 statements (tests/ctc_statement.py, scores_statement.py, beam_statement.py,
lexicon_statement.py).  tests/test_decode_cases_cpu.py shows, with the statements alone, that every case compared here is
decidable and that every tie case hangs on the documented rule.

Bounds: the gate of tests/test_ctc_loss_gpu.py for every CTC total, |err| <= GATE * To * max(1, |value|), GATE = 1e-6, To the
frames after the discard; probabilities within tests/crnn_layer_check.py's check_ctc bound, (C + 8) u relative to the float64
softmax plus 2^-126 (below float32's smallest normal a probability is flushed: the floor family has such frames).  Label rows,
lexicon indices, character scores and the "same bits" statements are exact."""
import functools

import numpy as np
import pytest

from tests import beam_statement as bs
from tests import crnn_layer_check as lc
from tests import ctc_statement as cs
from tests import decode_cases as dc
from tests import lexicon_statement as ls
from tests import scores_statement as ss
from tests import synth

pytestmark = pytest.mark.gpu

GATE = dc.GATE
T = dc.T
CONFIGS = dc.configs()
LEXICON_CONFIGS = [cfg for cfg in CONFIGS if cfg[1] <= 5]


def _id(cfg):
    return f"C{cfg[0]}-d{cfg[1]}"


@functools.lru_cache(maxsize=None)
def _weights(classes):
    import keras_ocr_amd

    return keras_ocr_amd.weights.synthetic_crnn_weights(4321, n_classes=classes)


@pytest.fixture(scope="module")
def recogniser(ctx, crnn_weights):
    """at(classes, discard): the session's context with a recogniser of that many classes, that discard, lexicon(classes)"""
    state = {}

    def at(classes, discard, words=None):
        words = words or dc.lexicon(classes)
        if state.get("loaded") != (classes, words):
            ctx.load_crnn(_weights(classes))
            ctx.set_lexicon(*dc.rows(words))
            state["loaded"] = (classes, words)
        ctx.crnn_set_rnn_steps_to_discard(discard)
        assert ctx.crnn_classes() == classes and ctx.crnn_label_width() == T - discard
        return ctx

    yield at
    ctx.set_lexicon(None)
    ctx.crnn_set_rnn_steps_to_discard(2)
    ctx.load_crnn(crnn_weights)


def _stack(cases):
    return np.stack([c["logits"] for c in cases])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    """two result dicts of crnn_decode_logits hold the same bits"""
    return a.keys() == b.keys() and all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a)


def _rows_of(labels):
    """label rows (M, To) -1 padded -> (rows, lengths) as the loss takes them"""
    return labels, (labels >= 0).sum(-1)


def _within_gate(got, want, frames):
    """-inf / +inf exactly where the statement has them, the gate elsewhere"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    if not np.array_equal(got[~fin], want[~fin]):
        return False
    return bool((np.abs(got[fin] - want[fin]) <= GATE * frames * np.maximum(1.0, np.abs(want[fin]))).all())


# ---- greedy decode and probabilities -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_greedy_and_probabilities(recogniser, cfg):
    """labels are np.argmax (the first maximum) of the same float32 logits, collapsed -- exact, ties included; probabilities
    within check_ctc's bound of the float64 softmax; a shifted crop gives the same bits"""
    c = recogniser(*cfg)
    cases = dc.of_config(*cfg)
    out = c.crnn_decode_logits(_stack(cases), return_probs=True)
    assert out["labels"].dtype == np.int32 and out["labels"].shape == (len(cases), T - cfg[1])
    assert out["probs"].shape == (len(cases), T - cfg[1], cfg[0])
    for i, case in enumerate(cases):
        assert np.array_equal(out["labels"][i], dc.greedy(case["logits"][cfg[1]:])), case["name"]
        worst, rms = lc.check_ctc(case["logits"][None], out["probs"][i:i + 1], cfg[1])
        print(f"\n{case['name']}: probabilities at {worst:.3f} of the bound (rms {rms:.3f})")
        assert worst <= 1.0, (case["name"], worst)
        if case["same_as"]:
            j = [k["name"] for k in cases].index(case["same_as"])
            assert np.array_equal(out["labels"][i], out["labels"][j]) and np.array_equal(_bits(out["probs"][i]), _bits(out["probs"][j]))
    assert np.array_equal(c.crnn_decode_logits(_stack(cases))["labels"], out["labels"])  # without the probabilities too


def test_equals_the_entries_on_a_real_forward(recogniser):
    """on the logits a real forward produced (the "ctc" tap's input) every part equals its own entry point bit for bit"""
    ctx = recogniser(37, 2)
    x = np.stack([synth.text_page(31, 200, 3, seed=s)[..., 0] / np.float32(255) for s in range(1000, 1009)])
    ctx.crnn_set_taps(["ctc"])
    try:
        labels, probs = ctx.crnn_forward(x, return_probs=True)
        logits = ctx.crnn_taps()["ctc"]["in"][0].reshape(len(x), T, 37)
    finally:
        ctx.crnn_set_taps([])
    lengths = (labels >= 0).sum(-1)
    out = ctx.crnn_decode_logits(logits, return_probs=True, scores=True, beam=(16, 3), top_words=3, return_values=True,
                                 loss_labels=(labels, lengths, np.full(len(x), 48)))
    assert np.array_equal(out["labels"], labels) and np.array_equal(_bits(out["probs"]), _bits(probs))
    plain = ctx.crnn_decode_logits(logits, return_probs=True)
    assert np.array_equal(plain["labels"], labels) and np.array_equal(_bits(plain["probs"]), _bits(probs))
    _, log_word, chars = ctx.crnn_forward_scores(x)
    assert np.array_equal(_bits(out["log_word"]), _bits(log_word)) and np.array_equal(_bits(out["chars"]), _bits(chars))
    beam_labels, beam_log_prob = ctx.crnn_beam(x, 16, 3)
    assert np.array_equal(out["beam_labels"], beam_labels) and np.array_equal(_bits(out["beam_log_prob"]), _bits(beam_log_prob))
    index, log_prob, values = ctx.crnn_lexicon(x, 3, return_values=True)
    assert np.array_equal(out["lex_index"], index) and np.array_equal(_bits(out["lex_log_prob"]), _bits(log_prob))
    assert np.array_equal(_bits(out["lex_values"]), _bits(values))
    assert np.array_equal(_bits(out["loss"]), _bits(ctx.crnn_ctc_loss(x, labels, lengths, np.full(len(x), 48))))
    assert np.array_equal(ctx.crnn_forward(x), labels)  # and the forward is what it was


# ---- scores ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_scores(recogniser, cfg):
    """ctc_scores_kernel on every family, the tie families included (tests/test_scores_gpu.py keeps them out: no_ties)"""
    c = recogniser(*cfg)
    cases = dc.of_config(*cfg)
    frames = T - cfg[1]
    logits = _stack(cases)
    plain = c.crnn_decode_logits(logits, return_probs=True)
    out = c.crnn_decode_logits(logits, return_probs=True, scores=True)
    assert np.array_equal(out["labels"], plain["labels"]) and np.array_equal(_bits(out["probs"]), _bits(plain["probs"]))
    assert np.array_equal(_bits(out["chars"]), _bits(ss.char_scores(out["probs"])))
    want = ss.log_word(out["probs"])
    assert np.isfinite(want).all() and _within_gate(out["log_word"], want, frames)
    rows, lengths = _rows_of(out["labels"])
    loss = c.crnn_decode_logits(logits, loss_labels=(rows, lengths, np.full(len(cases), frames)))["loss"]
    assert np.array_equal(_bits(out["log_word"]), _bits(-loss))
    for i, case in enumerate(cases):
        if case["same_as"]:  # the shifted crop: the same bits
            j = [k["name"] for k in cases].index(case["same_as"])
            assert _same({k: v[i] for k, v in out.items()}, {k: v[j] for k, v in out.items()})


# ---- loss ------------------------------------------------------------------------------------------------------------------

def _loss_labels(case, rng):
    """label rows for one case: its own decode, the decode of the whole alphabet's cycle (full width), rows of one letter
    (L letters need 2 L - 1 frames: the long ones have no alignment), the empty row, random rows"""
    frames, blank = T - case["discard"], case["classes"] - 1
    own = [int(v) for v in dc.greedy(case["logits"][case["discard"]:]) if v >= 0]
    labels = [own, [t % blank for t in range(frames)], [1 % blank] * frames, [1 % blank] * (frames // 2 + 1), [1 % blank] * (frames // 2),
              [0, 0] * (frames // 4), []]
    labels += [[int(v) for v in rng.integers(0, blank, n)] for n in (1, min(7, frames), frames)]
    return labels


@pytest.mark.parametrize("cfg", CONFIGS, ids=_id)
def test_loss(recogniser, cfg):
    """ctc_loss_kernel<true> against ctc_statement.ctc_loss on the float64 softmax: the gate, +inf exactly where the statement
    is +inf; every case with ten label rows, all frames and (every third row) five fewer"""
    c = recogniser(*cfg)
    frames = T - cfg[1]
    rng = np.random.default_rng(40)
    logits, labels, in_len = [], [], []
    for case in dc.of_config(*cfg):
        for k, lab in enumerate(_loss_labels(case, rng)):
            tm = frames - 5 if k % 3 == 2 and frames > 5 + len(lab) else frames
            logits.append(case["logits"])
            labels.append(lab)
            in_len.append(tm)
    rows, lengths = dc.rows([lab or [-1] for lab in labels])
    lengths = np.array([len(lab) for lab in labels], np.int32)
    want = np.empty(len(labels))
    loss = np.empty(len(labels), np.float32)
    for s in range(0, len(labels), 64):  # at most 64 crops per call
        e = min(s + 64, len(labels))
        lg = np.stack(logits[s:e])
        loss[s:e] = c.crnn_decode_logits(lg, loss_labels=(rows[s:e], lengths[s:e], in_len[s:e]))["loss"]
        want[s:e] = cs.ctc_loss(dc.softmax(lg[:, cfg[1]:].astype(np.float64)), rows[s:e], lengths[s:e], in_len[s:e])
    assert np.isinf(want).any() and np.isfinite(want).any() and not np.isnan(want).any()
    assert (want[np.isinf(want)] > 0).all()
    bad = [(labels[i], in_len[i], loss[i], want[i]) for i in range(len(labels)) if not _within_gate(loss[i:i + 1], want[i:i + 1], frames)]
    assert not bad, bad[:3]


# ---- beam search -----------------------------------------------------------------------------------------------------------

def _check_rows(c, logits, labels, log_prob):
    """tests/test_beam_gpu.py's invariants: log_prob sorted and -loss of its row bit for bit; rows distinct, -1 padded on
    the right; missing rows all -1 with -inf"""
    m, k, frames = labels.shape
    assert (log_prob[:, 1:] <= log_prob[:, :-1]).all()  # (-inf behind -inf: no difference to take)
    lengths = (labels >= 0).sum(-1)
    assert all((row[:n] >= 0).all() and (row[n:] == -1).all() for rows, ns in zip(labels, lengths) for row, n in zip(rows, ns))
    assert labels.max() < c.crnn_classes() - 1
    assert np.isfinite(log_prob[:, 0]).all()
    for j in range(k):
        there = log_prob[:, j] != -np.inf
        assert (lengths[~there, j] == 0).all()
        if there.any():
            loss = c.crnn_decode_logits(logits[there], loss_labels=(labels[there, j], lengths[there, j], np.full(int(there.sum()), frames)))["loss"]
            assert np.array_equal(_bits(log_prob[there, j]), _bits(-loss))
    for rows, lp in zip(labels, log_prob):
        assert len({tuple(r) for r, v in zip(rows, lp) if v != -np.inf}) == int((lp != -np.inf).sum())


BEAM_RUNS = [(cfg, pair) for cfg in CONFIGS for pair in dc.BEAM_PAIRS if any(pair in case["beam"] for case in dc.of_config(*cfg))]


@pytest.mark.parametrize("cfg, pair", BEAM_RUNS, ids=lambda v: _id(v) if v in CONFIGS else f"B{v[0]}-K{v[1]}")
def test_beam(recogniser, cfg, pair):
    """rows equal the statement's on every committed case, ties included, values within the gate, -1 / -inf where the
    statement has fewer rows; saturated and floor crops: row 0 and its value, row 0 the greedy decode, the invariants on the rest"""
    cases = [case for case in dc.of_config(*cfg) if pair in case["beam"]]
    assert pair[0] < 64 or len(cases) <= 8
    c = recogniser(*cfg)
    frames = T - cfg[1]
    logits = _stack(cases)
    out = c.crnn_decode_logits(logits, beam=pair)
    labels, log_prob = out["beam_labels"], out["beam_log_prob"]
    assert labels.shape == (len(cases), pair[1], frames) and log_prob.shape == (len(cases), pair[1])
    for i, case in enumerate(cases):
        want_l, want_p, _ = dc.beam(case["name"], *pair)
        rows = slice(0, 1) if case["judge"] == "lead" else slice(None)
        assert np.array_equal(labels[i, rows], want_l[rows]), (case["name"], pair, labels[i, :3, :12], want_l[:3, :12])
        assert _within_gate(log_prob[i, rows], want_p[rows], frames), (case["name"], pair, log_prob[i, :3], want_p[:3])
        if case["judge"] == "lead":
            assert np.array_equal(labels[i, 0], out["labels"][i]), case["name"]
        if case["same_as"]:
            j = [k["name"] for k in cases].index(case["same_as"])
            assert np.array_equal(labels[i], labels[j]) and np.array_equal(_bits(log_prob[i]), _bits(log_prob[j]))
    _check_rows(c, logits, labels, log_prob)


def test_beam_equals_the_enumeration(recogniser):
    """4 classes, 3 frames, beam width 64: every labelling, in the order and with the values of the sum over all 4^3 alignments"""
    c = recogniser(4, 47)
    cases = dc.of_config(4, 47)
    out = c.crnn_decode_logits(_stack(cases), beam=(64, 64))
    for i, case in enumerate(cases):
        every = bs.all_labellings(dc.softmax(dc.decoded(case)))
        rows = [tuple(int(v) for v in r if v >= 0) for r in out["beam_labels"][i, :len(every)]]
        values = np.array([v for v, _ in every])
        assert _within_gate(out["beam_log_prob"][i, :len(every)], values, 3), case["name"]
        if case["judge"] == "lead":
            assert rows[0] == every[0][1]
        else:
            assert rows == [lab for _, lab in every], case["name"]
        assert (out["beam_labels"][i, len(every):] == -1).all() and (out["beam_log_prob"][i, len(every):] == -np.inf).all()


# ---- lexicon ---------------------------------------------------------------------------------------------------------------

def _check_lexicon(c, cases, words, k, indexed):
    """values of every (crop, word) pair within the gate, -inf where the word has no alignment; the indices of the crops in
    `indexed` equal top_words; log_prob is -loss of crop and word bit for bit"""
    frames = T - cases[0]["discard"]
    labels, lengths = dc.rows(words)
    logits = _stack(cases)
    out = c.crnn_decode_logits(logits, top_words=k, return_values=True)
    index, log_prob, values = out["lex_index"], out["lex_log_prob"], out["lex_values"]
    assert values.shape == (len(cases), len(words)) and index.shape == (len(cases), k)
    want = ls.values(cs.log_q(dc.softmax(logits[:, T - frames:].astype(np.float64))), labels, lengths)
    needs = np.array([ls.frames_needed(w) for w in words])
    assert np.array_equal(np.isfinite(want), np.broadcast_to(needs <= frames, want.shape))
    for i, case in enumerate(cases):
        assert _within_gate(values[i], want[i], frames), case["name"]
    want_i, want_p, _, _ = ls.top_words_ties(want, k)
    compared = 0
    for i, case in enumerate(cases):
        if (case["name"], k) in indexed:
            compared += 1
            assert np.array_equal(index[i], want_i[i]), (case["name"], index[i], want_i[i])
            assert _within_gate(log_prob[i], want_p[i], frames), case["name"]
    for j in range(k):
        there = index[:, j] >= 0
        assert (log_prob[~there, j] == -np.inf).all()
        if there.any():
            pick = index[there, j]
            loss = c.crnn_decode_logits(logits[there], loss_labels=(labels[pick], lengths[pick], np.full(int(there.sum()), frames)))["loss"]
            assert np.array_equal(_bits(log_prob[there, j]), _bits(-loss))
    assert np.array_equal((index >= 0).sum(-1), np.minimum(np.isfinite(values).sum(-1), k))
    for i, case in enumerate(cases):
        if case["same_as"]:  # the shifted crop: the same bits
            j = [k["name"] for k in cases].index(case["same_as"])
            assert all(np.array_equal(_bits(out[key][i]), _bits(out[key][j])) for key in ("lex_index", "lex_log_prob", "lex_values"))
    return index, log_prob, compared


@pytest.mark.parametrize("cfg", LEXICON_CONFIGS, ids=_id)
def test_lexicon(recogniser, cfg):
    c = recogniser(*cfg)
    cases = dc.of_config(*cfg)
    words = dc.lexicon(cfg[0])
    indexed = {(case["name"], k) for case, k in dc.lexicon_index_cases()}
    compared = 0
    for k in (dc.TOP_WORDS, dc.ALL_WORDS):
        index, log_prob, n = _check_lexicon(c, cases, words, k, indexed)
        compared += n
        if k != dc.ALL_WORDS:
            continue
        # twin words under twin columns: the same value, the smaller index first
        for i, case in enumerate(cases):
            if (case["name"], k) not in indexed:
                continue
            row = index[i].tolist()
            pairs = [(a, a + 1) for a in range(len(words) - 1)
                     if [7 if v == 3 else 3 if v == 7 else v for v in words[a]] == list(words[a + 1])]
            assert len(pairs) >= 6
            for a, b in pairs:
                assert row.index(a) + 1 == row.index(b) and log_prob[i, row.index(a)] == log_prob[i, row.index(b)], (case["name"], a, b)
    assert compared == sum(1 for case, _ in dc.lexicon_index_cases() if (case["classes"], case["discard"]) == cfg)


def _global_table_classes(frames, longest):
    """the smallest class count at which launch_lexicon_score's rows + table exceed 64 KB: rows = 128 lanes x R floats,
    R = (3 Lmax + 1) | 1; table = To x C floats"""
    rows = 128 * ((3 * longest + 1) | 1) * 4
    return (64 * 1024 - rows) // (frames * 4) + 1


def test_lexicon_saturated_with_the_table_in_global_memory(recogniser):
    """the saturated crops once more with an alphabet so wide that the log q table does not fit LDS beside the rows (a short
    lexicon keeps the rows small): lexicon_score_kernel<false>; test_lexicon runs <true> on the same family"""
    longest = 6
    classes = _global_table_classes(48, longest)
    rows = 128 * ((3 * longest + 1) | 1) * 4
    assert rows + 48 * classes * 4 > 64 * 1024 >= rows + 48 * (classes - 1) * 4 and rows + 48 * 96 * 4 <= 64 * 1024
    words = tuple(tuple(w) for w in dc.saturated_lexicon(classes, longest))
    assert max(len(w) for w in words) == longest
    c = recogniser(classes, 2, words=words)
    try:
        cases = dc._saturated_set(classes, 2, [], 14, boosts=(30, 8))  # pylint: disable=protected-access
        index, _, _ = _check_lexicon(c, cases, words, dc.TOP_WORDS, set())
        word = [i for i, case in enumerate(cases) if " word " in case["name"]]
        assert len(word) == 2 and (index[word, 0] == 0).all()
    finally:
        recogniser(37, 2)


# ---- independence ----------------------------------------------------------------------------------------------------------

def test_a_crop_does_not_depend_on_its_batch(recogniser):
    """the same bits alone, at another position, and beside a crop of another family: every part of the entry"""
    c = recogniser(37, 2)
    cases = dc.of_config(37, 2)
    logits = _stack(cases)
    rng = np.random.default_rng(41)
    rows, lengths = dc.rows([[int(v) for v in rng.integers(0, 36, n)] for n in rng.integers(1, 20, len(cases))])
    kwargs = dict(return_probs=True, scores=True, beam=(16, 3), top_words=3, return_values=True)

    def run(sel):
        return c.crnn_decode_logits(logits[sel], loss_labels=(rows[sel], lengths[sel], np.full(len(sel), 48)), **kwargs)

    whole = run(np.arange(len(cases)))
    perm = np.roll(np.arange(len(cases)), 7)
    assert _same(run(perm), {k: v[perm] for k, v in whole.items()})
    for i in (0, 5, len(cases) - 1):
        assert _same(run(np.array([i])), {k: v[i:i + 1] for k, v in whole.items()})
    families = [case["family"] for case in cases]
    a, b = families.index("saturated"), families.index("twins")
    assert _same(run(np.array([b, a])), {k: v[[b, a]] for k, v in whole.items()})


# ---- refusals --------------------------------------------------------------------------------------------------------------

def test_refusals(recogniser):
    import keras_ocr_amd

    c = recogniser(37, 2)
    lib, h = c._lib, c._h  # pylint: disable=protected-access
    lg = np.zeros((1, T, 37), np.float32)
    lab, lp = np.zeros((1, 64, 48), np.int32), np.zeros((1, 64), np.float32)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(logits=lg, m=1, labels=lab, log_word=None, chars=None, beam=(0, 1), beam_out=(None, None), top_words=0,
             lex_out=(None, None), loss=(None, 0, None, None, None), handle=h):
        return lib.kocr_crnn_decode_logits(handle, p(logits), m, p(labels), None, p(log_word), p(chars), beam[0], beam[1], p(beam_out[0]),
                                           p(beam_out[1]), top_words, p(lex_out[0]), p(lex_out[1]), None, p(loss[0]), loss[1], p(loss[2]),
                                           p(loss[3]), p(loss[4]))

    assert call() == 0 and call(m=0, logits=None, labels=None) == 0
    assert call(handle=None) == -1
    one = np.ones(1, np.int32)
    for kwargs, word in [(dict(logits=None), "null"), (dict(labels=None), "null"), (dict(m=-1), "null"),
                         (dict(log_word=lp), "log_word"), (dict(beam=(4, 1)), "null"), (dict(beam=(4, 1), beam_out=(lab, None)), "null"),
                         (dict(top_words=3), "null"), (dict(top_words=3, lex_out=(lab, None)), "null"),
                         (dict(loss=(lab, 48, one, None, lp)), "null"), (dict(loss=(lab, 48, one, one, None)), "null"),
                         (dict(m=1025), "1024"),
                         (dict(beam=(65, 1), beam_out=(lab, lp)), "beam_width"), (dict(beam=(-1, 1), beam_out=(lab, lp)), "beam_width"),
                         (dict(beam=(4, 5), beam_out=(lab, lp)), "top_paths"), (dict(beam=(4, 0), beam_out=(lab, lp)), "top_paths"),
                         (dict(top_words=65, lex_out=(lab, lp)), "top_words"), (dict(top_words=-1, lex_out=(lab, lp)), "top_words"),
                         (dict(loss=(lab, 48, one * 49, one * 48, lp)), "label_length"),
                         (dict(loss=(lab, 48, one, one * 49, lp)), "input_length"),
                         (dict(loss=(lab + 36, 48, one, one * 48, lp)), "label 36")]:
        assert call(**kwargs) == -1 and word in lib.kocr_last_error(h).decode(), (kwargs.keys(), word, lib.kocr_last_error(h))
    with pytest.raises(ValueError, match="shape"):
        c.crnn_decode_logits(np.zeros((1, T, 36), np.float32))
    with pytest.raises(ValueError, match="beam_width"):
        c.crnn_decode_logits(lg, beam=(65, 1))
    with pytest.raises(ValueError, match="top_words"):
        c.crnn_decode_logits(lg, top_words=65)
    with pytest.raises(ValueError, match="1024"):
        c.crnn_decode_logits(np.zeros((1025, T, 37), np.float32))
    assert c.crnn_decode_logits(np.zeros((1024, T, 37), np.float32))["labels"].shape == (1024, 48)  # one whole batch is taken
    c.set_lexicon(None)
    try:
        with pytest.raises(ValueError, match="no lexicon"):
            c.crnn_decode_logits(lg, top_words=3)
    finally:
        c.set_lexicon(*dc.rows(dc.lexicon(37)))
    fresh = keras_ocr_amd.Context(0)
    try:
        rc = call(handle=fresh._h)  # pylint: disable=protected-access
        assert rc == keras_ocr_amd._lib.KOCR_ENOWEIGHTS and "kocr_load_crnn" in lib.kocr_last_error(fresh._h).decode()  # pylint: disable=protected-access
    finally:
        fresh.close()
    assert c.crnn_decode_logits(lg)["labels"].shape == (1, 48)  # and the context still works
