"""CTC loss (kocr_ctc_batch_cost, kocr_crnn_ctc_loss) and the backbone features (kocr_crnn_features) on the GPU, against the
float64 statement of DESIGN.md section 4 (tests/ctc_statement.py) and the CPU oracle (oracle/crnn.py).

Gate for a loss computed from given probabilities: |loss - statement| <= 1e-6 * T_m * max(1, statement) (float32 log-space
recursion, one rounding per frame).  Infinite statements must be +inf on the GPU as well."""
import numpy as np
import pytest

from tests import ctc_statement as cs
from tests import synth

pytestmark = pytest.mark.gpu

GATE = 1e-6
# backbone features (LSTM outputs in (-1, 1)) vs the fp32 oracle: the conv stack runs in the fp16x2 split arithmetic, as for
# the probabilities (tests/test_crnn_gpu.py PROB_TOL = 1e-4); measured 1.13e-4 on the crops below
FEAT_TOL = 2e-4
MAX_RATIO = []  # largest |err| / gate per case, printed at the end (pytest -s)


def _crops(n, seed):
    x = np.zeros((n, 31, 200), np.float32)
    for i in range(n):
        x[i] = synth.text_page(31, 200, 3, seed=seed + i)[..., 0] / np.float32(255)
    return x


def _probs(rng, M, T, C, peaked):
    if peaked:  # one class takes almost all the mass, the rest a tiny Dirichlet share (down to underflow)
        y = rng.gamma(0.2, size=(M, T, C)) * 1e-6
        y[np.arange(M)[:, None], np.arange(T)[None, :], rng.integers(0, C, (M, T))] += 1.0
    else:
        y = rng.gamma(0.5, size=(M, T, C))
    return (y / y.sum(-1, keepdims=True)).astype(np.float32)


def _labels(rng, M, T, C, Tm):
    L = np.array([rng.integers(0, t + 1) for t in Tm])
    nf = M // 8
    L[1:1 + nf] = Tm[1:1 + nf]  # full-length labels (infeasible when two neighbours repeat)
    if M > 2:
        L[-1] = min(Tm[-1], max(65, Tm[-1] // 2))  # more states than lanes
    labels = np.full((M, T), -1, np.int32)
    for m in range(M):
        hi = 3 if m % 4 == 0 else C - 1  # every fourth sample: a small alphabet, many repeats
        labels[m, : L[m]] = rng.integers(0, hi, L[m])
    return labels, L


def _check_gate(got, want, Tm, what):
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf), what
    assert np.all(got[inf] > 0)
    assert np.all(np.isfinite(got[~inf])), what
    err = np.abs(got[~inf].astype(np.float64) - want[~inf])
    gate = GATE * Tm[~inf] * np.maximum(1.0, want[~inf])
    ratio = float((err / gate).max(initial=0.0))
    MAX_RATIO.append((what, ratio))
    print(f"\n{what}: max |err| / gate = {ratio:.3g} ({int((~inf).sum())} finite, {int(inf.sum())} +inf)")
    assert ratio <= 1.0, what


@pytest.fixture(scope="module")
def cctx(crnn_weights):
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    c.load_crnn(crnn_weights)
    yield c
    c.close()


@pytest.mark.parametrize("M,T,C,peaked", [
    (1, 48, 37, False), (7, 50, 1000, True), (512, 48, 37, False), (512, 50, 1000, False), (7, 300, 37, True),
    (64, 300, 1000, False), (512, 48, 37, True)])
def test_ctc_batch_cost_matches_the_statement(cctx, M, T, C, peaked):
    from keras_ocr_amd import recognition

    rng = np.random.default_rng(M * 1000 + T + C + peaked)
    y = _probs(rng, M, T, C, peaked)
    Tm = rng.integers(1, T + 1, M)
    Tm[0] = T
    labels, L = _labels(rng, M, T, C, Tm)
    want = cs.ctc_loss(y, labels, L, Tm)
    got = recognition.ctc_batch_cost(labels.astype(np.float32), y, Tm[:, None].astype(np.float32), L[:, None], ctx=cctx)
    assert got.shape == (M, 1) and got.dtype == np.float32
    assert np.isfinite(want).sum() >= max(1, M // 3)
    _check_gate(got[:, 0], want, Tm, f"ctc_batch_cost M={M} T={T} C={C} peaked={peaked}")


def test_one_frame_closed_form_infeasible_repeats_and_refusals(cctx):
    rng = np.random.default_rng(3)
    C = 37
    y = _probs(rng, 5, 4, C, False)
    lab = np.array([[4, -1], [-1, -1], [36 - 1, -1], [7, 7], [7, 8]], np.int32)
    got = cctx.ctc_batch_cost(y, lab, [1, 0, 1, 2, 2], [1, 1, 1, 2, 2])
    q = cs.log_q(y)
    want = -np.array([q[0, 0, 4], q[1, 0, C - 1], q[2, 0, 35]])
    assert np.all(np.abs(got[:3] - want) <= 1e-6 * np.maximum(1.0, want))
    assert np.isinf(got[3]) and got[3] > 0  # "aa" in two frames: no path
    assert np.isfinite(got[4])
    bad = [  # (labels, label_lengths, input_lengths, message)
        ([[1, 2]], [1], [0], "input_length"), ([[1, 2]], [1], [5], "input_length"),
        ([[1, 2]], [-1], [2], "label_length"), ([[1, 2, 3]], [3], [2], "label_length"),
        ([[36, 2]], [1], [2], "label 36"), ([[-1, 2]], [1], [2], "label -1"), ([[40, 2]], [1], [2], "label 40"),
        ([[1, 2]], [3], [4], "label row width")]
    for labs, ll, il, msg in bad:
        with pytest.raises(ValueError, match=msg) as e:
            cctx.ctc_batch_cost(y[:1], labs, ll, il)
        assert "sample 0" in str(e.value)
    with pytest.raises(ValueError, match="sample 1"):
        cctx.ctc_batch_cost(y[:2], [[1], [1]], [1, 1], [1, 0])
    assert np.array_equal(cctx.ctc_batch_cost(y, lab, [1, 0, 1, 2, 2], [1, 1, 1, 2, 2]), got, equal_nan=True)  # still usable


def _recognizer(ctx, weights, **build):
    import keras_ocr_amd
    from keras_ocr_amd.recognition import DEFAULT_BUILD_PARAMS

    n = weights["fc_12/bias"].shape[0]
    alphabet = keras_ocr_amd.recognition.DEFAULT_ALPHABET if n == 37 else "".join(chr(33 + i) for i in range(n - 1))
    return keras_ocr_amd.recognition.Recognizer(alphabet=alphabet, weights=dict(weights), ctx=ctx,
                                                build_params=dict(DEFAULT_BUILD_PARAMS, **build))


def _training_inputs(rng, labels_rows, lw, n_classes):
    """decoded rows, random strings and an empty label, all with input_length = lw (get_batch_generator's choice)"""
    M = labels_rows.shape[0]
    y_true = np.full((M, lw), -1.0, np.float32)
    L = np.zeros(M, np.int64)
    for m in range(M):
        if m % 3 == 0:
            row = labels_rows[m][labels_rows[m] >= 0]
        elif m % 3 == 1:
            row = rng.integers(0, n_classes - 1, rng.integers(1, 12))
        else:
            row = np.zeros(0, np.int64)
        y_true[m, : len(row)] = row
        L[m] = len(row)
    return y_true, np.full((M, 1), float(lw)), L[:, None].astype(np.float64)


def _check_training_model(rec, ctx, weights, x, discard, what):
    """training_model == ctc_batch_cost(model.predict) bit for bit; and within the Lipschitz bound of the oracle."""
    from keras_ocr_amd import recognition
    from oracle import crnn as ocrnn

    rng = np.random.default_rng(11)
    lw = ctx.crnn_label_width()
    assert rec.training_model.input_shape == [(None, 31, 200, 1), (None, lw), (None, 1), (None, 1)]
    assert rec.training_model.output_shape == (None, 1)
    rows = rec.prediction_model.predict(x[..., None])
    y_true, il, ll = _training_inputs(rng, rows, lw, ctx.crnn_classes())
    loss = rec.training_model.predict([x[..., None], y_true, il, ll], batch_size=4)
    probs = rec.model.predict(x[..., None])
    assert loss.shape == (x.shape[0], 1) and loss.dtype == np.float32
    assert np.array_equal(loss, recognition.ctc_batch_cost(y_true, probs, il, ll, ctx=ctx)), what
    w = weights if rec.build_params["stn"] else {k: v for k, v in weights.items() if not k.startswith("stn_")}
    want_p = ocrnn.crnn_forward(w, x[..., None], rnn_steps_to_discard=discard)
    Tm = il[:, 0].astype(np.int64)
    stmt = cs.ctc_loss(want_p, y_true.astype(np.int64), ll[:, 0].astype(np.int64), Tm)
    lip = np.abs(cs.log_q(probs) - cs.log_q(want_p)).max(-1).sum(-1)  # sum over frames of the max-norm of d log q
    gate = GATE * Tm * np.maximum(1.0, stmt)
    err = np.abs(loss[:, 0] - stmt)
    assert np.all(np.isfinite(stmt)) and np.all(err <= lip + gate), (what, err, lip)
    print(f"\n{what}: |loss - oracle statement| max {err.max():.3g}, Lipschitz bound min {lip.min():.3g}")
    return loss, probs, rows


def test_training_model_equals_ctc_batch_cost_and_the_oracle(cctx, crnn_weights):
    rec = _recognizer(cctx, crnn_weights)
    x = _crops(12, seed=700)
    loss, probs, rows = _check_training_model(rec, cctx, crnn_weights, x, 2, "training_model default")
    # the argmax path is one of the alignments of its own decoded label
    best = cs.log_q(probs).max(-1).sum(-1)
    L = (rows >= 0).sum(1)
    dec = cctx.crnn_ctc_loss(x, rows, L, np.full(len(x), rows.shape[1]))
    assert np.array_equal(dec[::3], loss[::3, 0])
    assert np.all(dec <= -best + 1e-5 * np.maximum(1.0, -best)), (dec, -best)
    with pytest.raises(NotImplementedError, match="inference-only"):
        rec.training_model.fit()
    with pytest.raises(NotImplementedError, match="inference-only"):
        rec.compile()


def test_loss_and_features_do_not_depend_on_the_batch(cctx):
    """A sample's loss and features do not depend on its position in the batch or on its neighbours (bit for bit).  Alone,
    the forward's 1x1 layers may take another GEMM kernel than at M = 512 (kocr_crnn_forward's own dispatch, unchanged
    here): there the loss agrees to float32 accumulation order, 1e-5 relative, and the features to the oracle's 1e-4."""
    x = _crops(512, seed=900)
    rng = np.random.default_rng(5)
    lw = cctx.crnn_label_width()
    labels = rng.integers(0, 36, (512, lw)).astype(np.int32)
    L = rng.integers(0, 20, 512)
    Tm = np.full(512, lw)
    loss = cctx.crnn_ctc_loss(x, labels, L, Tm)
    feats = cctx.crnn_features(x)
    assert np.all(np.isfinite(loss)) and feats.shape == (512, 50, 256)
    perm = np.roll(np.arange(512), 100)
    perm[[0, 7]] = perm[[7, 0]]
    loud = x[perm].copy()
    loud[1:] = 1.0 - loud[1:]  # every other neighbour inverted
    keep = [0]
    loss2 = cctx.crnn_ctc_loss(x[perm], labels[perm], L[perm], Tm[perm])
    feats2 = cctx.crnn_features(x[perm])
    assert np.array_equal(loss2, loss[perm]) and np.array_equal(feats2, feats[perm])
    loss3 = cctx.crnn_ctc_loss(loud, labels[perm], L[perm], Tm[perm])
    feats3 = cctx.crnn_features(loud)
    assert np.array_equal(loss3[keep], loss[perm][keep]) and np.array_equal(feats3[keep], feats[perm][keep])
    worst_l = worst_f = 0.0
    for i in (0, 257, 511):
        alone = cctx.crnn_ctc_loss(x[i:i + 1], labels[i:i + 1], L[i:i + 1], Tm[i:i + 1])
        fa = cctx.crnn_features(x[i:i + 1])
        worst_l = max(worst_l, float(abs(alone[0] - loss[i]) / max(1.0, abs(loss[i]))))
        worst_f = max(worst_f, float(np.abs(fa[0] - feats[i]).max()))
    print(f"\nalone vs in a batch of 512: loss {worst_l:.3g} relative, features {worst_f:.3g} absolute")
    assert worst_l <= 1e-5 and worst_f <= 1e-4


def test_backbone_matches_the_oracle(cctx, crnn_weights):
    from oracle import crnn as ocrnn

    rec = _recognizer(cctx, crnn_weights)
    assert rec.backbone.input_shape == (None, 31, 200, 1) and rec.backbone.output_shape == (None, 50, 256)
    x = _crops(6, seed=40)
    feats = rec.backbone.predict(x[..., None])
    _, inter = ocrnn.crnn_forward(crnn_weights, x[..., None], return_intermediates=True)
    assert feats.shape == inter["rnn_2"].shape == (6, 50, 256)
    err = float(np.abs(feats - inter["rnn_2"]).max())
    print(f"\nbackbone: max |feats - oracle| = {err:.3g}")
    assert err <= FEAT_TOL
    cctx.crnn_set_rnn_steps_to_discard(7)
    try:
        assert np.array_equal(cctx.crnn_features(x), feats)
    finally:
        cctx.crnn_set_rnn_steps_to_discard(2)


@pytest.mark.parametrize("build, classes", [({"stn": False}, 37), ({"rnn_steps_to_discard": 0}, 37), ({}, 96)],
                         ids=["no_stn", "discard_0", "classes_96"])
def test_non_default_builds(crnn_weights, build, classes):
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    try:
        w = crnn_weights if classes == 37 else keras_ocr_amd.weights.synthetic_crnn_weights(4321, n_classes=classes)
        rec = _recognizer(c, w, **build)
        discard = build.get("rnn_steps_to_discard", 2)
        assert rec.training_model.input_shape[1] == (None, 50 - discard)
        _check_training_model(rec, c, w, _crops(5, seed=60), discard, f"training_model {build} C={classes}")
        assert rec.backbone.predict(_crops(2, seed=61)).shape == (2, 50, 256)
    finally:
        c.close()


def test_zz_report_largest_ratio():
    print("\nlargest |err| / gate of ctc_batch_cost:", max(MAX_RATIO, key=lambda r: r[1]) if MAX_RATIO else None)
