"""The ordering contract of include/kocr.h, which every caller and the benchmark rely on:

  1. "calls on a ctx are serialised on its HIP stream"
         test_gated_device_call, test_gated_host_call (every launch, memset and copy of a call sits on the stream the
         context was given, in order), test_profiler_on_a_caller_stream (the profiler's events too)
  2. "Device-pointer calls are asynchronous on that stream unless they return host-side counts"
         test_gated_device_call: the calls that return nothing on the host come back while the gate ahead of them is
         still running; the documented exceptions (host counts or label rows, host boxes, host CTC labels, the resize
         tables) have complete and correct host outputs on return
  3. "separate contexts (also on one device) are independent"
         test_two_contexts_interleaved
  4. kocr_set_stream runs the context "on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)"
         test_gated_device_call / test_gated_host_call (a torch.cuda.Stream()), test_default_stream_handle_is_the_own_stream
         (handle 0, torch's default stream, selects the context's own non-blocking stream), test_switching_streams

The gate pattern is tests/stream_gate.py.  Its self-check is a condition, not a tolerance: the gate's GPU time must be at
least 4 x the host wall time of the call it shields, or the test fails as inconclusive.  For a call that returns while the
gate runs that is the wall time of the gated call itself.  A call that synchronises returns after the gate by definition,
so there the measure is the wall time of the same call, ungated and run to completion just before, which bounds the time
the library needs to enqueue its work from above.  Every test prints the gate and call times it measured (pytest -s) and
puts them into its assertion messages; the gate is sized at stream_gate.GATE_MS = 150 ms.

The argument lists and small inputs are those of tests/test_device_pointers_gpu.py.
"""
import numpy as np
import pytest

from tests import stream_gate as sg
from tests import synth
from tests.stream_gate import Case, HostOut, In, Out, Ptrs
from tests.test_device_pointers_gpu import N_CROPS, _ctc_inputs, _flat
from tests.test_device_pointers_gpu import box_groups, crops, dctx, pages  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

F32, I32, U8, F64, I64 = np.float32, np.int32, np.uint8, np.float64, np.int64
CAP = 64


def _boxes_view(boxes, counts):
    """the defined part of N x cap x 4 x 2 boxes: the counts, then counts[i] rows of image i"""
    return [counts] + [boxes[i, :max(0, min(int(c), boxes.shape[1]))] for i, c in enumerate(counts)]


def _partition(rng, total, parts, nonempty):
    """offsets int32 [parts + 1] from 0 to total, monotone (strictly when nonempty)"""
    if nonempty:
        cuts = np.sort(rng.choice(np.arange(1, total), parts - 1, replace=False))
    else:
        cuts = np.sort(rng.integers(0, total + 1, parts - 1))
    return np.concatenate([[0], cuts, [total]]).astype(I32)


def _quads(rng, n):
    """n rotated rectangles as int32 [n][4][2]"""
    out = []
    for _ in range(n):
        cx, cy, w, h, th = rng.uniform(60, 400), rng.uniform(60, 300), rng.uniform(40, 120), rng.uniform(15, 50), rng.uniform(-0.3, 0.3)
        c, s = np.cos(th), np.sin(th)
        out.append([(cx + x * c - y * s, cy + x * s + y * c) for x, y in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))])
    return np.asarray(out).astype(I32).reshape(n, 4, 2)


def _eval_inputs(seed, truths, preds):
    """one scoring batch: per image truths[i] truth boxes and preds[i] predictions, the first predictions jittered truths"""
    rng = np.random.default_rng(seed)
    tq = _quads(rng, sum(truths))
    toff, poff = np.concatenate([[0], np.cumsum(truths)]).astype(I32), np.concatenate([[0], np.cumsum(preds)]).astype(I32)
    pq = _quads(rng, sum(preds))
    for i in range(len(truths)):
        k = min(truths[i], preds[i])
        pq[poff[i]:poff[i] + k] = tq[toff[i]:toff[i] + k] + rng.integers(-4, 5, (k, 4, 2)).astype(I32)
    ignore = (rng.random(sum(truths)) < 0.25).astype(U8)
    words = [[ord(c) for c in w] for w in ("alpha", "bravo", "charlie", "delta", "ab", "ax", "echo", "")]
    tt = [words[int(rng.integers(len(words)))] for _ in range(sum(truths))]
    pt = [tt[toff[i] + j] if j < truths[i] and rng.random() < 0.6 else words[int(rng.integers(len(words)))]
          for i in range(len(preds)) for j in range(preds[i])]
    return tq, toff, pq, poff, ignore, tt, pt


def _texts(texts, total):
    """concatenated code points padded to `total`, and the offsets"""
    flat = [c for t in texts for c in t]
    off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(I32)
    assert len(flat) <= total
    return np.asarray(flat + [ord("z")] * (total - len(flat)), I32), off


def _eval_cases():
    # real: truths 3 + 4, predictions 5 + 3; poison: 4 + 3 and 3 + 5 -- other offsets, the same totals and the same 27 pairs
    r, p = _eval_inputs(21, (3, 4), (5, 3)), _eval_inputs(22, (4, 3), (3, 5))
    pairs = 27
    assert all(int((np.diff(v[1]) * np.diff(v[3])).sum()) == pairs for v in (r, p))
    total = 64
    (rtt, rtto), (ptt, ptto) = _texts(r[5], total), _texts(p[5], total)
    (rpt, rpto), (ppt, ppto) = _texts(r[6], total), _texts(p[6], total)
    quads = [In(r[0], p[0]), In(r[1], p[1]), In(r[2], p[2]), In(r[3], p[3])]
    iou = Case("kocr_iou_table", [2] + quads + [Out(pairs, F64), pairs, None], False)
    score = Case("kocr_score", [2] + quads + [In(r[4], p[4]), In(rtt, ptt), In(rtto, ptto), In(rpt, ppt), In(rpto, ppto), 0.5, 0.5,
                                              Out(pairs, U8), Out(7, U8), Out(8, U8), Out(3, I64), Out(pairs, F64), pairs, None], False)
    return {"kocr_iou_table": iou, "kocr_score": score}


def _maps_case():
    from keras_ocr_amd._lib import _flatten_lines
    from tests import maps_statement as ms
    from tests.test_maps_gpu import random_pages

    H, W = 130, 202
    q, sp, loff, ioff = _flatten_lines(random_pages(np.random.default_rng(H * 1000 + W), 4, H, W, 6))
    n, n_lines, rng = len(q), len(loff) - 1, np.random.default_rng(5)
    assert n > n_lines > 4
    hm = ms.get_gaussian_heatmap(37, 2.0)
    hm_p = rng.integers(0, 256, hm.shape, dtype=U8)
    q_p = np.ascontiguousarray(q[::-1] + F32(3))
    sp_p = np.where(np.arange(n) % 5 == 0, 1 - sp, sp).astype(U8)
    loff_p, ioff_p = _partition(rng, n, n_lines, True), _partition(rng, n_lines, 4, False)
    if np.array_equal(loff_p, loff) or np.array_equal(ioff_p, ioff):
        loff_p, ioff_p = _partition(rng, n, n_lines, True), _partition(rng, n_lines, 4, False)
    return Case("kocr_compute_maps", [In(hm, hm_p), hm.shape[0], hm.shape[1], 4, H, W, n, In(q, q_p), In(sp, sp_p), n_lines,
                                      In(loff, loff_p), In(ioff, ioff_p), Out((4, H // 2, W // 2, 2), F32)], True)


def _build_cases(ctx, pages, crops, box_groups):  # noqa: F811
    from oracle import tools as otools
    from keras_ocr_amd import detection

    lw, C = ctx.crnn_label_width(), ctx.crnn_classes()
    n, h, w, _ = pages.shape
    raw = [synth.text_page(64, 96, 4, seed=s) for s in (3, 4, 5, 6, 7, 8)]
    pages_p = np.stack([otools.resize_image(p, 2, 2048)[0] for p in raw[3:]])
    c5, c5_p = crops[:5], crops[5:10]
    cases = {}

    def add(key, *a, **k):
        cases[key] = Case(*a, **k)

    for key, dt, x, x_p in (("kocr_craft_forward[u8]", 0, pages, pages_p),
                            ("kocr_craft_forward[f32]", 1, pages.astype(F32) / 255, pages_p.astype(F32) / 255)):
        add(key, "kocr_craft_forward", [In(x, x_p), dt, n, h, w, Out((n, h // 2, w // 2, 2), F32), 2], True)
    add("kocr_crnn_forward", "kocr_crnn_forward", [In(c5, c5_p), 5, Out((5, lw), I32), Out((5, lw, C), F32)], True)
    add("kocr_crnn_forward[1030]", "kocr_crnn_forward",
        [In(crops, crops[::-1]), N_CROPS, Out((N_CROPS, lw), I32), Out((N_CROPS, lw, C), F32)], True)
    add("kocr_crnn_forward_scores", "kocr_crnn_forward_scores",
        [In(c5, c5_p), 5, Out((5, lw), I32), Out((5, lw, C), F32), Out(5, F32), Out((5, lw), F32)], True)
    add("kocr_crnn_beam", "kocr_crnn_beam", [In(c5, c5_p), 5, 8, 3, Out((5, 3, lw), I32), Out((5, 3), F32)], True)
    add("kocr_crnn_lexicon", "kocr_crnn_lexicon",
        [In(c5, c5_p), 5, 3, Out((5, 3), I32), Out((5, 3), F32), Out((5, ctx.lexicon_size()), F32)], True)
    add("kocr_crnn_features", "kocr_crnn_features", [In(c5, c5_p), 5, Out((5, 50, 256), F32)], True)
    rng = np.random.default_rng(2)
    src, src_p = rng.integers(0, 256, (2, 37, 53, 3), dtype=U8), rng.integers(0, 256, (2, 37, 53, 3), dtype=U8)
    # include/kocr.h: synchronises for its interpolation tables
    add("kocr_resize_pad", "kocr_resize_pad", [In(src, src_p), 2, 37, 53, 74, 106, 80, 112, 255, Out((2, 80, 112, 3), U8)], False)
    # the sizes of tests/test_maps_gpu.py::test_evaluate_mse and ::test_random_pages
    rng = np.random.default_rng(12)
    x, x_p = (detection.compute_input(rng.integers(0, 256, (5, 64, 96, 3), dtype=U8)) for _ in range(2))
    y, y_p, pred, pred_p = (rng.random((5, 32, 48, 2)).astype(F32) for _ in range(4))
    add("kocr_heat_mse", "kocr_heat_mse", [In(y, y_p), In(pred, pred_p), 5, 32, 48, Out(5, F64)], True)
    add("kocr_craft_mse", "kocr_craft_mse", [In(x, x_p), 1, 5, 64, 96, In(y, y_p), 2, Out(5, F64)], True)
    cases["kocr_compute_maps"] = _maps_case()
    # include/kocr.h: the CTC labels and lengths are host arrays, the two calls synchronise
    yp, yp_p = (np.random.default_rng(s).random((9, 20, 11), dtype=F32) for s in (5, 50))
    labels, ll, il = _ctc_inputs(9, 20, 11, 6)
    add("kocr_ctc_batch_cost", "kocr_ctc_batch_cost", [In(yp, yp_p), 9, 20, 11, labels, labels.shape[1], ll, il, Out(9, F32)], False)
    labels, ll, il = _ctc_inputs(5, lw, C, 8)
    add("kocr_crnn_ctc_loss", "kocr_crnn_ctc_loss", [In(c5, c5_p), 5, labels, labels.shape[1], ll, il, Out(5, F32)], False)
    # ---- documented as synchronising: host outputs complete on return ----
    heat = synth.heatmap_batch()
    add("kocr_get_boxes", "kocr_get_boxes", [In(heat[[0, 1, 2]], heat[[2, 0, 1]]), 3, heat.shape[1], heat.shape[2], 0.7, 0.4, 0.4, 10,
                                            Out((3, CAP, 4, 2), F32), HostOut(3, I32), CAP], False,
        view=lambda o: _boxes_view(o[0], o[1]), ok=(0, -6))
    add("kocr_detect", "kocr_detect", [In(pages, pages_p), 0, n, h, w, 0.7, 0.4, 0.4, 10, 2, Out((n, CAP, 4, 2), F32), HostOut(n, I32), CAP],
        False, view=lambda o: _boxes_view(o[0], o[1]))
    counts, flat = _flat(box_groups)
    m = int(counts.sum())
    add("kocr_warp_crops", "kocr_warp_crops", [In(pages, pages_p), n, h, w, flat, counts, 31, 200, Out((m, 31, 200), F32)], False)
    add("kocr_recognize_boxes", "kocr_recognize_boxes", [In(pages, pages_p), n, h, w, flat, counts, HostOut((m, lw), I32)], False)
    sizes = [np.full(3, v, I32) for v in (64, 96, 128, 192)]
    add("kocr_pipeline", "kocr_pipeline",
        [3, Ptrs([In(raw[i], raw[3 + i]) for i in range(3)])] + sizes + [128, 192, 0.7, 0.4, 0.4, 10, 2, HostOut((3, CAP, 4, 2), F32),
                                                                        HostOut(3, I32), CAP, HostOut((3 * CAP, lw), I32), 3 * CAP, HostOut(1, I32)],
        False, view=lambda o: _boxes_view(o[0], o[1]) + [o[3], o[2][:max(0, min(int(o[3][0]), 3 * CAP))]])
    cases.update(_eval_cases())
    # ---- host-pointer entry points (no on_device parameter): test_gated_host_call only ----
    srcf, srcf_p = src.astype(F32), src_p.astype(F32)
    add("kocr_resize_pad_f32", "kocr_resize_pad_f32", [In(srcf, srcf_p), 2, 37, 53, 3, 74, 106, 80, 112, 255.0, Out((2, 80, 112, 3), F32)],
        False, flag=False)
    add("kocr_warp_crops_f32", "kocr_warp_crops_f32",
        [In(pages.astype(F32), pages_p.astype(F32)), n, h, w, 3, flat, counts, 31, 200, Out((m, 31, 200), F32)], False, flag=False)
    return cases


DEVICE_CASES = ["kocr_craft_forward[u8]", "kocr_craft_forward[f32]", "kocr_crnn_forward", "kocr_crnn_forward[1030]",
                "kocr_crnn_forward_scores", "kocr_crnn_beam", "kocr_crnn_lexicon", "kocr_crnn_features", "kocr_resize_pad",
                "kocr_heat_mse", "kocr_craft_mse", "kocr_compute_maps", "kocr_ctc_batch_cost", "kocr_crnn_ctc_loss",
                "kocr_get_boxes", "kocr_detect", "kocr_warp_crops", "kocr_recognize_boxes", "kocr_pipeline", "kocr_iou_table",
                "kocr_score"]
HOST_CASES = DEVICE_CASES + ["kocr_resize_pad_f32", "kocr_warp_crops_f32"]


class _Env:
    pass


@pytest.fixture(scope="module")
def env(dctx, pages, crops, box_groups):  # noqa: F811
    """the module's context with a lexicon, its cases, three torch streams (never more at once), the gate and, per case,
    the reference: the host-array call on the context's own stream, computed once"""
    import torch
    import keras_ocr_amd

    e = _Env()
    e.ctx, e.lib = dctx, keras_ocr_amd.load_library()
    rng = np.random.default_rng(7)
    dctx.set_lexicon(rng.integers(0, dctx.crnn_classes() - 1, (40, 12)).astype(I32), rng.integers(1, 13, 40).astype(I32))
    e.cases = _build_cases(dctx, pages, crops, box_groups)
    assert sorted(e.cases) == sorted(HOST_CASES)
    e.streams = [torch.cuda.Stream() for _ in range(3)]
    e.gate = sg.Gate()
    e.refs = {}

    def reference(name):
        if name not in e.refs:
            case = e.cases[name]
            e.ctx.set_stream(None)
            rc, outs, _ = sg.host_call(e.lib, e.ctx, case, "real")
            rc_p, outs_p, _ = sg.host_call(e.lib, e.ctx, case, "poison")
            assert rc in case.ok and rc_p in case.ok, (name, rc, rc_p, e.ctx._lib.kocr_last_error(e.ctx._h))
            want, other = case.view(outs), case.view(outs_p)
            # the comparison proves something only if the poison gives another result
            assert not sg.same_bits(other, want), f"{name}: the poison gives the real inputs' result"
            e.refs[name] = (rc, want)
        return e.refs[name]

    e.reference = reference
    yield e
    dctx.set_stream(None)
    dctx.set_lexicon(None)


def _conclusive(name, g, shielded_ms, what):
    print(f"{name}: gate {g.gate_ms:.1f} ms, gated call {g.call_ms:.2f} ms, {what} {shielded_ms:.2f} ms")
    assert g.gate_ms >= 4 * shielded_ms, (f"{name}: INCONCLUSIVE, the gate was too short: gate {g.gate_ms:.1f} ms on the GPU < 4 x "
                                          f"{shielded_ms:.2f} ms ({what}); gated call {g.call_ms:.2f} ms")


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_gated_device_call(env, name):
    """on_device = 1 on a torch.cuda.Stream(): late inputs behind a gate, snapshots behind the call, nothing else"""
    case, s = env.cases[name], env.streams[0]
    rc_want, want = env.reference(name)
    env.ctx.set_stream(s.cuda_stream)
    # the first call grows arenas and may block.  The second is the ungated measure, and it runs on the POISON: every arena
    # buffer the gated call uses then holds poison-derived values, so an interior launch off the stream cannot find the right
    # activations of an earlier call lying there
    rc, _ = sg.device_call(env.lib, env.ctx, case, s)
    assert rc == rc_want, (name, rc)
    rc, warm_ms = sg.device_call(env.lib, env.ctx, case, s, "poison")
    assert rc in case.ok, (name, rc)
    g = sg.gated_call(env.lib, env.ctx, case, s, env.gate)
    assert g.rc == rc_want, (name, g.rc)
    times = f"gate {g.gate_ms:.1f} ms, gated call {g.call_ms:.2f} ms, ungated call to completion {warm_ms:.2f} ms"
    if case.asynchronous:
        assert g.gate_running, f"{name}: returned only after the gate had finished -- it blocks, or the gate was too short ({times})"
        _conclusive(name, g, g.call_ms, "host wall time of the gated call")
    else:
        _conclusive(name, g, warm_ms, "host wall time of the ungated call to completion")
    got = case.view(g.outs)
    assert sg.same_bits(got, want), (f"{name}: differs from the host-array call: the call read its inputs before they arrived, or "
                                     f"left an output unwritten ({times})")


@pytest.mark.parametrize("name", HOST_CASES)
def test_gated_host_call(env, name):
    """on_device = 0 on a torch.cuda.Stream() with a gate queued ahead: complete on return, equal to the own-stream result"""
    case, s = env.cases[name], env.streams[0]
    rc_want, want = env.reference(name)
    env.ctx.set_stream(s.cuda_stream)
    rc, outs, _ = sg.host_call(env.lib, env.ctx, case)
    assert rc == rc_want and sg.same_bits(case.view(outs), want), name
    # the last call before the gate runs on the POISON: the staged inputs and results it leaves in the arenas differ from
    # what the gated call must produce
    rc, outs, warm_ms = sg.host_call(env.lib, env.ctx, case, "poison")
    assert rc in case.ok and not sg.same_bits(case.view(outs), want), name
    g = sg.gated_call(env.lib, env.ctx, case, s, env.gate, on_device=0)
    assert g.rc == rc_want, (name, g.rc)
    _conclusive(name, g, warm_ms, "host wall time of the ungated call")
    assert sg.same_bits(case.view(g.outs), want), f"{name}: the host outputs were not complete and correct on return"


def _craft(env, ctx, d_img, d_heat, pages_shape):
    n, h, w, _ = pages_shape
    ctx.craft_forward_device(d_img.data_ptr(), 0, n, h, w, d_heat.data_ptr(), 2)


def test_default_stream_handle_is_the_own_stream(env, pages):  # noqa: F811
    """torch's default stream has handle 0, and handle 0 selects the context's own non-blocking stream (include/kocr.h:
    kocr_set_stream): the library's work does not wait for the legacy default stream, and the documented recipe --
    torch.cuda.synchronize() before the call, ctx.synchronize() after it -- gives correct results"""
    import torch

    _, (want,) = env.reference("kocr_craft_forward[u8]")
    assert torch.cuda.current_stream().cuda_stream == 0
    env.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    d_img = torch.from_numpy(pages).cuda().clone()   # produced by torch on the default stream
    d_heat = torch.zeros(want.shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    env.gate.run()   # the default stream is busy from here on
    e1.record()
    _craft(env, env.ctx, d_img, d_heat, pages.shape)
    env.ctx.synchronize()
    independent = not e1.query()
    torch.cuda.synchronize()
    assert independent, f"the call waited for the legacy default stream (gate {e0.elapsed_time(e1):.1f} ms): handle 0 is not the own stream"
    assert np.array_equal(d_heat.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # the recipe, with the inputs still being produced on the default stream when the host reaches the first synchronise
    env.gate.run()
    d_img2 = torch.from_numpy(pages).cuda() + 0
    d_heat.zero_()
    torch.cuda.synchronize()
    _craft(env, env.ctx, d_img2, d_heat, pages.shape)
    env.ctx.synchronize()
    assert np.array_equal(d_heat.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_switching_streams(env, pages):  # noqa: F811
    """kocr_set_stream synchronises the stream it leaves: an asynchronous call queued on A behind a gate is complete when
    set_stream(B) returns, so a copy on B alone sees the result; calls on B and on the own stream give the same bits"""
    import torch

    case = env.cases["kocr_craft_forward[u8]"]
    _, (want,) = env.reference("kocr_craft_forward[u8]")
    a, b = env.streams[1], env.streams[2]
    x = case.args[0]
    d_live, d_real = torch.from_numpy(x.poison).cuda(), torch.from_numpy(x.real).cuda()
    d_heat = torch.full(want.shape, -7.0, dtype=torch.float32, device="cuda")
    snap = torch.zeros_like(d_heat)
    env.ctx.set_stream(a.cuda_stream)
    _craft(env, env.ctx, d_real, d_heat, pages.shape)  # warm-up on A
    env.ctx.synchronize()
    d_heat.fill_(-7.0)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(a):
        e0.record()
        env.gate.run()
        e1.record()
        d_live.copy_(d_real, non_blocking=True)
        _craft(env, env.ctx, d_live, d_heat, pages.shape)
        returned_early = not e1.query()
    env.ctx.set_stream(b.cuda_stream)
    drained = e1.query()
    with torch.cuda.stream(b):
        snap.copy_(d_heat, non_blocking=True)   # ordered against A by nothing but set_stream's synchronisation
    b.synchronize()
    torch.cuda.synchronize()
    assert returned_early, f"inconclusive: the call on A was not asynchronous (gate {e0.elapsed_time(e1):.1f} ms)"
    assert drained, "set_stream returned while the gate on the old stream was still running"
    assert np.array_equal(snap.cpu().numpy().view(np.uint32), want.view(np.uint32)), "set_stream(B) returned before A's work was done"
    for target in (b.cuda_stream, None):
        env.ctx.set_stream(target)
        d_heat.fill_(-7.0)
        torch.cuda.synchronize()
        _craft(env, env.ctx, d_real, d_heat, pages.shape)
        env.ctx.synchronize()
        assert np.array_equal(d_heat.cpu().numpy().view(np.uint32), want.view(np.uint32)), target


@pytest.fixture(scope="module")
def ctx_y(craft_weights):
    """a second context on device 0: the other arithmetic mode, the unfolded schedule, other weights"""
    import keras_ocr_amd

    c = keras_ocr_amd.Context(0)
    c.set_split_mode(c.SPLIT_BF16X3)
    c.set_schedule(False, False)
    c.load_craft(craft_weights)
    c.load_crnn(keras_ocr_amd.weights.synthetic_crnn_weights(99))
    yield c
    c.close()


def test_two_contexts_interleaved(env, ctx_y, pages, crops):  # noqa: F811
    """X (default switches) and Y (bf16x3, unfolded, other weights), each on its own torch stream: asynchronous craft_forward and
    crnn_forward calls of the two interleaved with no synchronisation in between give each context's own results"""
    import torch

    x, c5 = env.ctx, crops[:5]
    n, h, w, _ = pages.shape
    lw, C = x.crnn_label_width(), x.crnn_classes()
    assert ctx_y.crnn_classes() == C
    x.set_stream(None)
    modes = {c: (c.get_split_mode(), c.get_schedule()) for c in (x, ctx_y)}
    assert modes[x] != modes[ctx_y]
    alone = {c: (c.craft_forward(pages, micro_batch=2),) + c.crnn_forward(c5, return_probs=True) for c in (x, ctx_y)}
    assert not np.array_equal(alone[x][0], alone[ctx_y][0]) and not np.array_equal(alone[x][2], alone[ctx_y][2])
    d_pages, d_crops = torch.from_numpy(pages).cuda(), torch.from_numpy(c5).cuda()
    out = {(c, r): (torch.full((n, h // 2, w // 2, 2), -7.0, dtype=torch.float32, device="cuda"),
                    torch.full((5, lw), -7, dtype=torch.int32, device="cuda"),
                    torch.full((5, lw, C), -7.0, dtype=torch.float32, device="cuda")) for c in (x, ctx_y) for r in range(2)}
    streams = {x: env.streams[1], ctx_y: env.streams[2]}
    for c in (x, ctx_y):
        c.set_stream(streams[c].cuda_stream)
        c.craft_forward_device(d_pages.data_ptr(), 0, n, h, w, out[c, 0][0].data_ptr(), 2)  # warm-up: arenas of the device path
        c.crnn_forward_device(d_crops.data_ptr(), 5, out[c, 0][1].data_ptr(), out[c, 0][2].data_ptr())
        c.synchronize()
        for t in out[c, 0]:
            t.fill_(-7)
    torch.cuda.synchronize()
    gate_end = []
    for s in streams.values():   # both streams start busy, so the calls below pile up on the two queues side by side
        with torch.cuda.stream(s):
            env.gate.run()
            gate_end.append(torch.cuda.Event())
            gate_end[-1].record()
    for r in range(2):
        for c in ((x, ctx_y) if r == 0 else (ctx_y, x)):
            c.craft_forward_device(d_pages.data_ptr(), 0, n, h, w, out[c, r][0].data_ptr(), 2)
        for c in (x, ctx_y):
            c.crnn_forward_device(d_crops.data_ptr(), 5, out[c, r][1].data_ptr(), out[c, r][2].data_ptr())
    piled_up = [not e.query() for e in gate_end]
    torch.cuda.synchronize()   # once
    assert all(piled_up), f"inconclusive: a gate had finished before all eight calls were enqueued {piled_up}"
    for (c, r), (heat, labels, probs) in out.items():
        who = "X" if c is x else "Y"
        assert np.array_equal(heat.cpu().numpy().view(np.uint32), alone[c][0].view(np.uint32)), f"{who} round {r}: heat-maps"
        assert np.array_equal(labels.cpu().numpy(), alone[c][1]), f"{who} round {r}: labels"
        assert np.array_equal(probs.cpu().numpy().view(np.uint32), alone[c][2].view(np.uint32)), f"{who} round {r}: probabilities"
    for c in (x, ctx_y):
        assert (c.get_split_mode(), c.get_schedule()) == modes[c]
        c.set_stream(None)


def test_profiler_on_a_caller_stream(env, pages):  # noqa: F811
    """the profiler's events are recorded on the context's stream: the same kernel names and launch counts either way"""
    rows = []
    for target in (None, env.streams[0].cuda_stream):
        env.ctx.set_stream(target)
        env.ctx.craft_forward(pages, micro_batch=2)
        env.ctx.profile_reset()
        env.ctx.profile_enable(True)
        try:
            env.ctx.craft_forward(pages, micro_batch=2)
            rows.append({k: v["launches"] for k, v in env.ctx.profile_report().items()})
        finally:
            env.ctx.profile_enable(False)
            env.ctx.profile_reset()
    assert rows[0] and sum(rows[0].values()) > 10
    assert rows[1] == rows[0]
