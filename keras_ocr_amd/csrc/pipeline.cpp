// pipeline.cpp — the fused device path of Pipeline.recognize (pipeline.py:28-75):
//   resize_image + pad (pipeline.py:44-57)  ->  Detector.detect (:62; detection.py:745-785)
//   ->  Recognizer.recognize_from_boxes (:63-65; recognition.py:491-537).
// Everything stays resident in HBM between the stages; the host sees only the per-image box
// counts (a few bytes, needed to size the crop batch), the boxes and the decoded label rows.
#include "abi.h"

extern "C" int kocr_resize_pad(kocr_ctx* ctx, const uint8_t* src, int n, int sh, int sw, int dh, int dw, int Hmax,
                               int Wmax, int cval, uint8_t* dst, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (n < 0 || (n > 0 && (!src || !dst))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_resize_pad: null buffer");
  if (n == 0) return KOCR_OK;
  ctx->invalidate_results();
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t sb = (size_t)n * sh * sw * 3, db = (size_t)n * Hmax * Wmax * 3;
  const size_t tb = (size_t)(4 * (Wmax + Hmax) + 64) * sizeof(int);
  Staging st{ctx, ctx->io, "kocr_resize_pad", on_device != 0};
  KOCR_TRY(st.reserve(tb, {sb, db}));
  const uint8_t* d_src;
  uint8_t* d_dst;
  KOCR_TRY(st.in(src, sb, d_src));
  KOCR_TRY(st.out(dst, db, d_dst));
  KOCR_TRY(launch_resize_pad(ctx, d_src, n, sh, sw, d_dst, dh, dw, Hmax, Wmax, cval, ctx->io));
  KOCR_TRY(st.back(dst, d_dst, db));
  return st.finish();
}

// Detector.detect's device half in one call: CRAFT forward + getBoxes, heat-maps never leave HBM.
extern "C" int kocr_detect(kocr_ctx* ctx, const void* img, int dtype, int N, int H, int W, float detection_threshold,
                           float text_threshold, float link_threshold, int size_threshold, int micro_batch,
                           float* boxes, int32_t* counts, int cap, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || (N > 0 && (!img || !boxes || !counts))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_detect: null buffer");
  if (dtype != KOCR_U8 && dtype != KOCR_F32) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_detect: bad dtype");
  if (N == 0) return KOCR_OK;
  if (cap <= 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_detect: cap must be positive");
  ctx->invalidate_results();
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int h2 = H / 2, w2 = W / 2;
  const size_t in_img = (size_t)H * W * 3 * (dtype == KOCR_U8 ? 1 : 4);
  const size_t heat_b = (size_t)N * h2 * w2 * 2 * sizeof(float);
  const size_t box_b = (size_t)N * cap * 8 * sizeof(float);
  Staging st{ctx, ctx->pl, "kocr_detect", on_device != 0};
  KOCR_TRY(st.reserve(0, {in_img * N}, {heat_b, box_b}));  // box_b on the device path too: the pl arena keeps its size
  float* d_heat;
  float* d_boxes;
  const char* d_in;
  KOCR_TRY(st.scratch(heat_b, d_heat));
  KOCR_TRY(st.out(boxes, box_b, d_boxes));
  KOCR_TRY(st.in((const char*)img, in_img * N, d_in));
  const int mb = craft_micro_batch(micro_batch, N, H, W);
  KOCR_TRY(ctx->ws_reserve(craft_workspace_bytes(mb, H, W)));
  for (int s = 0; s < N; s += mb) {
    const int nb = std::min(mb, N - s);
    ctx->ws_reset();
    KOCR_TRY(craft_forward(ctx, d_in + (size_t)s * in_img, dtype, nb, H, W, d_heat + (size_t)s * h2 * w2 * 2));
  }
  int n_empty = 0;
  const float* d_scores = nullptr;
  KOCR_TRY(postproc_get_boxes(ctx, d_heat, N, h2, w2, detection_threshold, text_threshold, link_threshold,
                              size_threshold, d_boxes, cap, counts, &n_empty, nullptr, &d_scores));
  KOCR_TRY(chars_resident(ctx, "kocr_detect", d_heat, N, h2, w2, d_boxes, cap, counts));
  KOCR_TRY(st.back(boxes, d_boxes, box_b));
  KOCR_TRY(st.finish());
  ctx->keep_det_scores(d_scores, N, cap);
  if (n_empty > 0)
    KOCR_FAIL(ctx, KOCR_EEMPTYCONTOUR, "kocr_detect: empty contour list (IndexError at detection.py:272)");
  return KOCR_OK;
}

// Recognizer.recognize_from_boxes' device half in one call: crops are warped and recognised without
// leaving HBM.  All N images share one size; boxes/counts/labels are HOST buffers.
extern "C" int kocr_recognize_boxes(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                    const int32_t* counts, int32_t* labels, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || (N > 0 && (!img_rgb || !counts))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognize_boxes: null buffer");
  const int C = crnn_classes(ctx);
  if (C == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_recognize_boxes: call kocr_load_crnn first");
  std::vector<WarpParam> prm;
  const long M = prepare_box_warps(ctx, "kocr_recognize_boxes", N, boxes, counts, labels, CRNN_CROP_H, CRNN_CROP_W, prm);
  if (M <= 0) return (int)M;
  ctx->invalidate_results();
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int LW = crnn_label_width(ctx);
  const size_t ib = (size_t)N * H * W * 3, crop_b = (size_t)M * CRNN_CROP_PIXELS * sizeof(float);
  const size_t lab_b = (size_t)M * LW * sizeof(int32_t), pb = (size_t)M * sizeof(WarpParam);
  const bool scores = ctx->scores_on;
  const size_t lw_b = scores ? (size_t)M * sizeof(float) : 0, ch_b = lw_b * LW;
  const int BW = ctx->beam_width, BK = ctx->beam_top_paths;
  const size_t bl_b = BW ? (size_t)M * BK * LW * sizeof(int32_t) : 0, bv_b = BW ? (size_t)M * BK * sizeof(float) : 0;
  const int LK = ctx->lex_top;
  const size_t li_b = LK ? (size_t)M * LK * sizeof(int32_t) : 0, lv_b = LK ? (size_t)M * LK * sizeof(float) : 0;
  Staging st{ctx, ctx->io, "kocr_recognize_boxes", on_device != 0};
  KOCR_TRY(st.reserve(0, {ib}, {pb, crop_b, lab_b, lw_b, ch_b, bl_b, bv_b, li_b, lv_b}));
  const WarpParam* d_prm;
  float* d_crops;
  int32_t* d_lab;
  const uint8_t* d_img;
  CrnnScores sc{nullptr, nullptr};
  KOCR_TRY(st.scratch(pb, d_prm));
  KOCR_TRY(st.scratch(crop_b, d_crops));
  KOCR_TRY(st.scratch(lab_b, d_lab));
  if (scores) {
    KOCR_TRY(st.scratch(lw_b, sc.d_logw));
    KOCR_TRY(st.scratch(ch_b, sc.d_chars));
  }
  CrnnBeam bm{BW, BK, nullptr, nullptr};
  if (BW) {
    KOCR_TRY(st.scratch(bl_b, bm.d_labels));
    KOCR_TRY(st.scratch(bv_b, bm.d_logp));
  }
  CrnnLexicon lx{LK, nullptr, nullptr, nullptr};
  if (LK) {
    KOCR_TRY(st.scratch(li_b, lx.d_index));
    KOCR_TRY(st.scratch(lv_b, lx.d_logp));
  }
  KOCR_TRY(st.in(img_rgb, ib, d_img));
  KOCR_TRY(st.put((WarpParam*)d_prm, prm.data(), pb));
  KOCR_TRY(launch_warp(ctx, d_img, H, W, d_prm, (int)M, CRNN_CROP_H, CRNN_CROP_W, d_crops));
  KOCR_TRY(ctx->ws_reserve(crnn_workspace_bytes(crnn_batch(M), C) + (LK ? lexicon_workspace_bytes(ctx, crnn_batch(M), true) : 0)));
  KOCR_TRY(crnn_batches(ctx, M, [&](long s, int nb) {
    const CrnnScores part{scores ? sc.d_logw + s : nullptr, scores ? sc.d_chars + s * LW : nullptr};
    const CrnnBeam bpart{BW, BK, BW ? bm.d_labels + s * BK * LW : nullptr, BW ? bm.d_logp + s * BK : nullptr};
    const CrnnLexicon lpart{LK, LK ? lx.d_index + s * LK : nullptr, LK ? lx.d_logp + s * LK : nullptr, nullptr};
    return crnn_forward(ctx, d_crops + s * CRNN_CROP_PIXELS, nb, d_lab + s * LW, nullptr, CRNN_DECODE, nullptr, nullptr,
                        scores ? &part : nullptr, BW ? &bpart : nullptr, LK ? &lpart : nullptr);
  }));
  KOCR_TRY(st.download(labels, d_lab, lab_b));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->keep_rec_scores(sc.d_logw, sc.d_chars, (int)M, LW);
  ctx->keep_beams(bm.d_labels, bm.d_logp, (int)M, LW);
  ctx->keep_lexicon(lx.d_index, lx.d_logp, (int)M);
  return KOCR_OK;
}

extern "C" int kocr_pipeline(kocr_ctx* ctx, int N, const uint8_t* const* imgs, const int32_t* hs, const int32_t* ws,
                             const int32_t* dhs, const int32_t* dws, int Hmax, int Wmax, float detection_threshold,
                             float text_threshold, float link_threshold, int size_threshold, int micro_batch,
                             float* boxes, int32_t* counts, int cap, int32_t* labels, int max_crops,
                             int32_t* n_crops, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (n_crops) *n_crops = 0;
  if (N < 0 || (N > 0 && (!imgs || !hs || !ws || !dhs || !dws || !boxes || !counts)))
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_pipeline: null buffer");
  ctx->invalidate_results();
  if (N == 0) return KOCR_OK;
  if (!ctx->craft) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_pipeline: call kocr_load_craft first");
  if (crnn_classes(ctx) == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_pipeline: call kocr_load_crnn first");
  if (Hmax < 16 || Wmax < 16 || cap <= 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_pipeline: bad sizes");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int h2 = Hmax / 2, w2 = Wmax / 2;
  const size_t bat_b = (size_t)N * Hmax * Wmax * 3;
  const size_t heat_b = (size_t)N * h2 * w2 * 2 * sizeof(float);
  const size_t box_b = (size_t)N * cap * 8 * sizeof(float);
  // ---- persistent buffers of this call ----
  Staging pl{ctx, ctx->pl, "kocr_pipeline"};
  KOCR_TRY(pl.reserve(0, {}, {bat_b, heat_b, box_b}));
  uint8_t* d_bat;
  float *d_heat, *d_boxes;
  KOCR_TRY(pl.scratch(bat_b, d_bat));
  KOCR_TRY(pl.scratch(heat_b, d_heat));
  KOCR_TRY(pl.scratch(box_b, d_boxes));
  // ---- resize + pad, runs of identically-shaped contiguous images in one launch ----
  Staging io{ctx, ctx->io, "kocr_pipeline", on_device != 0};
  int i = 0;
  while (i < N) {
    int j = i + 1;
    while (j < N && hs[j] == hs[i] && ws[j] == ws[i] && dhs[j] == dhs[i] && dws[j] == dws[i] &&
           imgs[j] == imgs[j - 1] + (size_t)hs[i] * ws[i] * 3)
      ++j;
    const int run = j - i;
    const size_t sb = (size_t)run * hs[i] * ws[i] * 3;
    const size_t tb = (size_t)(4 * (Wmax + Hmax) + 64) * sizeof(int);
    KOCR_TRY(io.reserve(tb, {sb}));
    const uint8_t* d_src;
    KOCR_TRY(io.in(imgs[i], sb, d_src));
    KOCR_TRY(launch_resize_pad(ctx, d_src, run, hs[i], ws[i], d_bat + (size_t)i * Hmax * Wmax * 3, dhs[i], dws[i],
                               Hmax, Wmax, 255, ctx->io));
    i = j;
  }
  // ---- detector forward (micro-batched) ----
  const int mb = craft_micro_batch(micro_batch, N, Hmax, Wmax);
  KOCR_TRY(ctx->ws_reserve(craft_workspace_bytes(mb, Hmax, Wmax)));
  for (int s = 0; s < N; s += mb) {
    const int nb = std::min(mb, N - s);
    ctx->ws_reset();
    KOCR_TRY(craft_forward(ctx, d_bat + (size_t)s * Hmax * Wmax * 3, KOCR_U8, nb, Hmax, Wmax,
                           d_heat + (size_t)s * h2 * w2 * 2));
  }
  // ---- boxes: the host learns only the per-image counts here (needed to size the crop batch); the boxes themselves
  // go to the caller asynchronously while the device already derives the crop homographies from its own copy ----
  // CAPACITY WITHOUT RECOMPUTATION (round 6; the reference has no cap, detection.py:230-286): `cap` and `max_crops` size the
  // CALLER's buffers only.  A page with more boxes than cap gets a larger device box buffer (its own arena: growing the pl
  // arena would free the heat-maps) and ONLY the post-processing runs again on the resident heat-maps -- it stops at its
  // counting pass when the capacity does not suffice, so the first attempt cost the threshold + labelling kernels.  Crops and
  // recogniser then run on all M crops whatever max_crops is; when the caller's buffers are too small the results stay in
  // HBM, KOCR_ECAPACITY reports the true counts, and kocr_pipeline_results copies them into larger buffers: one detector
  // forward, one recogniser pass, always.
  PPDeviceOut dv;
  int d_cap = cap;
  int rc_pp = postproc_get_boxes(ctx, d_heat, N, h2, w2, detection_threshold, text_threshold, link_threshold,
                                 size_threshold, d_boxes, d_cap, counts, nullptr, &dv);
  if (rc_pp == KOCR_ECAPACITY) {
    int need = 0;
    for (int k = 0; k < N; ++k) need = std::max(need, (int)counts[k]);
    if (need <= d_cap) return rc_pp;  // the other capacity error (dilation canvases beyond 2^31 pixels): not a matter of cap
    d_cap = need;
    Staging bx{ctx, ctx->bx, "kocr_pipeline"};
    KOCR_TRY(bx.reserve(0, {}, {(size_t)N * d_cap * 8 * sizeof(float)}));
    KOCR_TRY(bx.scratch((size_t)N * d_cap * 8 * sizeof(float), d_boxes));
    rc_pp = postproc_get_boxes(ctx, d_heat, N, h2, w2, detection_threshold, text_threshold, link_threshold, size_threshold,
                               d_boxes, d_cap, counts, nullptr, &dv);
  }
  KOCR_TRY(rc_pp);
  KOCR_TRY(chars_resident(ctx, "kocr_pipeline", d_heat, N, h2, w2, d_boxes, d_cap, counts));
  long M = 0;
  for (int k = 0; k < N; ++k) M += counts[k];
  if (n_crops) *n_crops = (int32_t)M;
  const bool host_fits = d_cap == cap && labels && M <= max_crops;
  if (d_cap == cap) KOCR_HIP(ctx, hipMemcpyAsync(boxes, d_boxes, box_b, hipMemcpyDeviceToHost, ctx->stream));
  int host_flags[5] = {0, 0, 0, 0, 0};  // totals[0..3] of the post-processing, warp status
  auto finish = [&]() -> int {
    KOCR_HIP(ctx, hipMemcpyAsync(host_flags, dv.d_totals, 16, hipMemcpyDeviceToHost, ctx->stream));
    KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (host_flags[2] > 0)
      KOCR_FAIL(ctx, KOCR_EEMPTYCONTOUR, "kocr_pipeline: empty contour list (IndexError at detection.py:272)");
    if (host_flags[4] == 1) KOCR_FAIL(ctx, KOCR_EZERODIV, "kocr_pipeline: box with zero width or height (tools.py:95)");
    if (host_flags[4] != 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_pipeline: singular perspective transform");
    return KOCR_OK;
  };
  if (M == 0) {
    KOCR_TRY(finish());
    ctx->last_pl = {d_boxes, dv.d_counts, nullptr, N, cap, 0, true};
    ctx->keep_det_scores(dv.d_scores, N, d_cap);
    ctx->keep_rec_scores(nullptr, nullptr, 0, crnn_label_width(ctx));
    ctx->keep_beams(nullptr, nullptr, 0, crnn_label_width(ctx));
    ctx->keep_lexicon(nullptr, nullptr, 0);
    return KOCR_OK;
  }
  if (!labels && d_cap == cap) {
    KOCR_TRY(finish());  // an empty contour list (the reference's IndexError) takes precedence over the capacity error
    KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_pipeline: more crops than max_crops");
  }
  // ---- crops: homographies on the device (warp.hip), no host round trip ----
  const int LW = crnn_label_width(ctx);
  const size_t crop_b = (size_t)M * CRNN_CROP_PIXELS * sizeof(float), lab_b = (size_t)M * LW * sizeof(int32_t);
  const size_t pb = (size_t)M * sizeof(WarpParam);
  const bool scores = ctx->scores_on;
  const size_t lw_b = scores ? (size_t)M * sizeof(float) : 0, ch_b = lw_b * LW;
  const int BW = ctx->beam_width, BK = ctx->beam_top_paths;
  const size_t bl_b = BW ? (size_t)M * BK * LW * sizeof(int32_t) : 0, bv_b = BW ? (size_t)M * BK * sizeof(float) : 0;
  const int LK = ctx->lex_top;
  const size_t li_b = LK ? (size_t)M * LK * sizeof(int32_t) : 0, lv_b = LK ? (size_t)M * LK * sizeof(float) : 0;
  KOCR_TRY(io.reserve(0, {}, {pb, crop_b, lab_b, 256, lw_b, ch_b, bl_b, bv_b, li_b, lv_b}));
  WarpParam* d_prm;
  float* d_crops;
  int32_t* d_lab;
  int* d_status;
  CrnnScores sc{nullptr, nullptr};
  KOCR_TRY(io.scratch(pb, d_prm));
  KOCR_TRY(io.scratch(crop_b, d_crops));
  KOCR_TRY(io.scratch(lab_b, d_lab));
  KOCR_TRY(io.scratch(256, d_status));
  if (scores) {
    KOCR_TRY(io.scratch(lw_b, sc.d_logw));
    KOCR_TRY(io.scratch(ch_b, sc.d_chars));
  }
  CrnnBeam bm{BW, BK, nullptr, nullptr};
  if (BW) {
    KOCR_TRY(io.scratch(bl_b, bm.d_labels));
    KOCR_TRY(io.scratch(bv_b, bm.d_logp));
  }
  CrnnLexicon lx{LK, nullptr, nullptr, nullptr};
  if (LK) {
    KOCR_TRY(io.scratch(li_b, lx.d_index));
    KOCR_TRY(io.scratch(lv_b, lx.d_logp));
  }
  KOCR_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int), ctx->stream));
  KOCR_TRY(launch_warp_prepare(ctx, d_boxes, dv.d_counts, N, d_cap, CRNN_CROP_H, CRNN_CROP_W, d_prm, d_status));
  KOCR_TRY(launch_warp(ctx, d_bat, Hmax, Wmax, d_prm, (int)M, CRNN_CROP_H, CRNN_CROP_W, d_crops));
  // ---- recogniser ----
  KOCR_TRY(ctx->ws_reserve(crnn_workspace_bytes(crnn_batch(M), crnn_classes(ctx)) +
                           (LK ? lexicon_workspace_bytes(ctx, crnn_batch(M), true) : 0)));
  KOCR_TRY(crnn_batches(ctx, M, [&](long s, int nb) {
    const CrnnScores part{scores ? sc.d_logw + s : nullptr, scores ? sc.d_chars + s * LW : nullptr};
    const CrnnBeam bpart{BW, BK, BW ? bm.d_labels + s * BK * LW : nullptr, BW ? bm.d_logp + s * BK : nullptr};
    const CrnnLexicon lpart{LK, LK ? lx.d_index + s * LK : nullptr, LK ? lx.d_logp + s * LK : nullptr, nullptr};
    return crnn_forward(ctx, d_crops + s * CRNN_CROP_PIXELS, nb, d_lab + s * LW, nullptr, CRNN_DECODE, nullptr, nullptr,
                        scores ? &part : nullptr, BW ? &bpart : nullptr, LK ? &lpart : nullptr);
  }));
  if (host_fits) KOCR_HIP(ctx, hipMemcpyAsync(labels, d_lab, lab_b, hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipMemcpyAsync(&host_flags[4], d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_TRY(finish());
  ctx->last_pl = {d_boxes, dv.d_counts, d_lab, N, d_cap, (int)M, true};
  ctx->keep_det_scores(dv.d_scores, N, d_cap);
  ctx->keep_rec_scores(sc.d_logw, sc.d_chars, (int)M, LW);
  ctx->keep_beams(bm.d_labels, bm.d_logp, (int)M, LW);
  ctx->keep_lexicon(lx.d_index, lx.d_logp, (int)M);
  if (!host_fits) {
    ctx->set_err("kocr_pipeline: an image has more boxes than cap, or there are more crops than max_crops; the results are "
                 "resident -- fetch them with kocr_pipeline_results into buffers sized from counts / n_crops");
    return KOCR_ECAPACITY;
  }
  return KOCR_OK;
}

// The resident results of the last kocr_pipeline call copied into the caller's (larger) buffers: see include/kocr.h
extern "C" int kocr_pipeline_results(kocr_ctx* ctx, float* boxes, int cap, int32_t* labels, int max_crops) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_pl;
  if (!r.valid) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_pipeline_results: no kocr_pipeline result is resident (call it right after kocr_pipeline)");
  if (!boxes || cap < r.cap || (r.M > 0 && (!labels || max_crops < r.M)))
    KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_pipeline_results: buffers smaller than the resident results (cap >= " + std::to_string(r.cap) +
                                       ", max_crops >= " + std::to_string(r.M) + ")");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  // device rows are r.cap boxes apart, the caller's cap boxes
  KOCR_HIP(ctx, hipMemcpy2DAsync(boxes, (size_t)cap * 32, r.d_boxes, (size_t)r.cap * 32, (size_t)r.cap * 32, (size_t)r.N,
                                 hipMemcpyDeviceToHost, ctx->stream));
  if (r.M > 0)
    KOCR_HIP(ctx, hipMemcpyAsync(labels, r.d_labels, (size_t)r.M * crnn_label_width(ctx) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

// The resident scores (see include/kocr.h, "Scores")
static const char* const SCORES_OFF = ": the results on this context were produced with scores off (kocr_set_scores(ctx, 1) before the call)";

extern "C" int kocr_detection_scores(kocr_ctx* ctx, float* scores, int cap) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_sc;
  if (r.det_off) KOCR_FAIL(ctx, KOCR_EINVAL, std::string("kocr_detection_scores") + SCORES_OFF);
  if (!r.det_valid)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_detection_scores: no detection scores are resident (call it right after kocr_get_boxes, "
                                "kocr_detect or kocr_pipeline)");
  if (!scores || cap < r.cap)
    KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_detection_scores: buffer smaller than the resident scores (cap >= " + std::to_string(r.cap) + ")");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  // device rows are r.cap scores apart, the caller's cap scores
  KOCR_HIP(ctx, hipMemcpy2DAsync(scores, (size_t)cap * 4, r.d_det, (size_t)r.cap * 4, (size_t)r.cap * 4, (size_t)r.N,
                                 hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

extern "C" int kocr_recognition_scores(kocr_ctx* ctx, float* log_word, float* char_scores, int max_crops, int32_t* n_crops,
                                       int32_t* label_width) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_sc;
  if (r.rec_off) KOCR_FAIL(ctx, KOCR_EINVAL, std::string("kocr_recognition_scores") + SCORES_OFF);
  if (!r.rec_valid)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognition_scores: no recognition scores are resident (call it right after "
                                "kocr_recognize_boxes or kocr_pipeline)");
  if (n_crops) *n_crops = r.M;
  if (label_width) *label_width = r.lw;
  if (r.M > 0 && (!log_word || !char_scores || max_crops < r.M))
    KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_recognition_scores: buffers smaller than the resident scores (max_crops >= " +
                                       std::to_string(r.M) + ")");
  if (r.M == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  // rows of the width they were PRODUCED with, whatever kocr_crnn_label_width() says by now
  KOCR_HIP(ctx, hipMemcpyAsync(log_word, r.d_logw, (size_t)r.M * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipMemcpyAsync(char_scores, r.d_chars, (size_t)r.M * r.lw * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

// The resident beam alternatives (see include/kocr.h, "Beam search")
extern "C" int kocr_recognition_beams(kocr_ctx* ctx, int32_t* labels, float* log_prob, int max_crops, int32_t* n_crops,
                                      int32_t* label_width, int32_t* top_paths) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_beam;
  if (r.off)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognition_beams: the results on this context were produced with the beam off "
                                "(kocr_set_beam(ctx, beam_width, top_paths) before the call)");
  if (!r.valid)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognition_beams: no beam alternatives are resident (call it right after "
                                "kocr_recognize_boxes or kocr_pipeline)");
  if (n_crops) *n_crops = r.M;
  if (label_width) *label_width = r.lw;
  if (top_paths) *top_paths = r.K;
  if (r.M > 0 && (!labels || !log_prob || max_crops < r.M))
    KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_recognition_beams: buffers smaller than the resident alternatives (max_crops >= " +
                                       std::to_string(r.M) + ")");
  if (r.M == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  // rows of the width and top_paths they were PRODUCED with
  KOCR_HIP(ctx, hipMemcpyAsync(labels, r.d_labels, (size_t)r.M * r.K * r.lw * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipMemcpyAsync(log_prob, r.d_logp, (size_t)r.M * r.K * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

// The resident lexicon matches (see include/kocr.h, "Lexicon")
extern "C" int kocr_recognition_lexicon(kocr_ctx* ctx, int32_t* index, float* log_prob, int max_crops, int32_t* n_crops,
                                        int32_t* top_words) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_lex;
  if (r.off)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognition_lexicon: the results on this context were produced with the lexicon match off "
                                "(kocr_set_lexicon_match(ctx, top_words) before the call)");
  if (!r.valid)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognition_lexicon: no lexicon matches are resident (call it right after "
                                "kocr_recognize_boxes or kocr_pipeline)");
  if (n_crops) *n_crops = r.M;
  if (top_words) *top_words = r.K;
  if (r.M > 0 && (!index || !log_prob || max_crops < r.M))
    KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_recognition_lexicon: buffers smaller than the resident matches (max_crops >= " +
                                       std::to_string(r.M) + ")");
  if (r.M == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  // rows of the top_words they were PRODUCED with
  KOCR_HIP(ctx, hipMemcpyAsync(index, r.d_index, (size_t)r.M * r.K * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipMemcpyAsync(log_prob, r.d_logp, (size_t)r.M * r.K * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

// The results of the last successful kocr_pipeline call as they lie in HBM (see include/kocr.h)
extern "C" int kocr_pipeline_device_results(kocr_ctx* ctx, const float** d_boxes, const int32_t** d_counts, const int32_t** d_labels,
                                            int32_t* N, int32_t* cap, int32_t* M) {
  if (!ctx) return KOCR_EINVAL;
  if (!ctx->last_pl.valid) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_pipeline_device_results: no kocr_pipeline result is resident (call it right after kocr_pipeline)");
  if (d_boxes) *d_boxes = ctx->last_pl.d_boxes;
  if (d_counts) *d_counts = ctx->last_pl.d_counts;
  if (d_labels) *d_labels = ctx->last_pl.d_labels;
  if (N) *N = ctx->last_pl.N;
  if (cap) *cap = ctx->last_pl.cap;
  if (M) *M = ctx->last_pl.M;
  return KOCR_OK;
}
