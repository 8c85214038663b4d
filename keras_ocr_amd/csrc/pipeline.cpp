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

// ---- orientation (include/kocr.h, "orientation") ----
// The device buffers of one oriented run over M words: what the crop stage and the recogniser produce for the 2 M
// candidate-interleaved crops, and the compact rows of the M winners that orient_select_kernel writes.
namespace {
struct OrientRun {
  WarpParam* prm;  // [2M]
  float* crops;    // [2M][31][200]
  int32_t* lab2;   // [2M][LW]
  float* logw2;    // [2M]
  float* chars2;   // [2M][LW]
  int32_t* turns2; // [2M]
  float* quads2;   // [2M][8]
  int32_t* lab;    // [M][LW]
  float* logw;     // [M]
  float* chars;    // [M][LW]
  int32_t* turn;   // [M]
  float* quad;     // [M][8]
  float* pair;     // [M][2]
};

std::vector<size_t> orient_sizes(long M, int LW) {
  const size_t m = (size_t)M, f = sizeof(float);
  return {2 * m * sizeof(WarpParam), 2 * m * CRNN_CROP_PIXELS * f, 2 * m * LW * sizeof(int32_t), 2 * m * f, 2 * m * LW * f,
          2 * m * sizeof(int32_t), 2 * m * 8 * f, m * LW * sizeof(int32_t), m * f, m * LW * f, m * sizeof(int32_t), m * 8 * f, 2 * m * f};
}

// the bytes orient_alloc takes from an arena, as Staging::reserve counts one buffer
size_t orient_bytes(long M, int LW) {
  size_t total = 0;
  for (size_t b : orient_sizes(M, LW)) total += b + 256;
  return total;
}

int orient_alloc(Staging& st, long M, int LW, OrientRun& r) {
  const std::vector<size_t> b = orient_sizes(M, LW);
  KOCR_TRY(st.scratch(b[0], r.prm));
  KOCR_TRY(st.scratch(b[1], r.crops));
  KOCR_TRY(st.scratch(b[2], r.lab2));
  KOCR_TRY(st.scratch(b[3], r.logw2));
  KOCR_TRY(st.scratch(b[4], r.chars2));
  KOCR_TRY(st.scratch(b[5], r.turns2));
  KOCR_TRY(st.scratch(b[6], r.quads2));
  KOCR_TRY(st.scratch(b[7], r.lab));
  KOCR_TRY(st.scratch(b[8], r.logw));
  KOCR_TRY(st.scratch(b[9], r.chars));
  KOCR_TRY(st.scratch(b[10], r.turn));
  KOCR_TRY(st.scratch(b[11], r.quad));
  KOCR_TRY(st.scratch(b[12], r.pair));
  return KOCR_OK;
}

// Warp, recogniser with scores, choice: r.prm / r.turns2 / r.quads2 are set up, the winners' rows are written.
int orient_run(kocr_ctx* ctx, const uint8_t* d_img, int H, int W, long M, int LW, const OrientRun& r) {
  KOCR_TRY(launch_warp(ctx, d_img, H, W, r.prm, (int)(2 * M), CRNN_CROP_H, CRNN_CROP_W, r.crops));
  KOCR_TRY(ctx->ws_reserve(crnn_workspace_bytes(crnn_batch(2 * M), crnn_classes(ctx))));
  KOCR_TRY(crnn_batches(ctx, 2 * M, [&](long s, int nb) {
    const CrnnScores part{r.logw2 + s, r.chars2 + s * LW};
    return crnn_forward(ctx, r.crops + s * CRNN_CROP_PIXELS, nb, r.lab2 + s * LW, nullptr, CRNN_DECODE, nullptr, nullptr, &part);
  }));
  return launch_orient_select(ctx, r.lab2, r.logw2, r.chars2, r.turns2, r.quads2, M, LW, r.lab, r.logw, r.chars, r.turn, r.quad, r.pair);
}

// what an oriented run leaves resident: the winners' scores (with scores on), no alternatives, the orientation
void orient_keep(kocr_ctx* ctx, const OrientRun& r, long M, int LW) {
  ctx->keep_rec_scores(r.logw, r.chars, (int)M, LW);
  ctx->keep_beams(nullptr, nullptr, 0, LW);
  ctx->keep_lexicon(nullptr, nullptr, 0);
  ctx->keep_orientation(r.turn, r.quad, r.pair, (int)M);
}

const char* orient_refusal(const kocr_ctx* ctx, bool with_chars) {
  if (ctx->beam_width) return ": orientation cannot be combined with a beam (kocr_set_beam)";
  if (ctx->lex_top) return ": orientation cannot be combined with a lexicon match (kocr_set_lexicon_match)";
  if (with_chars && ctx->chars_on) return ": orientation cannot be combined with character boxes (kocr_set_char_boxes)";
  return nullptr;
}

bool orient_args_ok(int mode, double tall_ratio, bool allow_off) {
  if (mode != KOCR_ORIENT_FLIP && mode != KOCR_ORIENT_ANY && !(allow_off && mode == KOCR_ORIENT_OFF)) return false;
  return std::isfinite(tall_ratio) && tall_ratio > 0;
}

// kocr_recognize_boxes with the switch on: the set-up on the host with the function the device runs (as prepare_box_warps)
int recognize_boxes_oriented(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes, const int32_t* counts,
                             int32_t* labels, int on_device) {
  const char* fn = "kocr_recognize_boxes";
  if (const char* why = orient_refusal(ctx, false)) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + why);
  long M = 0;
  for (int i = 0; i < N; ++i) {
    if (counts[i] < 0) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": negative count");
    M += counts[i];
  }
  if (M == 0) return KOCR_OK;
  if (!boxes || !labels) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": null buffer");
  std::vector<WarpParam> prm((size_t)2 * M);
  std::vector<int32_t> turns((size_t)2 * M);
  std::vector<float> quads((size_t)16 * M);
  long m = 0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < counts[i]; ++j, ++m)
      for (int c = 0; c < 2; ++c) {
        const size_t k = 2 * (size_t)m + c;
        int t = 0;
        const int rc = warp_prepare_turned(boxes + m * 8, ctx->orient_mode, ctx->orient_ratio, c, CRNN_CROP_H, CRNN_CROP_W, &prm[k], &t,
                                           &quads[k * 8]);
        if (rc == 1) KOCR_FAIL(ctx, KOCR_EZERODIV, std::string(fn) + ": box with zero width or height (ZeroDivisionError at tools.py:95)");
        if (rc != 0) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": singular perspective transform");
        prm[k].img = i;
        turns[k] = t;
      }
  ctx->invalidate_results();
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int LW = crnn_label_width(ctx);
  const size_t ib = (size_t)N * H * W * 3;
  Staging st{ctx, ctx->io, fn, on_device != 0};
  KOCR_TRY(st.reserve(0, {ib}, {orient_bytes(M, LW)}));
  OrientRun r;
  const uint8_t* d_img;
  KOCR_TRY(orient_alloc(st, M, LW, r));
  KOCR_TRY(st.in(img_rgb, ib, d_img));
  KOCR_TRY(st.put(r.prm, (const WarpParam*)prm.data(), prm.size() * sizeof(WarpParam)));
  KOCR_TRY(st.put(r.turns2, (const int32_t*)turns.data(), turns.size() * sizeof(int32_t)));
  KOCR_TRY(st.put(r.quads2, (const float*)quads.data(), quads.size() * sizeof(float)));
  KOCR_TRY(orient_run(ctx, d_img, H, W, M, LW, r));
  KOCR_TRY(st.download(labels, (const int32_t*)r.lab, (size_t)M * LW * sizeof(int32_t)));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // also: the host vectors' copies are done
  orient_keep(ctx, r, M, LW);
  return KOCR_OK;
}
}  // namespace

// Recognizer.recognize_from_boxes' device half in one call: crops are warped and recognised without
// leaving HBM.  All N images share one size; boxes/counts/labels are HOST buffers.
extern "C" int kocr_recognize_boxes(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                    const int32_t* counts, int32_t* labels, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || (N > 0 && (!img_rgb || !counts))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognize_boxes: null buffer");
  const int C = crnn_classes(ctx);
  if (C == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_recognize_boxes: call kocr_load_crnn first");
  if (ctx->orient_mode != KOCR_ORIENT_OFF) return recognize_boxes_oriented(ctx, img_rgb, N, H, W, boxes, counts, labels, on_device);
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
  ctx->keep_orientation(nullptr, nullptr, nullptr, 0);
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
  const bool oriented = ctx->orient_mode != KOCR_ORIENT_OFF;
  if (oriented)
    if (const char* why = orient_refusal(ctx, true)) KOCR_FAIL(ctx, KOCR_EINVAL, std::string("kocr_pipeline") + why);
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
    ctx->keep_orientation(nullptr, nullptr, nullptr, 0);
    return KOCR_OK;
  }
  if (!labels && d_cap == cap) {
    KOCR_TRY(finish());  // an empty contour list (the reference's IndexError) takes precedence over the capacity error
    KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_pipeline: more crops than max_crops");
  }
  const int LW = crnn_label_width(ctx);
  const char* const over_capacity =
      "kocr_pipeline: an image has more boxes than cap, or there are more crops than max_crops; the results are "
      "resident -- fetch them with kocr_pipeline_results into buffers sized from counts / n_crops";
  if (oriented) {
    // ---- both orientations of every box: turned set-up on the device, 2 M crops, recogniser with scores, choice ----
    OrientRun r;
    int* d_status;
    KOCR_TRY(io.reserve(0, {}, {orient_bytes(M, LW), 256}));
    KOCR_TRY(orient_alloc(io, M, LW, r));
    KOCR_TRY(io.scratch(256, d_status));
    KOCR_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int), ctx->stream));
    KOCR_TRY(launch_warp_prepare_turned(ctx, d_boxes, dv.d_counts, N, d_cap, ctx->orient_mode, ctx->orient_ratio, CRNN_CROP_H,
                                        CRNN_CROP_W, r.prm, r.turns2, r.quads2, d_status));
    KOCR_TRY(orient_run(ctx, d_bat, Hmax, Wmax, M, LW, r));
    if (host_fits)
      KOCR_HIP(ctx, hipMemcpyAsync(labels, r.lab, (size_t)M * LW * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    KOCR_HIP(ctx, hipMemcpyAsync(&host_flags[4], d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KOCR_TRY(finish());
    ctx->last_pl = {d_boxes, dv.d_counts, r.lab, N, d_cap, (int)M, true};
    ctx->keep_det_scores(dv.d_scores, N, d_cap);
    orient_keep(ctx, r, M, LW);
    if (!host_fits) {
      ctx->set_err(over_capacity);
      return KOCR_ECAPACITY;
    }
    return KOCR_OK;
  }
  // ---- crops: homographies on the device (warp.hip), no host round trip ----
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
  ctx->keep_orientation(nullptr, nullptr, nullptr, 0);
  if (!host_fits) {
    ctx->set_err(over_capacity);
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

// ---- orientation (see include/kocr.h, "orientation") ----
extern "C" int kocr_set_orientation(kocr_ctx* ctx, int mode, double tall_ratio) {
  if (!ctx) return KOCR_EINVAL;
  if (!orient_args_ok(mode, tall_ratio, true))
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_orientation: mode must be 0 (off), 1 (flip) or 2 (any) and tall_ratio finite and positive");
  if (mode != KOCR_ORIENT_OFF)
    if (const char* why = orient_refusal(ctx, true)) KOCR_FAIL(ctx, KOCR_EINVAL, std::string("kocr_set_orientation") + why);
  ctx->orient_mode = mode;
  ctx->orient_ratio = tall_ratio;
  return KOCR_OK;
}

extern "C" int kocr_get_orientation(const kocr_ctx* ctx, int* mode, double* tall_ratio) {
  if (!ctx) return KOCR_EINVAL;
  if (mode) *mode = ctx->orient_mode;
  if (tall_ratio) *tall_ratio = ctx->orient_ratio;
  return KOCR_OK;
}

extern "C" int kocr_recognition_orientation(kocr_ctx* ctx, int32_t* turns, float* quads, float* log_words, int max_crops,
                                            int32_t* n_crops) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_or;
  if (r.off)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognition_orientation: the results on this context were produced with orientation off "
                                "(kocr_set_orientation(ctx, mode, tall_ratio) before the call)");
  if (!r.valid)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognition_orientation: no orientation is resident (call it right after "
                                "kocr_recognize_boxes or kocr_pipeline)");
  if (n_crops) *n_crops = r.M;
  if (r.M > 0 && (!turns || !quads || !log_words || max_crops < r.M))
    KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_recognition_orientation: buffers smaller than the resident orientation (max_crops >= " +
                                       std::to_string(r.M) + ")");
  if (r.M == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  KOCR_HIP(ctx, hipMemcpyAsync(turns, r.d_turns, (size_t)r.M * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipMemcpyAsync(quads, r.d_quads, (size_t)r.M * 8 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipMemcpyAsync(log_words, r.d_pairs, (size_t)r.M * 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

// The turned crop stage alone: the boxes go into the [N][cap] layout getBoxes leaves (cap = the largest count), the set-up
// runs on the device as in kocr_pipeline
extern "C" int kocr_warp_crops_turned(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                      const int32_t* counts, int mode, double tall_ratio, int target_h, int target_w, float* crops,
                                      int32_t* turns, float* quads) {
  if (!ctx) return KOCR_EINVAL;
  const char* fn = "kocr_warp_crops_turned";
  if (N < 0 || target_h <= 0 || target_w <= 0 || (N > 0 && (!img_rgb || !counts))) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": bad argument");
  if (!orient_args_ok(mode, tall_ratio, false))
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": mode must be 1 (flip) or 2 (any) and tall_ratio finite and positive");
  long M = 0;
  int cap = 0;
  for (int i = 0; i < N; ++i) {
    if (counts[i] < 0) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": negative count");
    M += counts[i];
    cap = std::max(cap, (int)counts[i]);
  }
  if (M == 0) return KOCR_OK;
  if (!boxes || !crops || !turns || !quads) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": null buffer");
  std::vector<float> slots((size_t)N * cap * 8, 0.f);
  long m = 0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < counts[i]; ++j, ++m) std::memcpy(&slots[((size_t)i * cap + j) * 8], boxes + m * 8, 8 * sizeof(float));
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ib = (size_t)N * H * W * 3, cb = (size_t)2 * M * target_h * target_w * sizeof(float);
  const size_t sb = slots.size() * sizeof(float), nb = (size_t)N * sizeof(int32_t), pb = (size_t)2 * M * sizeof(WarpParam);
  const size_t tb = (size_t)2 * M * sizeof(int32_t), qb = (size_t)2 * M * 8 * sizeof(float);
  Staging st{ctx, ctx->io, fn};
  KOCR_TRY(st.reserve(0, {ib, cb, sb, nb, pb, tb, qb, 256}));
  const uint8_t* d_img;
  const float* d_slots;
  const int32_t* d_counts;
  float *d_crops, *d_quads;
  int32_t* d_turns;
  WarpParam* d_prm;
  int* d_status;
  KOCR_TRY(st.in(img_rgb, ib, d_img));
  KOCR_TRY(st.upload((const float*)slots.data(), sb, d_slots));
  KOCR_TRY(st.in(counts, nb, d_counts));
  KOCR_TRY(st.scratch(cb, d_crops));
  KOCR_TRY(st.scratch(pb, d_prm));
  KOCR_TRY(st.scratch(tb, d_turns));
  KOCR_TRY(st.scratch(qb, d_quads));
  KOCR_TRY(st.scratch(256, d_status));
  KOCR_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int), ctx->stream));
  KOCR_TRY(launch_warp_prepare_turned(ctx, d_slots, d_counts, N, cap, mode, tall_ratio, target_h, target_w, d_prm, d_turns, d_quads,
                                      d_status));
  KOCR_TRY(launch_warp(ctx, d_img, H, W, d_prm, (int)(2 * M), target_h, target_w, d_crops));
  int status = 0;
  KOCR_TRY(st.download(crops, (const float*)d_crops, cb));
  KOCR_TRY(st.download(turns, (const int32_t*)d_turns, tb));
  KOCR_TRY(st.download(quads, (const float*)d_quads, qb));
  KOCR_TRY(st.download(&status, (const int*)d_status, sizeof(int)));
  KOCR_TRY(st.finish());
  if (status == 1) KOCR_FAIL(ctx, KOCR_EZERODIV, std::string(fn) + ": box with zero width or height (ZeroDivisionError at tools.py:95)");
  if (status != 0) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": singular perspective transform");
  return KOCR_OK;
}

// The choice alone, on the caller's rows
extern "C" int kocr_orient_select(kocr_ctx* ctx, int M, int L, const int32_t* labels, const float* log_word, const float* char_scores,
                                  const int32_t* turns, const float* quads, int32_t* out_labels, float* out_log_word,
                                  float* out_char_scores, int32_t* out_turns, float* out_quads, float* out_log_words) {
  if (!ctx) return KOCR_EINVAL;
  const char* fn = "kocr_orient_select";
  if (M < 0 || L < 1) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": bad sizes");
  if (M == 0) return KOCR_OK;
  if (!labels || !log_word || !char_scores || !turns || !quads || !out_labels || !out_log_word || !out_char_scores || !out_turns ||
      !out_quads || !out_log_words)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": null buffer");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t m = (size_t)M, f = sizeof(float), i4 = sizeof(int32_t);
  Staging st{ctx, ctx->io, fn};
  KOCR_TRY(st.reserve(0, {2 * m * L * i4, 2 * m * f, 2 * m * L * f, 2 * m * i4, 16 * m * f, m * L * i4, m * f, m * L * f, m * i4, 8 * m * f,
                          2 * m * f}));
  const int32_t *d_lab, *d_turns;
  const float *d_logw, *d_chars, *d_quads;
  int32_t *o_lab, *o_turn;
  float *o_logw, *o_chars, *o_quad, *o_pair;
  KOCR_TRY(st.in(labels, 2 * m * L * i4, d_lab));
  KOCR_TRY(st.in(log_word, 2 * m * f, d_logw));
  KOCR_TRY(st.in(char_scores, 2 * m * L * f, d_chars));
  KOCR_TRY(st.in(turns, 2 * m * i4, d_turns));
  KOCR_TRY(st.in(quads, 16 * m * f, d_quads));
  KOCR_TRY(st.out(out_labels, m * L * i4, o_lab));
  KOCR_TRY(st.out(out_log_word, m * f, o_logw));
  KOCR_TRY(st.out(out_char_scores, m * L * f, o_chars));
  KOCR_TRY(st.out(out_turns, m * i4, o_turn));
  KOCR_TRY(st.out(out_quads, 8 * m * f, o_quad));
  KOCR_TRY(st.out(out_log_words, 2 * m * f, o_pair));
  KOCR_TRY(launch_orient_select(ctx, d_lab, d_logw, d_chars, d_turns, d_quads, M, L, o_lab, o_logw, o_chars, o_turn, o_quad, o_pair));
  KOCR_TRY(st.back(out_labels, o_lab, m * L * i4));
  KOCR_TRY(st.back(out_log_word, o_logw, m * f));
  KOCR_TRY(st.back(out_char_scores, o_chars, m * L * f));
  KOCR_TRY(st.back(out_turns, o_turn, m * i4));
  KOCR_TRY(st.back(out_quads, o_quad, 8 * m * f));
  KOCR_TRY(st.back(out_log_words, o_pair, 2 * m * f));
  return st.finish();
}
