// pipeline.cpp — the fused device path of Pipeline.recognize (pipeline.py:28-75):
//   resize_image + pad (pipeline.py:44-57)  ->  Detector.detect (:62; detection.py:745-785)
//   ->  Recognizer.recognize_from_boxes (:63-65; recognition.py:491-537).
// Everything stays resident in HBM between the stages; the host sees only the per-image box
// counts (a few bytes, needed to size the crop batch), the boxes and the decoded label rows.
// kocr_pipeline_tiled (at the end of the file) is the same path with the detector run on overlapping tiles of the page.
#include "abi.h"

extern "C" int kocr_resize_pad(kocr_ctx* ctx, const uint8_t* src, int n, int sh, int sw, int dh, int dw, int Hmax,
                               int Wmax, int cval, uint8_t* dst, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (n < 0 || (n > 0 && (!src || !dst))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_resize_pad: null buffer");
  if (n == 0) return KOCR_OK;
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
  if (!craft_loaded(ctx)) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_detect: call kocr_load_craft first");
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
  KOCR_TRY(ctx->ws_reserve(craft_workspace_bytes(craft_micro_batch(micro_batch, N, H, W), H, W)));
  KOCR_TRY(craft_batches(ctx, micro_batch, N, H, W, [&](int s, int nb) {
    return craft_forward(ctx, d_in + (size_t)s * in_img, dtype, nb, H, W, d_heat + (size_t)s * h2 * w2 * 2);
  }));
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
// The device buffers of one oriented run over M words: what the crop stage produces for the 2 M candidate-interleaved crops,
// the recogniser stage over them (its label rows and scores are the candidates'), and the compact rows of the M winners.
namespace {
struct OrientRun {
  RecStage rec;
  OrientWinners won;
  WarpParam* prm = nullptr;   // [2M]
  float* crops = nullptr;     // [2M][31][200]
  int32_t* turns2 = nullptr;  // [2M]
  float* quads2 = nullptr;    // [2M][8]
  OrientRun(kocr_ctx* ctx, long M) : rec(ctx, 2 * M, true) { won.words = M; }
  // a per-box list of character sets (device, [M]): both candidates of box m are crops 2 m and 2 m + 1
  void set_charsets(kocr_ctx* ctx, const int32_t* d_set_of) { rec.req.cm = ctx->charmask(d_set_of, 1); }
  template <class F> int each(F f) {
    const size_t m = (size_t)won.words, lw = (size_t)rec.LW, i4 = sizeof(int32_t), f4 = sizeof(float);
    KOCR_TRY(f(prm, 2 * m * sizeof(WarpParam)));
    KOCR_TRY(f(crops, 2 * m * CRNN_CROP_PIXELS * f4));
    KOCR_TRY(rec.each(f));
    KOCR_TRY(f(turns2, 2 * m * i4));
    KOCR_TRY(f(quads2, 2 * m * 8 * f4));
    KOCR_TRY(f(won.lab, m * lw * i4));
    KOCR_TRY(f(won.logw, m * f4));
    KOCR_TRY(f(won.chars, m * lw * f4));
    KOCR_TRY(f(won.turn, m * i4));
    KOCR_TRY(f(won.quad, m * 8 * f4));
    return f(won.pair, 2 * m * f4);
  }
};

// Warp, recogniser with scores, choice: r.prm / r.turns2 / r.quads2 are set up, the winners' rows are written.
int orient_run(kocr_ctx* ctx, const uint8_t* d_img, int H, int W, OrientRun& r) {
  const long M = r.won.words;
  KOCR_TRY(launch_warp(ctx, d_img, H, W, r.prm, (int)(2 * M), CRNN_CROP_H, CRNN_CROP_W, r.crops));
  KOCR_TRY(r.rec.run(r.crops));
  const CrnnDecode& rq = r.rec.req;
  return launch_orient_select(ctx, rq.d_labels, rq.sc.d_logw, rq.sc.d_chars, r.turns2, r.quads2, M, r.rec.LW, r.won.lab, r.won.logw,
                              r.won.chars, r.won.turn, r.won.quad, r.won.pair);
}

const char* orient_refusal(const kocr_ctx* ctx, bool with_chars) {
  if (ctx->beam_width) return ": orientation cannot be combined with a beam (kocr_set_beam)";
  if (ctx->lex_top) return ": orientation cannot be combined with a lexicon match (kocr_set_lexicon_match)";
  if (ctx->pattern >= 0) return ": orientation cannot be combined with a pattern (kocr_set_pattern)";
  if (with_chars && ctx->chars_on) return ": orientation cannot be combined with character boxes (kocr_set_char_boxes)";
  return nullptr;
}

bool orient_args_ok(int mode, double tall_ratio, bool allow_off) {
  if (mode != KOCR_ORIENT_FLIP && mode != KOCR_ORIENT_ANY && !(allow_off && mode == KOCR_ORIENT_OFF)) return false;
  return std::isfinite(tall_ratio) && tall_ratio > 0;
}

// kocr_recognize_boxes with the switch on: the set-up on the host with the function the device runs (as prepare_box_warps)
int recognize_boxes_oriented(kocr_ctx* ctx, const char* fn, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                             const int32_t* counts, int32_t* labels, int on_device, const int32_t* set_of) {
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
        KOCR_TRY(warp_status_error(ctx, fn, rc));
        prm[k].img = i;
        turns[k] = t;
      }
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ib = (size_t)N * H * W * 3;
  OrientRun r(ctx, M);
  Staging st{ctx, ctx->io, fn, on_device != 0};
  KOCR_TRY(st.reserve(0, {ib}, {staging_bytes(r), set_of ? (size_t)M * sizeof(int32_t) : 0}));
  const uint8_t* d_img;
  KOCR_TRY(staging_take(st, r));
  KOCR_TRY(st.in(img_rgb, ib, d_img));
  if (set_of) {  // the caller's array outlives the copy: the call synchronises before it returns
    const int32_t* d_set;
    KOCR_TRY(st.upload(set_of, (size_t)M * sizeof(int32_t), d_set));
    r.set_charsets(ctx, d_set);
  }
  KOCR_TRY(st.put(r.prm, (const WarpParam*)prm.data(), prm.size() * sizeof(WarpParam)));
  KOCR_TRY(st.put(r.turns2, (const int32_t*)turns.data(), turns.size() * sizeof(int32_t)));
  KOCR_TRY(st.put(r.quads2, (const float*)quads.data(), quads.size() * sizeof(float)));
  KOCR_TRY(orient_run(ctx, d_img, H, W, r));
  KOCR_TRY(st.download(labels, (const int32_t*)r.won.lab, (size_t)M * r.rec.LW * sizeof(int32_t)));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // also: the host vectors' copies are done
  r.rec.keep(&r.won);
  return KOCR_OK;
}
}  // namespace

// Recognizer.recognize_from_boxes' device half in one call: crops are warped and recognised without
// leaving HBM.  All N images share one size; boxes/counts/labels are HOST buffers.  set_of (HOST, nullable; `fn` =
// kocr_recognize_boxes_charsets): one character set per box in place of the context's switch, checked before any launch.
// pattern_of (HOST, nullable; kocr_recognize_boxes_patterns): one pattern per box likewise.
static int recognize_boxes_call(kocr_ctx* ctx, const char* fn, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                const int32_t* counts, int32_t* labels, int on_device, const int32_t* set_of,
                                const int32_t* pattern_of = nullptr) {
  const std::string f(fn);
  if (N < 0 || (N > 0 && (!img_rgb || !counts))) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null buffer");
  if (crnn_classes(ctx) == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, f + ": call kocr_load_crnn first");
  if (set_of) {
    long n = 0;
    for (int i = 0; i < N; ++i) n += std::max<int32_t>(counts[i], 0);
    KOCR_TRY(charsets_validate(ctx, fn, set_of, n, "box"));
  }
  if (pattern_of) {
    long n = 0;
    for (int i = 0; i < N; ++i) n += std::max<int32_t>(counts[i], 0);
    KOCR_TRY(patterns_validate(ctx, fn, pattern_of, n, "box"));
  }
  if (pattern_of || ctx->pattern >= 0) KOCR_TRY(pattern_refusal(ctx, fn));
  if (ctx->orient_mode != KOCR_ORIENT_OFF)
    return recognize_boxes_oriented(ctx, fn, img_rgb, N, H, W, boxes, counts, labels, on_device, set_of);
  std::vector<WarpParam> prm;
  const long M = prepare_box_warps(ctx, fn, N, boxes, counts, labels, CRNN_CROP_H, CRNN_CROP_W, prm);
  if (M <= 0) return (int)M;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ib = (size_t)N * H * W * 3, crop_b = (size_t)M * CRNN_CROP_PIXELS * sizeof(float), pb = (size_t)M * sizeof(WarpParam);
  RecStage rec(ctx, M);
  if (pattern_of) rec.set_patterns(pattern_of, nullptr);
  Staging st{ctx, ctx->io, fn, on_device != 0};
  KOCR_TRY(st.reserve(0, {ib}, {pb, crop_b, rec.bytes(), set_of ? (size_t)M * sizeof(int32_t) : 0,
                                pattern_of ? (size_t)M * sizeof(int32_t) : 0}));
  WarpParam* d_prm;
  float* d_crops;
  const uint8_t* d_img;
  KOCR_TRY(st.scratch(pb, d_prm));
  KOCR_TRY(st.scratch(crop_b, d_crops));
  KOCR_TRY(rec.take(st));
  KOCR_TRY(st.in(img_rgb, ib, d_img));
  KOCR_TRY(st.put(d_prm, (const WarpParam*)prm.data(), pb));
  if (set_of) {  // the caller's array outlives the copy: the call synchronises before it returns
    const int32_t* d_set;
    KOCR_TRY(st.upload(set_of, (size_t)M * sizeof(int32_t), d_set));
    rec.req.cm = ctx->charmask(d_set, 0);
  }
  if (pattern_of) {
    const int32_t* d_of;
    KOCR_TRY(st.upload(pattern_of, (size_t)M * sizeof(int32_t), d_of));
    rec.set_patterns(pattern_of, d_of);
  }
  KOCR_TRY(launch_warp(ctx, d_img, H, W, d_prm, (int)M, CRNN_CROP_H, CRNN_CROP_W, d_crops));
  KOCR_TRY(rec.run(d_crops));
  KOCR_TRY(st.download(labels, (const int32_t*)rec.req.d_labels, (size_t)M * rec.LW * sizeof(int32_t)));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  rec.keep();
  return KOCR_OK;
}

extern "C" int kocr_recognize_boxes(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                    const int32_t* counts, int32_t* labels, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  return recognize_boxes_call(ctx, "kocr_recognize_boxes", img_rgb, N, H, W, boxes, counts, labels, on_device, nullptr);
}

extern "C" int kocr_recognize_boxes_charsets(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                             const int32_t* counts, int32_t* labels, int on_device, const int32_t* set_of) {
  if (!ctx) return KOCR_EINVAL;
  if (N > 0 && !set_of) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognize_boxes_charsets: null buffer");
  return recognize_boxes_call(ctx, "kocr_recognize_boxes_charsets", img_rgb, N, H, W, boxes, counts, labels, on_device, set_of);
}

extern "C" int kocr_recognize_boxes_patterns(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                                             const int32_t* counts, int32_t* labels, int on_device, const int32_t* pattern_of) {
  if (!ctx) return KOCR_EINVAL;
  if (N > 0 && !pattern_of) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognize_boxes_patterns: null buffer");
  if (ctx->patterns.P == 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_recognize_boxes_patterns: no patterns are loaded (kocr_set_patterns first)");
  return recognize_boxes_call(ctx, "kocr_recognize_boxes_patterns", img_rgb, N, H, W, boxes, counts, labels, on_device, nullptr, pattern_of);
}

namespace {
// What kocr_pipeline and kocr_pipeline_tiled share.  The caller's side of both: the images with their sizes before and after
// tools.resize_image, the thresholds of getBoxes, the buffers the results go to.
struct PipelineCall {
  const char* fn;
  int N;
  const uint8_t* const* imgs;
  const int32_t *hs, *ws, *dhs, *dws;
  float detection_threshold, text_threshold, link_threshold;
  int size_threshold, micro_batch;
  float* boxes;
  int32_t* counts;
  int cap;
  int32_t* labels;
  int max_crops;
  int32_t* n_crops;
  bool on_device;
};

// The checks ahead of any work; *go = false: the call is over (nothing to do, rc KOCR_OK)
int pipeline_begin(kocr_ctx* ctx, const PipelineCall& c, bool sizes_ok, bool* go) {
  const std::string f(c.fn);
  *go = false;
  if (c.n_crops) *c.n_crops = 0;
  if (c.N < 0 || (c.N > 0 && (!c.imgs || !c.hs || !c.ws || !c.dhs || !c.dws || !c.boxes || !c.counts)))
    KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null buffer");
  ctx->invalidate_results();  // also for the returns before the first arena is sized: N == 0 replaces the results by none
  if (c.N == 0) return KOCR_OK;
  if (!craft_loaded(ctx)) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, f + ": call kocr_load_craft first");
  if (crnn_classes(ctx) == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, f + ": call kocr_load_crnn first");
  if (!sizes_ok || c.cap <= 0) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": bad sizes");
  if (ctx->orient_mode != KOCR_ORIENT_OFF)
    if (const char* why = orient_refusal(ctx, true)) KOCR_FAIL(ctx, KOCR_EINVAL, f + why);
  if (ctx->pattern >= 0) KOCR_TRY(pattern_refusal(ctx, c.fn));
  *go = true;
  return KOCR_OK;
}

// resize + pad into d_bat [N][Hmax][Wmax][3], runs of identically-shaped contiguous images in one launch
int pipeline_resize(kocr_ctx* ctx, const PipelineCall& c, int Hmax, int Wmax, uint8_t* d_bat) {
  Staging io{ctx, ctx->io, c.fn, c.on_device};
  const uint8_t* const* imgs = c.imgs;
  const int32_t *hs = c.hs, *ws = c.ws, *dhs = c.dhs, *dws = c.dws;
  int i = 0;
  while (i < c.N) {
    int j = i + 1;
    while (j < c.N && hs[j] == hs[i] && ws[j] == ws[i] && dhs[j] == dhs[i] && dws[j] == dws[i] &&
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
  return KOCR_OK;
}

int pipeline_tail(kocr_ctx* ctx, const PipelineCall& c, const uint8_t* d_bat, int Hmax, int Wmax, const float* d_heat, float* d_boxes);
}  // namespace

extern "C" int kocr_pipeline(kocr_ctx* ctx, int N, const uint8_t* const* imgs, const int32_t* hs, const int32_t* ws,
                             const int32_t* dhs, const int32_t* dws, int Hmax, int Wmax, float detection_threshold,
                             float text_threshold, float link_threshold, int size_threshold, int micro_batch,
                             float* boxes, int32_t* counts, int cap, int32_t* labels, int max_crops,
                             int32_t* n_crops, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  const PipelineCall c{"kocr_pipeline", N, imgs, hs, ws, dhs, dws, detection_threshold, text_threshold, link_threshold, size_threshold,
                       micro_batch, boxes, counts, cap, labels, max_crops, n_crops, on_device != 0};
  bool go;
  KOCR_TRY(pipeline_begin(ctx, c, Hmax >= 16 && Wmax >= 16, &go));
  if (!go) return KOCR_OK;
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
  KOCR_TRY(pipeline_resize(ctx, c, Hmax, Wmax, d_bat));
  // ---- detector forward (micro-batched) ----
  KOCR_TRY(ctx->ws_reserve(craft_workspace_bytes(craft_micro_batch(micro_batch, N, Hmax, Wmax), Hmax, Wmax)));
  KOCR_TRY(craft_batches(ctx, micro_batch, N, Hmax, Wmax, [&](int s, int nb) {
    return craft_forward(ctx, d_bat + (size_t)s * Hmax * Wmax * 3, KOCR_U8, nb, Hmax, Wmax, d_heat + (size_t)s * h2 * w2 * 2);
  }));
  return pipeline_tail(ctx, c, d_bat, Hmax, Wmax, d_heat, d_boxes);
}

namespace {
// The end that kocr_pipeline and kocr_pipeline_tiled share: everything behind the heat-maps d_heat [N][Hmax / 2][Wmax / 2][2]
// of the batch d_bat [N][Hmax][Wmax][3]; d_boxes [N][cap][4][2] lies in the pl arena beside them.
int pipeline_tail(kocr_ctx* ctx, const PipelineCall& c, const uint8_t* d_bat, int Hmax, int Wmax, const float* d_heat, float* d_boxes) {
  const std::string fn(c.fn);
  const int N = c.N, cap = c.cap, max_crops = c.max_crops, h2 = Hmax / 2, w2 = Wmax / 2;
  const float detection_threshold = c.detection_threshold, text_threshold = c.text_threshold, link_threshold = c.link_threshold;
  const int size_threshold = c.size_threshold;
  float* const boxes = c.boxes;
  int32_t *const counts = c.counts, *const labels = c.labels, *const n_crops = c.n_crops;
  const size_t box_b = (size_t)N * cap * 8 * sizeof(float);
  const bool oriented = ctx->orient_mode != KOCR_ORIENT_OFF;
  Staging io{ctx, ctx->io, c.fn, c.on_device};
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
    Staging bx{ctx, ctx->bx, c.fn};
    KOCR_TRY(bx.reserve(0, {}, {(size_t)N * d_cap * 8 * sizeof(float)}));
    KOCR_TRY(bx.scratch((size_t)N * d_cap * 8 * sizeof(float), d_boxes));
    rc_pp = postproc_get_boxes(ctx, d_heat, N, h2, w2, detection_threshold, text_threshold, link_threshold, size_threshold,
                               d_boxes, d_cap, counts, nullptr, &dv);
  }
  KOCR_TRY(rc_pp);
  KOCR_TRY(chars_resident(ctx, c.fn, d_heat, N, h2, w2, d_boxes, d_cap, counts));
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
      KOCR_FAIL(ctx, KOCR_EEMPTYCONTOUR, fn + ": empty contour list (IndexError at detection.py:272)");
    return warp_status_error(ctx, c.fn, host_flags[4], "tools.py:95");
  };
  if (M == 0) {
    KOCR_TRY(finish());
    ctx->last_pl = {d_boxes, dv.d_counts, nullptr, N, cap, 0, crnn_label_width(ctx), Resident::VALID};
    ctx->keep_det_scores(dv.d_scores, N, d_cap);
    RecStage(ctx, 0).keep();
    return KOCR_OK;
  }
  if (!labels && d_cap == cap) {
    KOCR_TRY(finish());  // an empty contour list (the reference's IndexError) takes precedence over the capacity error
    KOCR_FAIL(ctx, KOCR_ECAPACITY, fn + ": more crops than max_crops");
  }
  // ---- the end of both routes: the label rows `d_lab` of `rec` (an oriented run's: of its winners) to the caller, the
  // status words to the host, what stays resident ----
  int* d_status;
  auto finish_crops = [&](const RecStage& rec, const OrientWinners* won) -> int {
    const int32_t* d_lab = won ? won->lab : rec.req.d_labels;
    if (host_fits)
      KOCR_HIP(ctx, hipMemcpyAsync(labels, d_lab, (size_t)M * rec.LW * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    KOCR_HIP(ctx, hipMemcpyAsync(&host_flags[4], d_status, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    KOCR_TRY(finish());
    ctx->last_pl = {d_boxes, dv.d_counts, d_lab, N, d_cap, (int)M, rec.LW, Resident::VALID};
    ctx->keep_det_scores(dv.d_scores, N, d_cap);
    rec.keep(won);
    if (!host_fits)
      KOCR_FAIL(ctx, KOCR_ECAPACITY, fn + ": an image has more boxes than cap, or there are more crops than max_crops; the results are "
                                     "resident -- fetch them with kocr_pipeline_results into buffers sized from counts / n_crops");
    return KOCR_OK;
  };
  if (oriented) {
    // ---- both orientations of every box: turned set-up on the device, 2 M crops, recogniser with scores, choice ----
    OrientRun r(ctx, M);
    KOCR_TRY(io.reserve(0, {}, {staging_bytes(r), 256}));
    KOCR_TRY(staging_take(io, r));
    KOCR_TRY(io.scratch(256, d_status));
    KOCR_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int), ctx->stream));
    KOCR_TRY(launch_warp_prepare_turned(ctx, d_boxes, dv.d_counts, N, d_cap, ctx->orient_mode, ctx->orient_ratio, CRNN_CROP_H,
                                        CRNN_CROP_W, r.prm, r.turns2, r.quads2, d_status));
    KOCR_TRY(orient_run(ctx, d_bat, Hmax, Wmax, r));
    return finish_crops(r.rec, &r.won);
  }
  // ---- crops: homographies on the device (warp.hip), no host round trip; then the recogniser ----
  const size_t crop_b = (size_t)M * CRNN_CROP_PIXELS * sizeof(float), pb = (size_t)M * sizeof(WarpParam);
  RecStage rec(ctx, M);
  KOCR_TRY(io.reserve(0, {}, {pb, crop_b, 256, rec.bytes()}));
  WarpParam* d_prm;
  float* d_crops;
  KOCR_TRY(io.scratch(pb, d_prm));
  KOCR_TRY(io.scratch(crop_b, d_crops));
  KOCR_TRY(io.scratch(256, d_status));
  KOCR_TRY(rec.take(io));
  KOCR_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int), ctx->stream));
  KOCR_TRY(launch_warp_prepare(ctx, d_boxes, dv.d_counts, N, d_cap, CRNN_CROP_H, CRNN_CROP_W, d_prm, d_status));
  KOCR_TRY(launch_warp(ctx, d_bat, Hmax, Wmax, d_prm, (int)M, CRNN_CROP_H, CRNN_CROP_W, d_crops));
  KOCR_TRY(rec.run(d_crops));
  return finish_crops(rec, nullptr);
}

// The getters of resident results (include/kocr.h) share one sequence: produced with the switch off -> KOCR_EINVAL; nothing
// resident -> KOCR_EINVAL; the sizes reported; buffers too small -> KOCR_ECAPACITY; nothing to copy -> KOCR_OK; the copies on
// the ctx stream; synchronise.  What is copied: one pitched block (the detector side: `rows` device rows of dev_pitch bytes
// into the caller's rows host_pitch apart; `fits`: the caller's buffer is there and wide enough), then M crops of every flat
// row (the recogniser side: `bytes` per crop, as they were PRODUCED, whatever the context's settings say by now).
struct FetchSize {
  int32_t* out;
  int value;
};
struct FetchBlock {
  void* host;
  size_t host_pitch;
  const void* dev;
  size_t dev_pitch;
  int rows;
  bool fits;
};
struct FetchRow {
  void* host;
  const void* dev;
  size_t bytes;
};

int fetch_resident(kocr_ctx* ctx, const char* fn, Resident state, const char* off_tail, const char* none_tail, const std::string& small_tail,
                   std::initializer_list<FetchSize> sizes, const FetchBlock* block, int M, int max_crops,
                   std::initializer_list<FetchRow> rows) {
  if (state == Resident::OFF) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + off_tail);
  if (state == Resident::NONE) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + none_tail);
  for (const FetchSize& s : sizes)
    if (s.out) *s.out = s.value;
  bool fits = (!block || block->fits) && (M == 0 || max_crops >= M);
  for (const FetchRow& r : rows) fits = fits && (M == 0 || r.host);
  if (!fits) KOCR_FAIL(ctx, KOCR_ECAPACITY, std::string(fn) + small_tail);
  if (!block && M == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  if (block)
    KOCR_HIP(ctx, hipMemcpy2DAsync(block->host, block->host_pitch, block->dev, block->dev_pitch, block->dev_pitch, (size_t)block->rows,
                                   hipMemcpyDeviceToHost, ctx->stream));
  if (M > 0)
    for (const FetchRow& r : rows) KOCR_HIP(ctx, hipMemcpyAsync(r.host, r.dev, (size_t)M * r.bytes, hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

std::string smaller_than(const char* what, int M) {
  return std::string(": buffers smaller than the resident ") + what + " (max_crops >= " + std::to_string(M) + ")";
}
const char* const SCORES_OFF = ": the results on this context were produced with scores off (kocr_set_scores(ctx, 1) before the call)";
}  // namespace

// The resident results of the last kocr_pipeline call copied into the caller's (larger) buffers: see include/kocr.h
extern "C" int kocr_pipeline_results(kocr_ctx* ctx, float* boxes, int cap, int32_t* labels, int max_crops) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_pl;
  const FetchBlock rows{boxes, (size_t)cap * 32, r.d_boxes, (size_t)r.cap * 32, r.N, boxes && cap >= r.cap};
  return fetch_resident(ctx, "kocr_pipeline_results", r.state, "", ": no kocr_pipeline result is resident (call it right after kocr_pipeline)",
                        ": buffers smaller than the resident results (cap >= " + std::to_string(r.cap) + ", max_crops >= " +
                            std::to_string(r.M) + ")",
                        {}, &rows, r.M, max_crops, {{labels, r.d_labels, r.lw * sizeof(int32_t)}});
}

// The resident scores (see include/kocr.h, "Scores")
extern "C" int kocr_detection_scores(kocr_ctx* ctx, float* scores, int cap) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_sc;
  const FetchBlock rows{scores, (size_t)cap * 4, r.d_det, (size_t)r.cap * 4, r.N, scores && cap >= r.cap};
  return fetch_resident(ctx, "kocr_detection_scores", r.det, SCORES_OFF,
                        ": no detection scores are resident (call it right after kocr_get_boxes, kocr_detect or kocr_pipeline)",
                        ": buffer smaller than the resident scores (cap >= " + std::to_string(r.cap) + ")", {}, &rows, 0, 0, {});
}

extern "C" int kocr_recognition_scores(kocr_ctx* ctx, float* log_word, float* char_scores, int max_crops, int32_t* n_crops,
                                       int32_t* label_width) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_sc;
  return fetch_resident(ctx, "kocr_recognition_scores", r.rec, SCORES_OFF, ": no recognition scores are resident (call it right after kocr_recognize_boxes or kocr_pipeline)",
                        smaller_than("scores", r.M), {{n_crops, r.M}, {label_width, r.lw}}, nullptr, r.M, max_crops,
                        {{log_word, r.d_logw, sizeof(float)}, {char_scores, r.d_chars, r.lw * sizeof(float)}});
}

// The resident beam alternatives (see include/kocr.h, "Beam search")
extern "C" int kocr_recognition_beams(kocr_ctx* ctx, int32_t* labels, float* log_prob, int max_crops, int32_t* n_crops,
                                      int32_t* label_width, int32_t* top_paths) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_beam;
  return fetch_resident(ctx, "kocr_recognition_beams", r.state,
                        ": the results on this context were produced with the beam off (kocr_set_beam(ctx, beam_width, top_paths) before the call)",
                        ": no beam alternatives are resident (call it right after kocr_recognize_boxes or kocr_pipeline)", smaller_than("alternatives", r.M),
                        {{n_crops, r.M}, {label_width, r.lw}, {top_paths, r.K}}, nullptr, r.M, max_crops,
                        {{labels, r.d_labels, (size_t)r.K * r.lw * sizeof(int32_t)}, {log_prob, r.d_logp, r.K * sizeof(float)}});
}

// The resident lexicon matches (see include/kocr.h, "Lexicon")
extern "C" int kocr_recognition_lexicon(kocr_ctx* ctx, int32_t* index, float* log_prob, int max_crops, int32_t* n_crops,
                                        int32_t* top_words) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_lex;
  return fetch_resident(ctx, "kocr_recognition_lexicon", r.state,
                        ": the results on this context were produced with the lexicon match off (kocr_set_lexicon_match(ctx, top_words) before "
                        "the call)",
                        ": no lexicon matches are resident (call it right after kocr_recognize_boxes or kocr_pipeline)", smaller_than("matches", r.M),
                        {{n_crops, r.M}, {top_words, r.K}}, nullptr, r.M, max_crops,
                        {{index, r.d_index, r.K * sizeof(int32_t)}, {log_prob, r.d_logp, r.K * sizeof(float)}});
}

// The resident pattern decodes (see include/kocr.h, "Patterns")
extern "C" int kocr_recognition_patterns(kocr_ctx* ctx, int32_t* labels, float* log_path, float* log_prob, int max_crops, int32_t* n_crops) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_pat;
  return fetch_resident(ctx, "kocr_recognition_patterns", r.state,
                        ": the results on this context were produced with the pattern off (kocr_set_pattern(ctx, index) before the call)",
                        ": no pattern decodes are resident (call it right after kocr_recognize_boxes or kocr_pipeline)", smaller_than("decodes", r.M),
                        {{n_crops, r.M}}, nullptr, r.M, max_crops,
                        {{labels, r.d_labels, r.lw * sizeof(int32_t)}, {log_path, r.d_logpath, sizeof(float)}, {log_prob, r.d_logp, sizeof(float)}});
}

// The results of the last successful kocr_pipeline call as they lie in HBM (see include/kocr.h)
extern "C" int kocr_pipeline_device_results(kocr_ctx* ctx, const float** d_boxes, const int32_t** d_counts, const int32_t** d_labels,
                                            int32_t* N, int32_t* cap, int32_t* M) {
  if (!ctx) return KOCR_EINVAL;
  if (ctx->last_pl.state != Resident::VALID)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_pipeline_device_results: no kocr_pipeline result is resident (call it right after kocr_pipeline)");
  if (d_boxes) *d_boxes = ctx->last_pl.d_boxes;
  if (d_counts) *d_counts = ctx->last_pl.d_counts;
  if (d_labels) *d_labels = ctx->last_pl.d_labels;
  if (N) *N = ctx->last_pl.N;
  if (cap) *cap = ctx->last_pl.cap;
  if (M) *M = ctx->last_pl.M;
  return KOCR_OK;
}

// How many label rows of which width are resident (see include/kocr.h): the width they were PRODUCED with
extern "C" int kocr_pipeline_results_shape(kocr_ctx* ctx, int32_t* n_crops, int32_t* label_width) {
  if (!ctx) return KOCR_EINVAL;
  if (ctx->last_pl.state != Resident::VALID)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_pipeline_results_shape: no kocr_pipeline result is resident (call it right after kocr_pipeline)");
  if (n_crops) *n_crops = ctx->last_pl.M;
  if (label_width) *label_width = ctx->last_pl.lw;
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
  return fetch_resident(ctx, "kocr_recognition_orientation", r.state,
                        ": the results on this context were produced with orientation off (kocr_set_orientation(ctx, mode, tall_ratio) before "
                        "the call)",
                        ": no orientation is resident (call it right after kocr_recognize_boxes or kocr_pipeline)", smaller_than("orientation", r.M), {{n_crops, r.M}}, nullptr,
                        r.M, max_crops,
                        {{turns, r.d_turns, sizeof(int32_t)}, {quads, r.d_quads, 8 * sizeof(float)}, {log_words, r.d_pairs, 2 * sizeof(float)}});
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
  return warp_status_error(ctx, fn, status);
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

// ---- tiled pages (include/kocr.h, "tiled pages"; DESIGN.md section 4, "Tiled pages") ----
int tile_plan(kocr_ctx* ctx, const char* fn, int H, int W, int tile, int overlap, TilePlan& p) {
  const std::string f(fn);
  if (H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20)) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": page sides must be in [1, 2^20]");
  if (tile < 64 || tile % 32 != 0 || tile > (1 << 15)) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": tile must be a multiple of 32 in [64, 32768]");
  if (overlap < 0 || overlap % 16 != 0) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": overlap must be a non-negative multiple of 16");
  if (tile - 2 * overlap < 32) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": the stride tile - 2 overlap must be at least 32");
  p.T = tile;
  p.O = overlap;
  p.S = tile - 2 * overlap;
  auto count = [&](int d) { return d <= p.T ? 1 : (d - p.T + p.S - 1) / p.S + 1; };
  p.ny = count(H);
  p.nx = count(W);
  p.Hc = (p.ny - 1) * p.S + p.T;
  p.Wc = (p.nx - 1) * p.S + p.T;
  p.nT = p.ny * p.nx;
  return KOCR_OK;
}

namespace {
// The plan of N canvases that already have the plan's size, or KOCR_EINVAL
int canvas_plan(kocr_ctx* ctx, const char* fn, int N, int Hc, int Wc, int tile, int overlap, TilePlan& p) {
  KOCR_TRY(tile_plan(ctx, fn, Hc, Wc, tile, overlap, p));
  if (p.Hc != Hc || p.Wc != Wc)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": " + std::to_string(Hc) + " x " + std::to_string(Wc) + " is not a canvas of this tile and overlap (kocr_tile_plan gives " +
                                    std::to_string(p.Hc) + " x " + std::to_string(p.Wc) + ")");
  if ((size_t)N * p.nT > 0x7fffffffu) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": too many tiles");
  return KOCR_OK;
}

// The stitched heat-map goes to the post-processing, whose heat-map sides end at 4096 (postproc_get_boxes): the first limit a
// growing canvas meets
constexpr int TILED_MAX_CANVAS = 8192;
int tiled_limit(kocr_ctx* ctx, const char* fn, const TilePlan& p) {
  if (p.Hc > TILED_MAX_CANVAS || p.Wc > TILED_MAX_CANVAS)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": the canvas " + std::to_string(p.Hc) + " x " + std::to_string(p.Wc) +
                                    " exceeds 8192 x 8192 detector-input pixels (the post-processing takes heat-maps of at most 4096 x 4096)");
  return KOCR_OK;
}

size_t tiles_bytes(int N, const TilePlan& p) { return (size_t)N * p.nT * p.T * p.T * 3; }
size_t tile_heat_bytes(int N, const TilePlan& p) { return (size_t)N * p.nT * (p.T / 2) * (p.T / 2) * 2 * sizeof(float); }
size_t page_heat_bytes(int N, const TilePlan& p) { return (size_t)N * (p.Hc / 2) * (p.Wc / 2) * 2 * sizeof(float); }

// gather -> detector forward over the N nT tiles (micro_batch of them at a time) -> stitch, all on buffers in HBM
int forward_tiled(kocr_ctx* ctx, const uint8_t* d_canvas, int N, const TilePlan& p, int micro_batch, uint8_t* d_tiles, float* d_tile_heat,
                  float* d_heat) {
  const int NT = N * p.nT, T = p.T;
  const size_t tile_px = (size_t)T * T, heat_px = (size_t)(T / 2) * (T / 2);
  KOCR_TRY(launch_tile_gather(ctx, d_canvas, N, p, d_tiles));
  KOCR_TRY(ctx->ws_reserve(craft_workspace_bytes(craft_micro_batch(micro_batch, NT, T, T), T, T)));
  KOCR_TRY(craft_batches(ctx, micro_batch, NT, T, T, [&](int s, int nb) {
    return craft_forward(ctx, d_tiles + s * tile_px * 3, KOCR_U8, nb, T, T, d_tile_heat + s * heat_px * 2);
  }));
  return launch_heat_stitch(ctx, d_tile_heat, N, p, d_heat);
}
}  // namespace

extern "C" int kocr_tile_plan(kocr_ctx* ctx, int H, int W, int tile, int overlap, int32_t* out) {
  if (!ctx || !out) return KOCR_EINVAL;
  TilePlan p;
  KOCR_TRY(tile_plan(ctx, "kocr_tile_plan", H, W, tile, overlap, p));
  const int32_t v[6] = {p.ny, p.nx, p.Hc, p.Wc, p.S, p.nT};
  std::memcpy(out, v, sizeof(v));
  return KOCR_OK;
}

extern "C" int kocr_gather_tiles(kocr_ctx* ctx, const uint8_t* canvas, int N, int Hc, int Wc, int tile, int overlap, uint8_t* tiles,
                                 int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || (N > 0 && (!canvas || !tiles))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_gather_tiles: null buffer");
  if (N == 0) return KOCR_OK;
  TilePlan p;
  KOCR_TRY(canvas_plan(ctx, "kocr_gather_tiles", N, Hc, Wc, tile, overlap, p));
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t cb = (size_t)N * Hc * Wc * 3, tb = tiles_bytes(N, p);
  Staging st{ctx, ctx->io, "kocr_gather_tiles", on_device != 0};
  KOCR_TRY(st.reserve(0, {cb, tb}));
  const uint8_t* d_canvas;
  uint8_t* d_tiles;
  KOCR_TRY(st.in(canvas, cb, d_canvas));
  KOCR_TRY(st.out(tiles, tb, d_tiles));
  KOCR_TRY(launch_tile_gather(ctx, d_canvas, N, p, d_tiles));
  KOCR_TRY(st.back(tiles, d_tiles, tb));
  return st.finish();
}

extern "C" int kocr_stitch_heat(kocr_ctx* ctx, const float* tile_heat, int N, int Hc, int Wc, int tile, int overlap, float* heat,
                                int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || (N > 0 && (!tile_heat || !heat))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_stitch_heat: null buffer");
  if (N == 0) return KOCR_OK;
  TilePlan p;
  KOCR_TRY(canvas_plan(ctx, "kocr_stitch_heat", N, Hc, Wc, tile, overlap, p));
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t tb = tile_heat_bytes(N, p), hb = page_heat_bytes(N, p);
  Staging st{ctx, ctx->io, "kocr_stitch_heat", on_device != 0};
  KOCR_TRY(st.reserve(0, {tb, hb}));
  const float* d_tile_heat;
  float* d_heat;
  KOCR_TRY(st.in(tile_heat, tb, d_tile_heat));
  KOCR_TRY(st.out(heat, hb, d_heat));
  KOCR_TRY(launch_heat_stitch(ctx, d_tile_heat, N, p, d_heat));
  KOCR_TRY(st.back(heat, d_heat, hb));
  return st.finish();
}

extern "C" int kocr_craft_forward_tiled(kocr_ctx* ctx, const uint8_t* canvas, int N, int Hc, int Wc, int tile, int overlap, float* heat,
                                        int micro_batch, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  const char* fn = "kocr_craft_forward_tiled";
  if (N < 0 || (N > 0 && (!canvas || !heat))) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": null buffer");
  if (N == 0) return KOCR_OK;
  TilePlan p;
  KOCR_TRY(canvas_plan(ctx, fn, N, Hc, Wc, tile, overlap, p));
  KOCR_TRY(tiled_limit(ctx, fn, p));
  if (!craft_loaded(ctx)) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, std::string(fn) + ": call kocr_load_craft first");  // ahead of the tile gather
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t cb = (size_t)N * Hc * Wc * 3, hb = page_heat_bytes(N, p), tb = tiles_bytes(N, p), thb = tile_heat_bytes(N, p);
  Staging st{ctx, ctx->pl, fn, on_device != 0};
  KOCR_TRY(st.reserve(0, {cb, hb}, {tb, thb}));
  const uint8_t* d_canvas;
  uint8_t* d_tiles;
  float *d_tile_heat, *d_heat;
  KOCR_TRY(st.in(canvas, cb, d_canvas));
  KOCR_TRY(st.out(heat, hb, d_heat));
  KOCR_TRY(st.scratch(tb, d_tiles));
  KOCR_TRY(st.scratch(thb, d_tile_heat));
  KOCR_TRY(forward_tiled(ctx, d_canvas, N, p, micro_batch, d_tiles, d_tile_heat, d_heat));
  KOCR_TRY(st.back(heat, d_heat, hb));
  return st.finish();
}

// kocr_detect on canvases read in tiles: the getBoxes half runs on the stitched maps
extern "C" int kocr_detect_tiled(kocr_ctx* ctx, const uint8_t* canvas, int N, int Hc, int Wc, int tile, int overlap,
                                 float detection_threshold, float text_threshold, float link_threshold, int size_threshold,
                                 int micro_batch, float* boxes, int32_t* counts, int cap, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  const char* fn = "kocr_detect_tiled";
  if (N < 0 || (N > 0 && (!canvas || !boxes || !counts))) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": null buffer");
  if (N == 0) return KOCR_OK;
  if (cap <= 0) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": cap must be positive");
  TilePlan p;
  KOCR_TRY(canvas_plan(ctx, fn, N, Hc, Wc, tile, overlap, p));
  KOCR_TRY(tiled_limit(ctx, fn, p));
  if (!craft_loaded(ctx)) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, std::string(fn) + ": call kocr_load_craft first");  // ahead of the tile gather
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int h2 = Hc / 2, w2 = Wc / 2;
  const size_t cb = (size_t)N * Hc * Wc * 3, hb = page_heat_bytes(N, p), tb = tiles_bytes(N, p), thb = tile_heat_bytes(N, p);
  const size_t box_b = (size_t)N * cap * 8 * sizeof(float);
  Staging st{ctx, ctx->pl, fn, on_device != 0};
  KOCR_TRY(st.reserve(0, {cb}, {hb, box_b, tb, thb}));
  const uint8_t* d_canvas;
  uint8_t* d_tiles;
  float *d_tile_heat, *d_heat, *d_boxes;
  KOCR_TRY(st.scratch(hb, d_heat));
  KOCR_TRY(st.out(boxes, box_b, d_boxes));
  KOCR_TRY(st.in(canvas, cb, d_canvas));
  KOCR_TRY(st.scratch(tb, d_tiles));
  KOCR_TRY(st.scratch(thb, d_tile_heat));
  KOCR_TRY(forward_tiled(ctx, d_canvas, N, p, micro_batch, d_tiles, d_tile_heat, d_heat));
  int n_empty = 0;
  const float* d_scores = nullptr;
  KOCR_TRY(postproc_get_boxes(ctx, d_heat, N, h2, w2, detection_threshold, text_threshold, link_threshold, size_threshold, d_boxes, cap,
                              counts, &n_empty, nullptr, &d_scores));
  KOCR_TRY(chars_resident(ctx, fn, d_heat, N, h2, w2, d_boxes, cap, counts));
  KOCR_TRY(st.back(boxes, d_boxes, box_b));
  KOCR_TRY(st.finish());
  ctx->keep_det_scores(d_scores, N, cap);
  if (n_empty > 0) KOCR_FAIL(ctx, KOCR_EEMPTYCONTOUR, std::string(fn) + ": empty contour list (IndexError at detection.py:272)");
  return KOCR_OK;
}

// kocr_pipeline with the detector run in tiles: resize + pad to the canvas of the largest page -> gather -> forward -> stitch
// -> the shared tail
extern "C" int kocr_pipeline_tiled(kocr_ctx* ctx, int N, const uint8_t* const* imgs, const int32_t* hs, const int32_t* ws,
                                   const int32_t* dhs, const int32_t* dws, int tile, int overlap, float detection_threshold,
                                   float text_threshold, float link_threshold, int size_threshold, int micro_batch, float* boxes,
                                   int32_t* counts, int cap, int32_t* labels, int max_crops, int32_t* n_crops, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  const PipelineCall c{"kocr_pipeline_tiled", N, imgs, hs, ws, dhs, dws, detection_threshold, text_threshold, link_threshold, size_threshold,
                       micro_batch, boxes, counts, cap, labels, max_crops, n_crops, on_device != 0};
  bool go;
  KOCR_TRY(pipeline_begin(ctx, c, true, &go));
  if (!go) return KOCR_OK;
  int dh = 0, dw = 0;
  for (int i = 0; i < N; ++i) {
    dh = std::max(dh, (int)dhs[i]);
    dw = std::max(dw, (int)dws[i]);
  }
  TilePlan p;
  KOCR_TRY(tile_plan(ctx, c.fn, dh, dw, tile, overlap, p));
  if ((size_t)N * p.nT > 0x7fffffffu) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_pipeline_tiled: too many tiles");
  KOCR_TRY(tiled_limit(ctx, c.fn, p));
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t bat_b = (size_t)N * p.Hc * p.Wc * 3, heat_b = page_heat_bytes(N, p), box_b = (size_t)N * cap * 8 * sizeof(float);
  const size_t tb = tiles_bytes(N, p), thb = tile_heat_bytes(N, p);
  Staging pl{ctx, ctx->pl, c.fn};
  KOCR_TRY(pl.reserve(0, {}, {bat_b, heat_b, box_b, tb, thb}));
  uint8_t *d_bat, *d_tiles;
  float *d_heat, *d_boxes, *d_tile_heat;
  KOCR_TRY(pl.scratch(bat_b, d_bat));
  KOCR_TRY(pl.scratch(heat_b, d_heat));
  KOCR_TRY(pl.scratch(box_b, d_boxes));
  KOCR_TRY(pl.scratch(tb, d_tiles));
  KOCR_TRY(pl.scratch(thb, d_tile_heat));
  KOCR_TRY(pipeline_resize(ctx, c, p.Hc, p.Wc, d_bat));
  KOCR_TRY(forward_tiled(ctx, d_bat, N, p, micro_batch, d_tiles, d_tile_heat, d_heat));
  return pipeline_tail(ctx, c, d_bat, p.Hc, p.Wc, d_heat, d_boxes);
}
