// chars_api.cpp — kocr_char_boxes, the switch and the resident path (include/kocr.h, "characters"): argument checks, staging,
// the two launches of chars.hip.
#include "abi.h"
#include <cmath>
#include <climits>

namespace {

// tests/chars_statement.py: check_rule.  !(a <= x) also refuses a NaN
int chars_validate(kocr_ctx* ctx, const std::string& fn, const CharsRule& rule) {
  if (!(rule.peak_threshold > 0 && std::isfinite(rule.peak_threshold)))
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": peak_threshold " + std::to_string(rule.peak_threshold) + " is not a finite number > 0");
  if (!(rule.valley_ratio >= 0 && rule.valley_ratio <= 1))
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": valley_ratio " + std::to_string(rule.valley_ratio) + " outside [0, 1]");
  if (!(rule.extent_threshold >= 0 && rule.extent_threshold <= rule.peak_threshold))
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": extent_threshold " + std::to_string(rule.extent_threshold) + " outside [0, peak_threshold = " +
                                    std::to_string(rule.peak_threshold) + "]");
  return KOCR_OK;
}

// The two launches for the M = h_off[N] words of N pages whose heat-maps and quads are in HBM (quads: see launch_chars_split).
// Workspace from ctx->chw, the packed results from ctx->chr once the host has the counts: h_counts [M] and *total are
// complete when this returns KOCR_OK or KOCR_ECAPACITY (more than cap_chars characters; nothing is packed then).  With
// want_boxes the packed quads and scores are left at *d_quads / *d_scores, in stream order.
int chars_run(kocr_ctx* ctx, const std::string& fn, const float* d_heat, int N, int h, int w, const float* d_word_quads, int stride,
              const int32_t* h_off, const CharsRule& rule, bool want_boxes, long long cap_chars, int32_t* h_counts, long long* total,
              const float** d_quads, const float** d_scores) {
  *total = 0;
  *d_quads = *d_scores = nullptr;
  const int M = h_off[N];
  if (M == 0) return KOCR_OK;
  const size_t m = (size_t)M, off_b = ((size_t)N + 1) * sizeof(int32_t);
  Staging wk_st{ctx, ctx->chw, fn.c_str()};
  KOCR_TRY(wk_st.reserve(chars_workspace_bytes(N, M), {}));
  const int32_t* d_off;
  CharsWork wk;
  KOCR_TRY(wk_st.upload(h_off, off_b, d_off));
  KOCR_TRY(wk_st.scratch(m * sizeof(int32_t), wk.counts));
  KOCR_TRY(wk_st.scratch(m * sizeof(int32_t), wk.ncols));
  KOCR_TRY(wk_st.scratch(m * KOCR_CHARS_BOUNDS_STRIDE * sizeof(uint16_t), wk.bounds));
  KOCR_TRY(wk_st.scratch(m * KOCR_CHARS_MAX_PER_WORD * sizeof(float), wk.scores));
  KOCR_TRY(launch_chars_split(ctx, d_heat, N, h, w, d_word_quads, d_off, stride, M, rule, wk));
  KOCR_TRY(wk_st.download(h_counts, (const int32_t*)wk.counts, m * sizeof(int32_t)));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the counts size the packed results; h_off has been read
  long long chars = 0;
  for (int j = 0; j < M; ++j) chars += h_counts[j];
  *total = chars;
  if (!want_boxes || chars == 0) return KOCR_OK;
  if (chars > cap_chars)
    KOCR_FAIL(ctx, KOCR_ECAPACITY, fn + ": " + std::to_string(chars) + " characters, char_quads holds " + std::to_string(cap_chars));
  const size_t quads_b = (size_t)chars * 8 * sizeof(float), scores_b = (size_t)chars * sizeof(float);
  Staging res_st{ctx, ctx->chr, fn.c_str()};
  KOCR_TRY(res_st.reserve(0, {}, {quads_b, scores_b}));
  float *d_q, *d_s;
  KOCR_TRY(res_st.scratch(quads_b, d_q));
  KOCR_TRY(res_st.scratch(scores_b, d_s));
  KOCR_TRY(launch_chars_pack(ctx, d_word_quads, d_off, N, stride, M, wk, d_q, d_s));
  *d_quads = d_q;
  *d_scores = d_s;
  return KOCR_OK;
}

int chars_call(kocr_ctx* ctx, const float* heat, int N, int h, int w, const float* quads, const int32_t* offsets, const CharsRule& rule,
               int32_t* char_counts, float* char_quads, float* char_scores, int64_t cap_chars, int64_t* true_chars, int on_device,
               int flags) {
  const std::string fn("kocr_char_boxes");
  if (N < 0 || h < 0 || w < 0 || cap_chars < 0) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": bad sizes");
  if (flags != 0) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": flags must be 0");
  if ((!char_quads || !char_scores) && cap_chars != 0)
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null char_quads or char_scores with cap_chars " + std::to_string((long long)cap_chars));
  KOCR_TRY(chars_validate(ctx, fn, rule));
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  if (true_chars) *true_chars = 0;
  if (N == 0) return KOCR_OK;
  if (!offsets) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null offsets");
  if (offsets[0] != 0) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": offsets must start at 0");
  for (int i = 0; i < N; ++i)
    if (offsets[i + 1] < offsets[i]) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": offsets decreases at entry " + std::to_string(i + 1));
  const size_t total = (size_t)offsets[N];
  if (total == 0) return KOCR_OK;
  if (!heat || !quads || !char_counts) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null buffer");
  for (int i = 0; i < N; ++i)
    for (int j = offsets[i]; j < offsets[i + 1]; ++j)
      for (int c = 0; c < 8; ++c)
        if (!std::isfinite(quads[(size_t)j * 8 + c]))
          KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": page " + std::to_string(i) + ", word " + std::to_string(j - offsets[i]) + ": non-finite coordinate");

  // the quads are uploaded asynchronously from the caller's array: the stream is drained on every return path
  struct Drain {
    hipStream_t stream;
    ~Drain() { (void)hipStreamSynchronize(stream); }
  } drain{ctx->stream};
  const size_t heat_b = (size_t)N * h * w * 2 * sizeof(float), quads_b = total * 8 * sizeof(float);
  Staging st{ctx, ctx->io, "kocr_char_boxes", on_device != 0};
  KOCR_TRY(st.reserve(0, {heat_b}, {quads_b}));
  const float *d_heat, *d_word_quads, *d_quads, *d_scores;
  KOCR_TRY(st.in(heat, heat_b, d_heat));
  KOCR_TRY(st.upload(quads, quads_b, d_word_quads));
  long long chars = 0;
  const int rc = chars_run(ctx, fn, d_heat, N, h, w, d_word_quads, 0, offsets, rule, char_quads != nullptr, cap_chars, char_counts, &chars,
                           &d_quads, &d_scores);
  if (true_chars) *true_chars = chars;
  if (rc != KOCR_OK || !d_quads) return rc;
  KOCR_TRY(st.download(char_quads, d_quads, (size_t)chars * 8 * sizeof(float)));
  KOCR_TRY(st.download(char_scores, d_scores, (size_t)chars * sizeof(float)));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // results are complete on return; a failure is reported
  return KOCR_OK;
}

}  // namespace

int chars_resident(kocr_ctx* ctx, const char* fn, const float* d_heat, int N, int h, int w, const float* d_boxes, int cap,
                   const int32_t* h_counts) {
  if (!ctx->chars_on) return KOCR_OK;
  auto& r = ctx->last_ch;
  r.off.assign((size_t)N + 1, 0);
  for (int i = 0; i < N; ++i) r.off[i + 1] = r.off[i] + std::min(std::max((int)h_counts[i], 0), cap);
  r.counts.assign((size_t)r.off[N], 0);
  return chars_run(ctx, std::string(fn) + " (character boxes)", d_heat, N, h, w, d_boxes, cap, r.off.data(), ctx->chars_rule, true, LLONG_MAX,
                   r.counts.data(), &r.total, &r.d_quads, &r.d_scores);
}

extern "C" {

int kocr_char_boxes(kocr_ctx* ctx, const float* heat, int N, int h, int w, const float* quads, const int32_t* offsets,
                    double peak_threshold, double valley_ratio, double extent_threshold, int32_t* char_counts, float* char_quads,
                    float* char_scores, int64_t cap_chars, int64_t* true_chars, int on_device, int flags) {
  if (!ctx) return KOCR_EINVAL;
  const CharsRule rule{peak_threshold, valley_ratio, extent_threshold};
  return chars_call(ctx, heat, N, h, w, quads, offsets, rule, char_counts, char_quads, char_scores, cap_chars, true_chars, on_device, flags);
}

int kocr_set_char_boxes(kocr_ctx* ctx, int on, double peak_threshold, double valley_ratio, double extent_threshold) {
  if (!ctx) return KOCR_EINVAL;
  if (on != 0 && on != 1) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_char_boxes: on must be 0 or 1");
  if (on) {
    const CharsRule rule{peak_threshold, valley_ratio, extent_threshold};
    KOCR_TRY(chars_validate(ctx, "kocr_set_char_boxes", rule));
    ctx->chars_rule = rule;
  }
  ctx->chars_on = on != 0;
  return KOCR_OK;
}

int kocr_get_char_boxes(const kocr_ctx* ctx, int* on, double* peak_threshold, double* valley_ratio, double* extent_threshold) {
  if (!ctx) return KOCR_EINVAL;
  if (on) *on = ctx->chars_on ? 1 : 0;
  if (peak_threshold) *peak_threshold = ctx->chars_rule.peak_threshold;
  if (valley_ratio) *valley_ratio = ctx->chars_rule.valley_ratio;
  if (extent_threshold) *extent_threshold = ctx->chars_rule.extent_threshold;
  return KOCR_OK;
}

int kocr_detection_char_boxes(kocr_ctx* ctx, int32_t* char_counts, float* char_quads, float* char_scores, int cap, int64_t cap_chars,
                              int64_t* true_chars) {
  if (!ctx) return KOCR_EINVAL;
  const auto& r = ctx->last_ch;
  const std::string fn("kocr_detection_char_boxes");
  if (r.state == Resident::OFF)
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": the results on this context were produced with character boxes off (kocr_set_char_boxes(ctx, 1, "
                                     "...) before the call)");
  if (r.state == Resident::NONE)
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": no character boxes are resident (call it right after kocr_get_boxes, kocr_detect or kocr_pipeline)");
  if (true_chars) *true_chars = r.total;
  if (cap_chars < 0 || ((!char_quads || !char_scores) && cap_chars != 0))
    KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null char_quads or char_scores with cap_chars " + std::to_string((long long)cap_chars));
  if (!char_counts || cap < r.cap)
    KOCR_FAIL(ctx, KOCR_ECAPACITY, fn + ": buffer smaller than the resident counts (cap >= " + std::to_string(r.cap) + ")");
  // the counts lie on the host in packed word order; the caller's rows are cap words apart
  for (int i = 0; i < r.N; ++i) {
    int32_t* row = char_counts + (size_t)i * cap;
    const int words = r.off[i + 1] - r.off[i];
    std::copy(r.counts.begin() + r.off[i], r.counts.begin() + r.off[i + 1], row);
    std::fill(row + words, row + cap, 0);
  }
  if (!char_quads || r.total == 0) return KOCR_OK;
  if (r.total > cap_chars)
    KOCR_FAIL(ctx, KOCR_ECAPACITY, fn + ": " + std::to_string(r.total) + " characters, char_quads holds " + std::to_string((long long)cap_chars));
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  KOCR_HIP(ctx, hipMemcpyAsync(char_quads, r.d_quads, (size_t)r.total * 8 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipMemcpyAsync(char_scores, r.d_scores, (size_t)r.total * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

}  // extern "C"
