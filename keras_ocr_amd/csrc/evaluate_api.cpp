// evaluate_api.cpp — kocr_iou_table / kocr_score (include/kocr.h, "evaluation"): argument checks, staging, the three launches
// of evaluate.hip.
#include "abi.h"

namespace {

// One offset array on the host (read back when it lives on the device), checked: starts at 0, never decreases.
int eval_offsets(kocr_ctx* ctx, const std::string& fn, const char* what, const int32_t* off, size_t n, bool on_device,
                 std::vector<int32_t>& host) {
  host.assign(n + 1, 0);
  if (!off) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null " + what);
  if (on_device)
    KOCR_HIP(ctx, hipMemcpy(host.data(), off, (n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
  else
    memcpy(host.data(), off, (n + 1) * sizeof(int32_t));
  if (host[0] != 0) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": " + what + " must start at 0");
  for (size_t i = 0; i < n; ++i)
    if (host[i + 1] < host[i])
      KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": " + what + " decreases at entry " + std::to_string(i + 1));
  return KOCR_OK;
}

// the image of annotation a of a batch with these offsets (for messages)
int image_of(const std::vector<int32_t>& off, int a) {
  return (int)(std::upper_bound(off.begin(), off.end(), a) - off.begin()) - 1;
}

int eval_quads(kocr_ctx* ctx, const std::string& fn, const char* what, const int32_t* quads, const std::vector<int32_t>& off) {
  const int n = off.back();
  for (int a = 0; a < n; ++a)
    for (int c = 0; c < 8; ++c) {
      const int32_t v = quads[(size_t)a * 8 + c];
      if (v <= -(1 << 24) || v >= (1 << 24)) {
        const int img = image_of(off, a);
        KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": image " + std::to_string(img) + ", " + what + " " + std::to_string(a - off[img]) +
                                        ": coordinate " + std::to_string(v) + " outside (-2^24, 2^24)");
      }
    }
  return KOCR_OK;
}

int eval_texts(kocr_ctx* ctx, const std::string& fn, const char* what, const std::vector<int32_t>& text_off, const std::vector<int32_t>& off) {
  for (size_t a = 0; a + 1 < text_off.size(); ++a)
    if (text_off[a + 1] - text_off[a] > KOCR_SCORE_MAX_TEXT) {
      const int img = image_of(off, (int)a);
      KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": image " + std::to_string(img) + ", " + what + " " + std::to_string((int)a - off[img]) + ": text of " +
                                      std::to_string(text_off[a + 1] - text_off[a]) + " code points, more than KOCR_SCORE_MAX_TEXT = " +
                                      std::to_string(KOCR_SCORE_MAX_TEXT));
    }
  return KOCR_OK;
}

// Staging::in / back for buffers that may be empty (and then null): nothing is copied for zero bytes
template <class T> int ev_in(Staging& st, const T* p, size_t bytes, const T*& d) {
  if (bytes || st.on_device) return st.in(p, bytes, d);
  T* q;
  KOCR_TRY(st.scratch(0, q));
  d = q;
  return KOCR_OK;
}
template <class T> int ev_back(Staging& st, T* p, const T* d, size_t bytes) { return bytes ? st.back(p, d, bytes) : KOCR_OK; }

struct ScoreArgs {
  const uint8_t* ignore = nullptr;
  const int32_t *ttext = nullptr, *ttoff = nullptr, *ptext = nullptr, *ptoff = nullptr;
  double iou_threshold = 0, similarity_threshold = 0;
  uint8_t *pair_class = nullptr, *truth_missed = nullptr, *pred_unclaimed = nullptr;
  int64_t* counts = nullptr;
};

int eval_run(kocr_ctx* ctx, const char* name, int N, const int32_t* tq, const int32_t* toff, const int32_t* pq, const int32_t* poff,
             double* iou, int64_t P_cap, int64_t* P_true, bool on_device, const ScoreArgs* sc) {
  const std::string fn(name);
  if (N < 0 || P_cap < 0) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": bad sizes");
  if (sc && !sc->counts) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null counts");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  if (on_device) KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the offsets may still be in flight on the ctx stream
  if (N == 0) {
    if (P_true) *P_true = 0;
    if (sc) {
      if (on_device)
        KOCR_HIP(ctx, hipMemsetAsync(sc->counts, 0, 3 * sizeof(int64_t), ctx->stream));
      else
        sc->counts[0] = sc->counts[1] = sc->counts[2] = 0;
    }
    return KOCR_OK;
  }
  std::vector<int32_t> h_toff, h_poff, h_ttoff, h_ptoff;
  KOCR_TRY(eval_offsets(ctx, fn, "truth_offsets", toff, (size_t)N, on_device, h_toff));
  KOCR_TRY(eval_offsets(ctx, fn, "pred_offsets", poff, (size_t)N, on_device, h_poff));
  const size_t nt = (size_t)h_toff[N], np = (size_t)h_poff[N];
  if ((nt && !tq) || (np && !pq)) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null quads");
  std::vector<long long> pair_off((size_t)N + 1, 0);
  // pair_off is uploaded asynchronously: the stream is drained on every return path, an error's included, before the vector
  // goes (declared after it, so destroyed first)
  struct Drain {
    hipStream_t stream;
    ~Drain() { (void)hipStreamSynchronize(stream); }
  } drain{ctx->stream};
  for (int i = 0; i < N; ++i)
    pair_off[i + 1] = pair_off[i] + (long long)(h_toff[i + 1] - h_toff[i]) * (long long)(h_poff[i + 1] - h_poff[i]);
  const long long P = pair_off[N];
  if (!on_device) {
    KOCR_TRY(eval_quads(ctx, fn, "truth", tq, h_toff));
    KOCR_TRY(eval_quads(ctx, fn, "prediction", pq, h_poff));
  }
  if (sc) {
    if ((nt && (!sc->ignore || !sc->truth_missed)) || (np && !sc->pred_unclaimed)) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null buffer");
    KOCR_TRY(eval_offsets(ctx, fn, "truth_text_offsets", sc->ttoff, nt, on_device, h_ttoff));
    KOCR_TRY(eval_offsets(ctx, fn, "pred_text_offsets", sc->ptoff, np, on_device, h_ptoff));
    KOCR_TRY(eval_texts(ctx, fn, "truth", h_ttoff, h_toff));
    KOCR_TRY(eval_texts(ctx, fn, "prediction", h_ptoff, h_poff));
    if ((h_ttoff[nt] && !sc->ttext) || (h_ptoff[np] && !sc->ptext)) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null text");
  }
  if (P_true) *P_true = P;
  if (P > P_cap)
    KOCR_FAIL(ctx, KOCR_ECAPACITY, fn + ": " + std::to_string(P) + " pairs, the buffers hold " + std::to_string((long long)P_cap));
  if (P && ((sc && !sc->pair_class) || (!sc && !iou))) KOCR_FAIL(ctx, KOCR_EINVAL, fn + ": null buffer");

  const size_t tq_b = nt * 8 * sizeof(int32_t), pq_b = np * 8 * sizeof(int32_t), off_b = ((size_t)N + 1) * sizeof(int32_t);
  const size_t pair_b = ((size_t)N + 1) * sizeof(long long), iou_b = (size_t)P * sizeof(double);
  const size_t tt_b = sc ? (size_t)h_ttoff[nt] * sizeof(int32_t) : 0, pt_b = sc ? (size_t)h_ptoff[np] * sizeof(int32_t) : 0;
  const size_t tto_b = sc ? (nt + 1) * sizeof(int32_t) : 0, pto_b = sc ? (np + 1) * sizeof(int32_t) : 0;
  const size_t work_b = sc ? (size_t)P * sizeof(EvalWork) : 0, cnt_b = 3 * sizeof(int64_t);
  Staging st{ctx, ctx->io, name, on_device};
  KOCR_TRY(st.reserve(0, {tq_b, off_b, pq_b, off_b, iou_b, sc ? nt : 0, tt_b, tto_b, pt_b, pto_b, sc ? (size_t)P : 0, sc ? nt : 0, sc ? np : 0, cnt_b},
                      {pair_b, work_b, sizeof(unsigned)}));
  EvalBatch b;
  b.N = N;
  b.P = P;
  b.words = (long long)(nt + np);
  KOCR_TRY(ev_in(st, tq, tq_b, b.d_tq));
  KOCR_TRY(ev_in(st, toff, off_b, b.d_toff));
  KOCR_TRY(ev_in(st, pq, pq_b, b.d_pq));
  KOCR_TRY(ev_in(st, poff, off_b, b.d_poff));
  KOCR_TRY(st.upload((const long long*)pair_off.data(), pair_b, b.d_pair_off));
  double* d_iou = nullptr;
  if (iou) KOCR_TRY(st.out(iou, iou_b, d_iou));
  if (!sc) {
    KOCR_TRY(launch_eval_iou(ctx, b, d_iou, 0.0, nullptr, nullptr, nullptr));
    KOCR_TRY(ev_back(st, iou, d_iou, iou_b));
    KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // results are complete on return; a failure is reported
    return KOCR_OK;
  }
  KOCR_TRY(ev_in(st, sc->ignore, nt, b.d_ignore));
  KOCR_TRY(ev_in(st, sc->ttext, tt_b, b.d_ttext));
  KOCR_TRY(ev_in(st, sc->ttoff, tto_b, b.d_ttoff));
  KOCR_TRY(ev_in(st, sc->ptext, pt_b, b.d_ptext));
  KOCR_TRY(ev_in(st, sc->ptoff, pto_b, b.d_ptoff));
  uint8_t *d_class, *d_missed, *d_unclaimed;
  int64_t* d_counts;
  EvalWork* d_work;
  unsigned* d_work_count;
  KOCR_TRY(st.out(sc->pair_class, (size_t)P, d_class));
  KOCR_TRY(st.out(sc->truth_missed, nt, d_missed));
  KOCR_TRY(st.out(sc->pred_unclaimed, np, d_unclaimed));
  KOCR_TRY(st.out(sc->counts, cnt_b, d_counts));
  KOCR_TRY(st.scratch(work_b, d_work));
  KOCR_TRY(st.scratch(sizeof(unsigned), d_work_count));
  KOCR_HIP(ctx, hipMemsetAsync(d_work_count, 0, sizeof(unsigned), ctx->stream));
  KOCR_HIP(ctx, hipMemsetAsync(d_counts, 0, cnt_b, ctx->stream));
  KOCR_TRY(launch_eval_iou(ctx, b, d_iou, sc->iou_threshold, d_class, d_work, d_work_count));
  KOCR_TRY(launch_eval_text(ctx, b, d_work, d_work_count, sc->similarity_threshold, d_class));
  KOCR_TRY(launch_eval_reduce(ctx, b, d_class, d_missed, d_unclaimed, d_counts));
  if (iou) KOCR_TRY(ev_back(st, iou, d_iou, iou_b));
  KOCR_TRY(ev_back(st, sc->pair_class, d_class, (size_t)P));
  KOCR_TRY(ev_back(st, sc->truth_missed, d_missed, nt));
  KOCR_TRY(ev_back(st, sc->pred_unclaimed, d_unclaimed, np));
  KOCR_TRY(ev_back(st, sc->counts, d_counts, cnt_b));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // results are complete on return; a failure is reported
  return KOCR_OK;
}

}  // namespace

extern "C" {

int kocr_iou_table(kocr_ctx* ctx, int N, const int32_t* truth_quads, const int32_t* truth_offsets, const int32_t* pred_quads,
                   const int32_t* pred_offsets, double* iou, int64_t P, int64_t* P_true, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  return eval_run(ctx, "kocr_iou_table", N, truth_quads, truth_offsets, pred_quads, pred_offsets, iou, P, P_true, on_device != 0, nullptr);
}

int kocr_score(kocr_ctx* ctx, int N, const int32_t* truth_quads, const int32_t* truth_offsets, const int32_t* pred_quads,
               const int32_t* pred_offsets, const uint8_t* ignore, const int32_t* truth_text, const int32_t* truth_text_offsets,
               const int32_t* pred_text, const int32_t* pred_text_offsets, double iou_threshold, double similarity_threshold,
               uint8_t* pair_class, uint8_t* truth_missed, uint8_t* pred_unclaimed, int64_t* counts, double* iou, int64_t P,
               int64_t* P_true, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  ScoreArgs sc;
  sc.ignore = ignore;
  sc.ttext = truth_text;
  sc.ttoff = truth_text_offsets;
  sc.ptext = pred_text;
  sc.ptoff = pred_text_offsets;
  sc.iou_threshold = iou_threshold;
  sc.similarity_threshold = similarity_threshold;
  sc.pair_class = pair_class;
  sc.truth_missed = truth_missed;
  sc.pred_unclaimed = pred_unclaimed;
  sc.counts = counts;
  return eval_run(ctx, "kocr_score", N, truth_quads, truth_offsets, pred_quads, pred_offsets, iou, P, P_true, on_device != 0, &sc);
}

}  // extern "C"
