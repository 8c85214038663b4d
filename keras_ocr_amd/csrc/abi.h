// abi.h — host-side helpers shared by the extern "C" entry points of api.cpp and pipeline.cpp.
#pragma once
#include "common.h"
#include <algorithm>
#include <initializer_list>

// The device view of an entry point's caller buffers.  With on_device the caller's pointer is used as it is; otherwise
// `in` places an arena copy of a host input (hipMemcpyAsync on the ctx stream), `out` an arena buffer for a result that
// `back` copies to the caller.  `upload` / `scratch` / `download` do the same for buffers that live on the host, or only on
// the device, whatever on_device says; `put` copies a host array into a device buffer of the caller's.  Every arena
// allocation is checked: KOCR_ENOMEM naming the entry point.
struct Staging {
  kocr_ctx* ctx;
  Arena& arena;
  const char* fn;
  bool on_device = false;

  // Sizes the arena for `base` bytes (whatever the callee itself allocates there) plus the buffers this call takes from it:
  // each of `staged` unless on_device, each of `always`, placed as arena_alloc places them; then empties it.  Nothing is
  // reserved when that is zero.
  int reserve(size_t base, std::initializer_list<size_t> staged, std::initializer_list<size_t> always = {}) {
    size_t need = base;
    if (!on_device)
      for (size_t b : staged) need += b + 256;
    for (size_t b : always) need += b + 256;
    if (need) KOCR_TRY(arena_reserve(ctx, arena, need + 8192));
    arena.reset();
    return KOCR_OK;
  }
  template <class T> int scratch(size_t bytes, T*& d) {
    d = (T*)arena_alloc(arena, bytes);
    if (!d) KOCR_FAIL(ctx, KOCR_ENOMEM, std::string(fn) + ": workspace exhausted");
    return KOCR_OK;
  }
  template <class T> int put(T* d, const T* host, size_t bytes) {
    KOCR_HIP(ctx, hipMemcpyAsync((void*)d, (const void*)host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return KOCR_OK;
  }
  template <class T> int upload(const T* host, size_t bytes, const T*& d) {
    T* p;
    KOCR_TRY(scratch(bytes, p));
    d = p;
    return put(p, host, bytes);
  }
  template <class T> int download(T* host, const T* d, size_t bytes) {
    KOCR_HIP(ctx, hipMemcpyAsync((void*)host, (const void*)d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return KOCR_OK;
  }
  template <class T> int in(const T* p, size_t bytes, const T*& d) {
    if (on_device) {
      d = p;
      return KOCR_OK;
    }
    return upload(p, bytes, d);
  }
  template <class T> int out(T* p, size_t bytes, T*& d) {
    if (on_device) {
      d = p;
      return KOCR_OK;
    }
    return scratch(bytes, d);
  }
  template <class T> int back(T* p, const T* d, size_t bytes) { return on_device ? KOCR_OK : download(p, d, bytes); }
  // results copied to the host are complete on return; on_device calls stay asynchronous
  int finish() {
    if (!on_device) KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KOCR_OK;
  }
};

// A buffer list L has each(f): f(pointer&, bytes) for every device buffer it describes, stopping at the first failure.  Its
// bytes as Staging::reserve counts them, and the buffers themselves from an arena:
template <class L> size_t staging_bytes(L& list) {
  size_t total = 0;
  list.each([&](auto*&, size_t b) {
    total += b + 256;
    return KOCR_OK;
  });
  return total;
}
template <class L> int staging_take(Staging& st, L& list) {
  return list.each([&](auto*& p, size_t b) { return st.scratch(b, p); });
}

// Detector images per craft_forward: micro_batch (default 32, the Keras predict batch_size, detection.py:779), halved while
// its workspace exceeds 96 GiB of the 288 GB HBM, at most N.
int craft_micro_batch(int micro_batch, int N, int H, int W);

// The recogniser's batch loop: body(s, nb) for crops [s, s + nb) of M, at most CRNN_BATCH at a time, the workspace reset
// before each batch.  The caller has reserved ctx->ws for crnn_batch(M) crops.
constexpr int CRNN_BATCH = 1024;
inline int crnn_batch(long M) { return (int)std::min<long>(M, CRNN_BATCH); }
template <class Body> int crnn_batches(kocr_ctx* ctx, long M, Body body) {
  for (long s = 0; s < M; s += CRNN_BATCH) {
    ctx->ws_reset();
    KOCR_TRY(body(s, (int)std::min<long>(CRNN_BATCH, M - s)));
  }
  return KOCR_OK;
}

// The detector's twin: body(s, nb) for images [s, s + nb) of N, craft_micro_batch at a time, the workspace reset before each
// batch.  The caller has reserved ctx->ws for craft_micro_batch(micro_batch, N, H, W) images.
template <class Body> int craft_batches(kocr_ctx* ctx, int micro_batch, int N, int H, int W, Body body) {
  const int mb = craft_micro_batch(micro_batch, N, H, W);
  for (int s = 0; s < N; s += mb) {
    ctx->ws_reset();
    KOCR_TRY(body(s, std::min(mb, N - s)));
  }
  return KOCR_OK;
}

// The compact rows of the `words` winners that orient_select_kernel writes in an oriented run (pipeline.cpp)
struct OrientWinners {
  long words = 0;
  int32_t* lab = nullptr;   // [words][LW]
  float* logw = nullptr;    // [words]
  float* chars = nullptr;   // [words][LW]
  int32_t* turn = nullptr;  // [words]
  float* quad = nullptr;    // [words][8]
  float* pair = nullptr;    // [words][2]
};

// The recogniser stage of kocr_recognize_boxes / kocr_pipeline: the request (CrnnDecode, common.h) that the context's switches
// make for M crops -- the label rows always, score rows (scores), beam rows (beam width > 0), lexicon rows (top words > 0),
// pattern rows (pattern switched on) -- and its buffers.  An oriented run is the same stage over its 2 M candidate crops with
// scores forced on (no beam, no lexicon, no pattern: orient_refusal).  req.cm: the character sets the crops are decoded under
// -- the context's uniform switch unless the caller puts a per-crop list in its place (kocr_recognize_boxes_charsets).  req.pt:
// the pattern the crops are also decoded under -- the context's switch, or a per-crop list (set_patterns:
// kocr_recognize_boxes_patterns).
struct RecStage {
  kocr_ctx* ctx;
  long M;
  int LW;
  CrnnDecode req;
  RecStage(kocr_ctx* c, long m, bool force_scores = false) : ctx(c), M(m), LW(crnn_label_width(c)) {
    req.greedy = true;
    req.sc.on = c->scores_on || force_scores;
    req.bm.beam_width = c->beam_width;
    req.bm.top_paths = c->beam_top_paths;
    req.lx.top_words = c->lex_top;
    req.pt.on = c->pattern >= 0;
    req.pt.uniform = c->pattern;
    req.cm = c->charmask();
  }
  // one pattern per crop (HOST list and its device copy, [M]) in place of the context's switch; before bytes() / take()
  void set_patterns(const int32_t* of, const int32_t* d_of) {
    req.pt.on = true;
    req.pt.of = of;
    req.pt.d_of = d_of;
    req.pt.uniform = -1;
  }

  // the request's outputs, each for all M crops (no probabilities, no lexicon values: V plays no part)
  template <class F> int each(F f) {
    return req.each(LW, crnn_classes(ctx), 0, [&](auto*& p, size_t b) { return f(p, (size_t)M * b); });
  }
  // (a) what take() needs of an arena, counted as Staging::reserve counts its buffers
  size_t bytes() { return staging_bytes(*this); }
  // (b) the buffers from `st`
  int take(Staging& st) { return staging_take(st, *this); }
  // (c) the recogniser over d_crops [M][31][200]: ctx->ws sized for one batch (with the lexicon's and the patterns' share),
  // every batch given its rows of the buffers
  int run(const float* d_crops) {
    const int mb = crnn_batch(M), C = crnn_classes(ctx);
    KOCR_TRY(ctx->ws_reserve(crnn_workspace_bytes(mb, C) + (req.lx.top_words ? lexicon_workspace_bytes(ctx, mb, true) : 0) +
                             (req.pt.on ? pattern_workspace_bytes(ctx, (int)M, req.pt) : 0)));
    return crnn_batches(ctx, M, [&](long s, int nb) {
      return crnn_forward(ctx, d_crops + s * CRNN_CROP_PIXELS, nb, req.from(s, LW, C, 0));
    });
  }
  // (d) what the stage leaves resident for the getters, each record with the state of its switch.  An oriented run keeps its
  // winners' rows in place of the stage's own.  A stage of no crops that never ran keeps "nothing, M = 0".
  void keep(const OrientWinners* won = nullptr) const {
    const OrientWinners w = won ? *won : OrientWinners{};
    const int m = (int)(won ? w.words : M);
    ctx->keep_rec_scores(won ? w.logw : req.sc.d_logw, won ? w.chars : req.sc.d_chars, m, LW);
    ctx->keep_beams(req.bm.d_labels, req.bm.d_logp, m, LW);
    ctx->keep_lexicon(req.lx.d_index, req.lx.d_logp, m);
    ctx->keep_patterns(req.pt.d_labels, req.pt.d_logpath, req.pt.d_logp, m, LW, req.pt.on);
    ctx->keep_orientation(w.turn, w.quad, w.pair, (int)w.words);
  }
};

// The status word of the warp set-up (warp_prepare and its kin: 0, 1 = a box with zero width or height, the reference's
// ZeroDivisionError, else a singular transform) as the entry point's error; `at`: how the entry point cites the reference
int warp_status_error(kocr_ctx* ctx, const char* fn, int status, const char* at = "ZeroDivisionError at tools.py:95");

// The warp parameters of the boxes [M][4][2] (HOST) of N images, counts[i] (HOST) of them in image i, for crops of
// th x tw; `out` is the caller's result buffer (checked once there are boxes).  Returns M, or a negative KOCR_* code: a
// negative count or a null buffer KOCR_EINVAL, a box with zero width or height KOCR_EZERODIV (the reference's
// ZeroDivisionError), a singular transform KOCR_EINVAL.  M == 0 prepares nothing.
long prepare_box_warps(kocr_ctx* ctx, const char* fn, int N, const float* boxes, const int32_t* counts, const void* out, int th,
                       int tw, std::vector<WarpParam>& prm);

// The temporary layer of a kocr_conv2d_* call: the device buffers its preparation adds to ctx->owned after construction are
// freed, once the stream has drained, on every return path.  A buffer that is to outlive the call must therefore be allocated
// BEFORE the mark is taken (the max-|x| slot pool: amax_begin ahead of the layer; the range-statistics block:
// kocr_range_stats_enable) -- tests/test_lifecycle_gpu.py checks what a first call leaves behind.
struct TempLayer {
  kocr_ctx* ctx;
  size_t mark;
  explicit TempLayer(kocr_ctx* c) : ctx(c), mark(c->owned.size()) {}
  ~TempLayer() {
    hipStreamSynchronize(ctx->stream);
    ctx->release_since(mark);
  }
};
