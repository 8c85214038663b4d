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
    arena.off = 0;
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

// The warp parameters of the boxes [M][4][2] (HOST) of N images, counts[i] (HOST) of them in image i, for crops of
// th x tw; `out` is the caller's result buffer (checked once there are boxes).  Returns M, or a negative KOCR_* code: a
// negative count or a null buffer KOCR_EINVAL, a box with zero width or height KOCR_EZERODIV (the reference's
// ZeroDivisionError), a singular transform KOCR_EINVAL.  M == 0 prepares nothing.
long prepare_box_warps(kocr_ctx* ctx, const char* fn, int N, const float* boxes, const int32_t* counts, const void* out, int th,
                       int tw, std::vector<WarpParam>& prm);

// The temporary layer of a kocr_conv2d_* call: the device buffers its preparation adds to ctx->owned after construction are
// freed, once the stream has drained, on every return path.
struct TempLayer {
  kocr_ctx* ctx;
  size_t mark;
  explicit TempLayer(kocr_ctx* c) : ctx(c), mark(c->owned.size()) {}
  ~TempLayer() {
    hipStreamSynchronize(ctx->stream);
    while (ctx->owned.size() > mark) {
      hipFree(ctx->owned.back());
      ctx->owned.pop_back();
    }
  }
};
