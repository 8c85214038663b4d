// taps.cpp — the launch recorder of kocr_craft_set_taps / kocr_crnn_set_taps (taps.h) and its readers.
#include "taps.h"
#include <algorithm>

namespace {

int tap_copy(kocr_ctx* ctx, Taps::Part& pt, const Tensor& t) {
  Taps* tp = ctx->taps;
  const int W = t.cellW ? t.cellW : t.W;
  const int n = t.cellW ? tp->nb : t.N;  // a cell grid: one cell per image, the first nb cells
  if (!pt.N) {
    pt.N = tp->N;
    pt.H = t.H;
    pt.W = W;
    pt.C = t.C;
    pt.data.assign((size_t)pt.N * t.H * W * t.C, 0.f);
    pt.amax.assign(pt.N, -1.f);
  }
  if (pt.H != t.H || pt.W != W || pt.C != t.C || tp->n0 + n > pt.N || (t.cellW && (size_t)t.N * t.cells() < (size_t)n))
    KOCR_FAIL(ctx, KOCR_EINVAL, "taps: tap shape changed between micro-batches");
  const size_t img = (size_t)t.H * W * t.C;
  float* dst = pt.data.data() + (size_t)tp->n0 * img;
  const size_t row = (size_t)t.C * sizeof(float);
  if (t.cellW) {  // image i = cell (i / cells, i % cells): H rows of cellW pixels, the grid row's pitch apart
    const int cn = t.cells();
    for (int i = 0; i < n; ++i) {
      const float* src = t.p + t.co + ((size_t)(i / cn) * t.H * t.W + (size_t)(i % cn) * t.cellW) * t.cs;
      KOCR_HIP(ctx, hipMemcpy2DAsync(dst + i * img, W * row, src, (size_t)t.W * t.cs * sizeof(float), W * row, t.H,
                                     hipMemcpyDeviceToHost, ctx->stream));
    }
  } else if (t.cs == t.C && t.co == 0) {
    KOCR_HIP(ctx, hipMemcpyAsync(dst, t.p, t.pixels() * row, hipMemcpyDeviceToHost, ctx->stream));
  } else {  // a channel slice of a wider buffer: the logical N x H x W x C tensor
    KOCR_HIP(ctx, hipMemcpy2DAsync(dst, row, t.p + t.co, (size_t)t.cs * sizeof(float), row, t.pixels(), hipMemcpyDeviceToHost,
                                   ctx->stream));
  }
  if (t.amax)  // non-negative floats as their bits
    KOCR_HIP(ctx, hipMemcpyAsync(pt.amax.data() + tp->n0, t.amax, (size_t)n * sizeof(unsigned), hipMemcpyDeviceToHost,
                                 ctx->stream));
  return KOCR_OK;
}

int set_taps(kocr_ctx* ctx, TapNet net, int n, const char* const* names, const char* fn) {
  if (!ctx || n < 0 || (n > 0 && !names)) return KOCR_EINVAL;
  ctx->tap_rows = nullptr;
  if (ctx->taps) {
    KOCR_HIP(ctx, hipSetDevice(ctx->device));
    KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    delete ctx->taps;
    ctx->taps = nullptr;
  }
  if (n == 0) return KOCR_OK;
  Taps* tp = new Taps();
  tp->net = net;
  for (int i = 0; i < n; ++i) {
    if (!names[i]) {
      delete tp;
      KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": null name");
    }
    if (!strcmp(names[i], "*")) tp->all = true;
    tp->sel.emplace_back(names[i]);
  }
  ctx->taps = tp;
  return KOCR_OK;
}

}  // namespace

int tap_begin(kocr_ctx* ctx, const std::string& name, const Tensor* in, Taps::Tap** out) {
  *out = nullptr;
  Taps* tp = ctx->taps;
  if (!tp || tp->n0 < 0 || !(tp->all || std::find(tp->sel.begin(), tp->sel.end(), name) != tp->sel.end())) return KOCR_OK;
  Taps::Tap* t = tp->find(name);
  if (!t) {
    if (tp->rec.size() == tp->rec.capacity()) KOCR_FAIL(ctx, KOCR_ECAPACITY, "taps: too many taps");
    tp->rec.emplace_back();
    t = &tp->rec.back();
    t->name = name;
  }
  if (in && in->p) KOCR_TRY(tap_copy(ctx, t->part[0], *in));
  t->rows.clear();
  ctx->tap_rows = &t->rows;
  *out = t;
  return KOCR_OK;
}

int tap_end(kocr_ctx* ctx, Taps::Tap* t, const Tensor* full, const Tensor* pool) {
  if (!t) return KOCR_OK;
  ctx->tap_rows = nullptr;
  if (full && full->p) KOCR_TRY(tap_copy(ctx, t->part[1], *full));
  if (pool && pool->p) KOCR_TRY(tap_copy(ctx, t->part[2], *pool));
  return KOCR_OK;
}

int taps_begin(kocr_ctx* ctx, TapNet net, int N) {
  ctx->tap_rows = nullptr;
  if (!ctx->taps || ctx->taps->net != net) return KOCR_OK;
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // no copy of the previous call is still in flight
  ctx->taps->rec.clear();
  ctx->taps->rec.reserve(64);
  ctx->taps->N = N;
  ctx->taps->n0 = -1;
  return KOCR_OK;
}

void taps_batch(kocr_ctx* ctx, TapNet net, int n0, int nb) {
  ctx->tap_rows = nullptr;
  if (ctx->taps && ctx->taps->net == net) {
    ctx->taps->n0 = n0;
    ctx->taps->nb = nb;
  }
}

void taps_free(kocr_ctx* ctx) {
  delete ctx->taps;
  ctx->taps = nullptr;
  ctx->tap_rows = nullptr;
}

extern "C" {

int kocr_craft_set_taps(kocr_ctx* ctx, int n, const char* const* names) {
  return set_taps(ctx, TAPS_CRAFT, n, names, "kocr_craft_set_taps");
}

int kocr_crnn_set_taps(kocr_ctx* ctx, int n, const char* const* names) {
  return set_taps(ctx, TAPS_CRNN, n, names, "kocr_crnn_set_taps");
}

int kocr_craft_tap_count(kocr_ctx* ctx) {
  if (!ctx) return KOCR_EINVAL;
  return ctx->taps ? (int)ctx->taps->rec.size() : 0;
}

int kocr_craft_tap_info(kocr_ctx* ctx, int i, char* name, char* kernel, int32_t* dims) {
  if (!ctx) return KOCR_EINVAL;
  if (!ctx->taps || i < 0 || i >= (int)ctx->taps->rec.size()) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_craft_tap_info: no such tap");
  const Taps::Tap& t = ctx->taps->rec[i];
  if (name) snprintf(name, 64, "%s", t.name.c_str());
  if (kernel) {
    std::string k;
    for (const std::string& r : t.rows) k += (k.empty() ? "" : "+") + r;
    snprintf(kernel, 256, "%s", k.c_str());
  }
  if (dims)
    for (int p = 0; p < 3; ++p) {
      const Taps::Part& pt = t.part[p];
      dims[p * 4 + 0] = pt.N;
      dims[p * 4 + 1] = pt.H;
      dims[p * 4 + 2] = pt.W;
      dims[p * 4 + 3] = pt.C;
    }
  return KOCR_OK;
}

int kocr_craft_get_tap(kocr_ctx* ctx, const char* name, int which, float* dst, float* amax_dst) {
  if (!ctx || !name || which < 0 || which > 2) return KOCR_EINVAL;
  Taps::Tap* t = ctx->taps ? ctx->taps->find(name) : nullptr;
  if (!t || !t->part[which].N) KOCR_FAIL(ctx, KOCR_EINVAL, std::string("kocr_craft_get_tap: nothing recorded for ") + name);
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const Taps::Part& pt = t->part[which];
  if (dst) memcpy(dst, pt.data.data(), pt.data.size() * sizeof(float));
  if (amax_dst) memcpy(amax_dst, pt.amax.data(), pt.amax.size() * sizeof(float));
  return KOCR_OK;
}

}  // extern "C"
