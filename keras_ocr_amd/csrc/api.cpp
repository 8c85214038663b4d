// api.cpp — the extern "C" surface declared in include/kocr.h (context, memory, profiler,
// and the entry points that wrap the graphs).  No torch types: plain pointers and sizes.
#include "abi.h"
#include "taps.h"
#include <cmath>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <set>
#include <unordered_map>

// ---------------------------------------------------------------------------------------
// ctx internals
// ---------------------------------------------------------------------------------------
// Device memory: every allocation of the library, for all contexts of the process, goes through this pair.  The sizes are kept
// by address, so that a free needs none (kocr_device_free has only the pointer).
namespace {
std::mutex g_mem_mu;
std::unordered_map<void*, size_t> g_mem_size;
std::atomic<uint64_t> g_mem_count{0}, g_mem_bytes{0};
}  // namespace

hipError_t kocr_counted_malloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> g(g_mem_mu);
  g_mem_size[*p] = bytes;
  g_mem_count += 1;
  g_mem_bytes += bytes;
  return e;
}

hipError_t kocr_counted_free(void* p) {
  if (!p) return hipSuccess;
  {  // forgotten before it is freed: the address may be handed out again at once
    std::lock_guard<std::mutex> g(g_mem_mu);
    auto it = g_mem_size.find(p);
    if (it != g_mem_size.end()) {
      g_mem_count -= 1;
      g_mem_bytes -= it->second;
      g_mem_size.erase(it);
    }
  }
  return hipFree(p);
}

// every arena given back (kocr_debug_release_arenas; kocr_load_crnn with another class count); the debug modes stay as set
static int release_arenas(kocr_ctx* ctx) {
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < kocr_ctx::N_ARENAS; ++i) {
    Arena& a = *ctx->arena_at(i);
    if (!a.guards.empty()) arena_guard_check(a);  // before the memory they lie in goes
    if (a.base) KOCR_HIP(ctx, kocr_counted_free(a.base));
    kocr_ctx *const gctx = a.gctx, *const pctx = a.pctx;
    const unsigned char pbyte = a.pbyte;
    a = Arena{};
    a.gctx = gctx;
    a.pctx = pctx;
    a.pbyte = pbyte;
  }
  ctx->invalidate_results();
  return KOCR_OK;
}

int arena_reserve(kocr_ctx* ctx, Arena& a, size_t bytes) {
  ctx->invalidate_results();  // whoever sizes an arena is about to overwrite it (the entry points re-validate at their end)
  a.requested = bytes;
  a.peak = 0;
  const size_t guard = a.gctx ? ARENA_GUARD_RESERVE : 0;  // guard mode: room for the guards, outside the plan
  if (bytes + guard <= a.cap) return KOCR_OK;
  if (a.base) {
    if (!a.guards.empty()) arena_guard_check(a);  // before the memory they lie in goes
    KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
    KOCR_HIP(ctx, kocr_counted_free(a.base));
    a.base = nullptr;
    a.cap = 0;
  }
  const size_t want = bytes + (bytes >> 3) + 4096 + guard;
  void* p = nullptr;
  hipError_t e = kocr_counted_malloc(&p, want);
  if (e != hipSuccess) {
    ctx->set_err("workspace allocation of " + std::to_string(want) + " B failed: " + hipGetErrorString(e));
    return KOCR_ENOMEM;
  }
  a.base = (char*)p;
  a.cap = want;
  a.reset();
  return KOCR_OK;
}

void arena_guard_fill(Arena& a, size_t at, size_t len) {
  kocr_ctx* ctx = a.gctx;
  if (hipMemsetAsync(a.base + at, ARENA_GUARD_FILL, len, ctx->stream) != hipSuccess) ctx->set_err("arena guard: hipMemsetAsync failed");
}

void arena_poison_fill(Arena& a, void* p, size_t bytes) {
  kocr_ctx* ctx = a.pctx;
  if (bytes && hipMemsetAsync(p, a.pbyte, bytes, ctx->stream) != hipSuccess) ctx->set_err("arena poison: hipMemsetAsync failed");
}

void arena_guard_check(Arena& a) {
  kocr_ctx* ctx = a.gctx;
  std::vector<ArenaGuard> list;
  list.swap(a.guards);
  if (!ctx || list.empty()) return;
  int index = -1;
  for (int i = 0; i < kocr_ctx::N_ARENAS; ++i)
    if (ctx->arena_at(i) == &a) index = i;
  std::vector<unsigned char> copy;
  bool ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
  for (const ArenaGuard& g : list) {
    copy.assign(g.len, 0);
    ok = ok && hipMemcpy(copy.data(), a.base + g.at, g.len, hipMemcpyDeviceToHost) == hipSuccess;
    const long bad = ok ? arena_guard_damage(copy.data(), g.len) : 0;  // a guard that cannot be read counts as damaged
    if (bad < 0) continue;
    if (ctx->guard_damage.count++ == 0) {
      ctx->guard_damage.arena = index;
      ctx->guard_damage.offset = g.buf;
      ctx->guard_damage.byte = g.at + (size_t)bad;
    }
  }
}

int kocr_ctx::ws_reserve(size_t bytes) { return arena_reserve(this, ws, bytes); }

int kocr_ctx::amax_begin() {
  if (!d_amax) {
    void* d = nullptr;
    KOCR_TRY(dev_alloc(&d, AMAX_SLOTS * sizeof(unsigned)));
    d_amax = (unsigned*)d;
  }
  amax_used = 0;
  KOCR_HIP(this, hipMemsetAsync(d_amax, 0, AMAX_SLOTS * sizeof(unsigned), stream));
  return KOCR_OK;
}

// Only the fp16 kernels read a tensor's tracked max |x| (their exact power-of-two input scale); in bf16x3 mode no slot is
// handed out, so the producers' epilogues skip the reduction and the atomic altogether.
unsigned* kocr_ctx::amax_slots(int n) {
  if (split_mode == KOCR_SPLIT_BF16X3 || !d_amax || n <= 0 || amax_used + n > AMAX_SLOTS) return nullptr;
  unsigned* s = d_amax + amax_used;
  amax_used += n;
  return s;
}

void kocr_note_dispatch(const char* family, const ConvLayer& L, const Tensor& in) {
  static const char* path = getenv("KOCR_DISPATCH_LOG");
  if (!path) return;
  static std::mutex mu;
  static std::set<std::string> seen;
  char line[256];
  snprintf(line, sizeof line, "%-14s %-28s N %d H %d W %d Cin %d Cout %d k %dx%d dil %d%s", family, L.name.c_str(), in.N, in.H, in.W, L.Cin,
           L.Cout, L.KH, L.KW, L.dil, in.cellW ? " cells" : "");
  std::lock_guard<std::mutex> g(mu);
  if (!seen.insert(line).second) return;
  if (FILE* f = fopen(path, "a")) {
    fprintf(f, "%s\n", line);
    fclose(f);
  }
}

int kocr_ctx::upload(float** out, const std::vector<float>& host) {
  void* p = nullptr;
  KOCR_TRY(dev_alloc(&p, host.size() * sizeof(float)));
  KOCR_HIP(this, hipMemcpy(p, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
  *out = (float*)p;
  return KOCR_OK;
}

hipEvent_t kocr_ctx::get_event() {
  if (!ev_pool.empty()) {
    hipEvent_t e = ev_pool.back();
    ev_pool.pop_back();
    return e;
  }
  hipEvent_t e;
  hipEventCreate(&e);
  return e;
}

void kocr_ctx::prof_begin(const char* name, double flops, double bytes) {
  // bounded: a caller that leaves profiling on without ever asking for the report pays one synchronisation per 4096
  // launches instead of an event pool that grows without limit
  if (pending.size() >= 4096) prof_flush();
  Pending pd;
  pd.name = name;
  pd.a = get_event();
  pd.b = get_event();
  hipEventRecord(pd.a, stream);
  pending.push_back(pd);
  ProfRow& r = prof[name];
  r.launches += 1;
  r.flops += flops;
  r.bytes += bytes;
}

void kocr_ctx::prof_end() { hipEventRecord(pending.back().b, stream); }

int kocr_ctx::prof_flush() {
  if (pending.empty()) return KOCR_OK;
  KOCR_HIP(this, hipStreamSynchronize(stream));
  for (Pending& pd : pending) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, pd.a, pd.b);
    prof[pd.name].ms += ms;
    ev_pool.push_back(pd.a);
    ev_pool.push_back(pd.b);
  }
  pending.clear();
  return KOCR_OK;
}

int craft_micro_batch(int micro_batch, int N, int H, int W) {
  int mb = micro_batch > 0 ? micro_batch : 32;
  while (mb > 1 && craft_workspace_bytes(mb, H, W) > ((size_t)96 << 30)) mb = (mb + 1) / 2;
  return std::min(mb, N);
}

int warp_status_error(kocr_ctx* ctx, const char* fn, int status, const char* at) {
  if (status == 1) KOCR_FAIL(ctx, KOCR_EZERODIV, std::string(fn) + ": box with zero width or height (" + at + ")");
  if (status != 0) KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": singular perspective transform");
  return KOCR_OK;
}

long prepare_box_warps(kocr_ctx* ctx, const char* fn, int N, const float* boxes, const int32_t* counts, const void* out, int th,
                       int tw, std::vector<WarpParam>& prm) {
  const std::string f(fn);
  long M = 0;
  for (int i = 0; i < N; ++i) {
    if (counts[i] < 0) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": negative count");
    M += counts[i];
  }
  if (M == 0) return 0;
  if (!boxes || !out) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null buffer");
  prm.resize((size_t)M);
  long m = 0;
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < counts[i]; ++j, ++m) {
      KOCR_TRY(warp_status_error(ctx, fn, warp_prepare(boxes + m * 8, th, tw, &prm[m], nullptr)));
      prm[m].img = i;
    }
  return M;
}

// The targets of a CTC loss as the caller gives them (HOST; validated by ctc_validate, which gives Lmax) and where the losses
// [M] go
struct CtcTargets {
  const int32_t* labels;
  int stride;
  const int32_t* lengths;
  const int32_t* input_lengths;
  float* loss;
  int Lmax = 0;
  int row() const { return std::max(Lmax, 1); }                                   // columns of a staged label row
  size_t staged_bytes() const { return (size_t)(row() + 2) * sizeof(int32_t); }  // per sample
};
// Rows [s, s + nb) of the targets in the workspace as [nb][row()] | len[nb] | in_len[nb]: `dev`.  `host` is the staging
// vector: it has to outlive the asynchronous copy (the callers synchronise before it is reused or goes out of scope).
struct CtcStaged {
  std::vector<int32_t> host;
  CtcLabels dev;
};
static int ctc_stage_labels(Staging& st, const CtcTargets& tg, long s, int nb, CtcStaged& out) {
  const int ls = tg.row();
  out.host.assign((size_t)nb * (ls + 2), -1);
  for (int i = 0; i < nb; ++i) {
    const long m = s + i;
    for (int k = 0; k < tg.lengths[m]; ++k) out.host[(size_t)i * ls + k] = tg.labels[(size_t)m * tg.stride + k];
    out.host[(size_t)nb * ls + i] = tg.lengths[m];
    out.host[(size_t)nb * (ls + 1) + i] = tg.input_lengths[m];
  }
  const int32_t* d;
  KOCR_TRY(st.upload(out.host.data(), out.host.size() * sizeof(int32_t), d));
  out.dev = {d, ls, d + (size_t)nb * ls, d + (size_t)nb * (ls + 1), tg.Lmax};
  return KOCR_OK;
}

// The staged call behind every recogniser entry point that decodes: kocr_crnn_forward / _forward_scores / _beam / _lexicon /
// _pattern from crops, kocr_crnn_decode_logits / _charsets / _patterns from logits.  The entry validates its arguments, states
// them as a request on the caller's buffers (CrnnDecode; cm is the driver's) and names what else its family has:
struct CrnnSource {
  const float* p;  // the caller's crops [M][31][200] (any M, batch by batch; device with on_device) ...
  bool logits;     // ... or fc_12's logits [M][50][C] (HOST, at most one batch; with them the decode alone runs)
};
struct CrnnExtras {
  // The output and host-list arguments of the entry.  The plan counts 256 bytes for each, given or null, as Staging::reserve does
  // for an empty buffer.
  int slots = 0, lists = 0;
  size_t workspace = 0;              // lexicon_workspace_bytes / pattern_workspace_bytes of the call, where it has them
  bool taps = false;                 // the call records the taps of kocr_crnn_set_taps
  const int32_t* set_of = nullptr;   // HOST [M]: the crops' character sets in place of the context's switch
  const CtcTargets* loss = nullptr;  // logits only: the loss launch on the same logits, behind the decode
};
// Workspace for crnn_batch(M) crops; per batch: the lists (set_of, the request's pt.of) and the source in, a buffer per output
// of the request -- CrnnDecode::each is the one list of them and of their sizes --, the launches, every output back.
static int crnn_call(kocr_ctx* ctx, const char* fn, CrnnSource src, int M, const CrnnDecode& host, bool on_device, const CrnnExtras& x) {
  if (M == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int mb = crnn_batch(M), LW = crnn_label_width(ctx), C = crnn_classes(ctx), V = ctx->lex.V;
  const size_t i4 = sizeof(int32_t), f4 = sizeof(float), src_n = src.logits ? (size_t)CRNN_STEPS * C : CRNN_CROP_PIXELS;
  size_t staged = src_n * f4 * mb + 256 + 256 * (size_t)x.slots, always = 256 * (size_t)x.lists;
  CrnnDecode(host).each(LW, C, V, [&](auto*&, size_t b) {
    staged += b * mb;
    return KOCR_OK;
  });
  if (x.loss) staged += f4 * mb, always += x.loss->staged_bytes() * mb;
  always += ((x.set_of ? i4 : 0) + (host.pt.of ? i4 : 0)) * mb;
  Staging st{ctx, ctx->ws, fn, on_device};
  KOCR_TRY(st.reserve((src.logits ? 0 : crnn_workspace_bytes(mb, C)) + x.workspace + (on_device ? 0 : staged) + always, {}));
  CtcStaged tg;
  auto batch = [&](long s, int nb) -> int {
    if (x.taps) taps_batch(ctx, TAPS_CRNN, (int)s, nb);
    const CrnnDecode h = host.from(s, LW, C, V);  // the caller's rows of this batch
    CrnnDecode d = h;                             // ... and the device's; its lists are the batch's own, entry 0 its crop 0
    const int32_t* d_set = nullptr;
    if (x.set_of) KOCR_TRY(st.upload(x.set_of + s, i4 * nb, d_set));
    d.cm = ctx->charmask(d_set, 0);
    d.pt.first = 0;
    if (h.pt.of) {
      d.pt.of = h.pt.of + s;
      KOCR_TRY(st.upload(d.pt.of, i4 * nb, d.pt.d_of));
    }
    const float* d_src;
    KOCR_TRY(st.in(src.p + s * src_n, src_n * f4 * nb, d_src));
    void* dev[CrnnDecode::MAX_OUTPUTS];
    int n = 0;
    KOCR_TRY(d.each(LW, C, V, [&](auto*& p, size_t b) -> int {
      KOCR_TRY(st.out(p, b * nb, p));
      dev[n++] = p;
      return KOCR_OK;
    }));
    KOCR_TRY(src.logits ? crnn_decode_logits(ctx, d_src, nb, d) : crnn_forward(ctx, d_src, nb, d));
    n = 0;
    KOCR_TRY(CrnnDecode(h).each(LW, C, V, [&](auto*& p, size_t b) {
      return st.back(p, (std::remove_reference_t<decltype(p)>)dev[n++], b * nb);
    }));
    if (x.loss) {
      float* d_loss;
      KOCR_TRY(ctc_stage_labels(st, *x.loss, s, nb, tg));
      KOCR_TRY(st.out(x.loss->loss + s, f4 * nb, d_loss));
      KOCR_TRY(crnn_logits_loss(ctx, d_src, nb, tg.dev, d_loss));
      KOCR_TRY(st.back(x.loss->loss + s, d_loss, f4 * nb));
    }
    return st.finish();  // also: `tg` is reused or gone only after its copy
  };
  if (!x.taps) return crnn_batches(ctx, M, batch);
  KOCR_TRY(taps_begin(ctx, TAPS_CRNN, M));
  TapsEnd taps_end{ctx, TAPS_CRNN};
  return crnn_batches(ctx, M, batch);
}

// ---------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------
extern "C" {

int kocr_create(kocr_ctx** out, int hip_device) {
  if (!out) return KOCR_EINVAL;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || hip_device < 0 || hip_device >= count) return KOCR_EHIP;
  if (hipSetDevice(hip_device) != hipSuccess) return KOCR_EHIP;
  kocr_ctx* c = new kocr_ctx();
  if (const char* e = getenv("KOCR_SPLIT"))
    c->split_mode = (!strcmp(e, "f16") || !strcmp(e, "fp16") || !strcmp(e, "f16x2")) ? KOCR_SPLIT_F16X2
                    : (!strcmp(e, "f16x1") || !strcmp(e, "fast"))                     ? KOCR_SPLIT_F16X1
                                                                                      : KOCR_SPLIT_BF16X3;
  {
    auto on = [](const char* name, bool dflt) {
      const char* e = getenv(name);
      return e ? atoi(e) != 0 : dflt;
    };
    c->sw.dense_splitk = on("KOCR_DENSE_SPLITK", true);
    c->sw.lstm16 = on("KOCR_LSTM16", true);
    c->sw.hs16 = on("KOCR_HS16", true);
    c->sw.k5 = on("KOCR_K5", true);
    c->sw.up2x = on("KOCR_UP2X", true);
    c->sw.w43h = on("KOCR_W43H", true);
    c->sw.w43 = on("KOCR_W43", true);
    c->sw.w43r = on("KOCR_W43R", true);
    c->sw.w43v = on("KOCR_W43V", true);
    c->sw.w43rag = on("KOCR_W43RAG", true);
    c->sw.w43dilh = on("KOCR_W43DILH", true);
    c->sw.cells = on("KOCR_CELLS", true);
    c->sw.wsplit = on("KOCR_WSPLIT", true);
    c->sw.dsplit = on("KOCR_DSPLIT", true);
    c->sw.hsplit = on("KOCR_HSPLIT", true);
    c->sw.first = on("KOCR_FIRST", true);
  }
  c->prof_layers = getenv("KOCR_PROF_LAYERS") != nullptr;
  if (const char* e = getenv("KOCR_LINFOLD")) c->opt_linfold = atoi(e) != 0;
  if (const char* e = getenv("KOCR_UPFOLD")) c->opt_upfold = atoi(e) != 0;
  c->device = hip_device;
  if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, hip_device) != hipSuccess ||
      hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return KOCR_EHIP;
  }
  c->stream = c->own_stream;
  *out = c;
  return KOCR_OK;
}

void kocr_destroy(kocr_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  hipStreamSynchronize(ctx->stream);
  craft_free(ctx);
  crnn_free(ctx);
  ctx->release_since(0);
  for (Arena* a : {&ctx->ws, &ctx->pp, &ctx->pp2, &ctx->io, &ctx->pl, &ctx->bx, &ctx->chw, &ctx->chr}) kocr_counted_free(a->base);
  for (auto& pd : ctx->pending) {
    hipEventDestroy(pd.a);
    hipEventDestroy(pd.b);
  }
  for (hipEvent_t e : ctx->ev_pool) hipEventDestroy(e);
  hipStreamDestroy(ctx->own_stream);
  delete ctx;
}

const char* kocr_last_error(const kocr_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int kocr_set_stream(kocr_ctx* ctx, void* hip_stream) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
  return KOCR_OK;
}

int kocr_synchronize(kocr_ctx* ctx) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

int kocr_device_alloc(kocr_ctx* ctx, void** out, uint64_t bytes) {
  if (!ctx || !out) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  KOCR_HIP(ctx, kocr_counted_malloc(out, bytes ? bytes : 4));
  return KOCR_OK;
}

int kocr_device_free(kocr_ctx* ctx, void* p) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  KOCR_HIP(ctx, kocr_counted_free(p));
  return KOCR_OK;
}

int kocr_memcpy_h2d(kocr_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

int kocr_memcpy_d2h(kocr_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

int kocr_load_craft(kocr_ctx* ctx, int n, const char* const* names, const float* const* data,
                    const int64_t* shapes, const int* ranks) {
  if (!ctx || n <= 0 || !names || !data || !shapes || !ranks) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  return craft_load(ctx, n, names, data, shapes, ranks);
}

int kocr_craft_forward(kocr_ctx* ctx, const void* img, int dtype, int N, int H, int W, float* heat,
                       int micro_batch, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || (N > 0 && (!img || !heat))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_craft_forward: null buffer");
  if (dtype != KOCR_U8 && dtype != KOCR_F32) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_craft_forward: bad dtype");
  if (N == 0) return KOCR_OK;
  if (!craft_loaded(ctx)) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_craft_forward: call kocr_load_craft first");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int mb = craft_micro_batch(micro_batch, N, H, W);
  const size_t in_img = (size_t)H * W * 3 * (dtype == KOCR_U8 ? 1 : 4);
  const size_t out_img = (size_t)(H / 2) * (W / 2) * 2 * sizeof(float);
  Staging st{ctx, ctx->ws, "kocr_craft_forward", on_device != 0};
  KOCR_TRY(st.reserve(craft_workspace_bytes(mb, H, W), {in_img * mb, out_img * mb}));
  KOCR_TRY(taps_begin(ctx, TAPS_CRAFT, N));
  TapsEnd taps_end{ctx, TAPS_CRAFT};
  return craft_batches(ctx, micro_batch, N, H, W, [&](int s, int nb) -> int {
    taps_batch(ctx, TAPS_CRAFT, s, nb);
    const void* d_in;
    float* d_out;
    float* h_out = (float*)((char*)heat + (size_t)s * out_img);
    KOCR_TRY(st.in((const void*)((const char*)img + (size_t)s * in_img), in_img * nb, d_in));
    KOCR_TRY(st.out(h_out, out_img * nb, d_out));
    KOCR_TRY(craft_forward(ctx, d_in, dtype, nb, H, W, d_out));
    KOCR_TRY(st.back(h_out, d_out, out_img * nb));
    return st.finish();
  });
}

int kocr_load_crnn(kocr_ctx* ctx, int n, const char* const* names, const float* const* data,
                   const int64_t* shapes, const int* ranks) {
  if (!ctx || n <= 0 || !names || !data || !shapes || !ranks) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int before = crnn_classes(ctx);
  KOCR_TRY(crnn_load(ctx, n, names, data, shapes, ranks));
  // the arenas were sized for the previous class count (logits, probabilities): a recogniser of fewer classes would keep them
  // for ever.  Given back here, they grow again to what this one asks for -- the state of a fresh context.
  if (before && before != crnn_classes(ctx)) KOCR_TRY(release_arenas(ctx));
  // a lexicon's labels were validated against the class count of the recogniser it was loaded under
  if (ctx->lex.V && ctx->lex.classes != crnn_classes(ctx)) lexicon_unload(ctx, ctx->lex.classes);
  // ... and so were the character sets' class indices
  if (ctx->charsets.S && ctx->charsets.classes != crnn_classes(ctx)) charsets_unload(ctx);
  // ... and the patterns' transition tables
  if (ctx->patterns.P && ctx->patterns.classes != crnn_classes(ctx)) patterns_unload(ctx);
  return KOCR_OK;
}

int kocr_crnn_classes(kocr_ctx* ctx) { return ctx ? crnn_classes(ctx) : KOCR_EINVAL; }
int kocr_crnn_label_width(kocr_ctx* ctx) { return ctx ? crnn_label_width(ctx) : KOCR_EINVAL; }
int kocr_crnn_set_rnn_steps_to_discard(kocr_ctx* ctx, int steps) { return ctx ? crnn_set_discard(ctx, steps) : KOCR_EINVAL; }

// kocr_crnn_forward, and with log_word / char_scores kocr_crnn_forward_scores (`fn`: the one that was called): the same
// batches, with the score buffers ctc_scores_kernel as the last launch
static int crnn_forward_call(kocr_ctx* ctx, const char* fn, const float* crops, int M, const CrnnDecode& rq, int on_device) {
  const std::string f(fn);
  if (M < 0 || (M > 0 && (!crops || !rq.d_labels))) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null buffer");
  if (crnn_classes(ctx) == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, f + ": call kocr_load_crnn first");
  CrnnExtras x;
  x.slots = 4;
  x.taps = true;
  return crnn_call(ctx, fn, {crops, false}, M, rq, on_device != 0, x);
}

int kocr_crnn_forward(kocr_ctx* ctx, const float* crops, int M, int32_t* labels, float* probs, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  CrnnDecode rq;
  rq.greedy = true;
  rq.d_labels = labels;
  rq.d_probs = probs;
  return crnn_forward_call(ctx, "kocr_crnn_forward", crops, M, rq, on_device);
}

// kocr_crnn_forward with the scores of include/kocr.h ("Scores")
int kocr_crnn_forward_scores(kocr_ctx* ctx, const float* crops, int M, int32_t* labels, float* probs, float* log_word,
                             float* char_scores, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (M > 0 && (!log_word || !char_scores)) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_crnn_forward_scores: null buffer");
  CrnnDecode rq;
  rq.greedy = true;
  rq.d_labels = labels;
  rq.d_probs = probs;
  rq.sc = {log_word != nullptr, log_word, char_scores};
  return crnn_forward_call(ctx, "kocr_crnn_forward_scores", crops, M, rq, on_device);
}

// The beam search of include/kocr.h ("Beam search") alone: the forward up to fc_12, then ctc_beam_kernel
int kocr_crnn_beam(kocr_ctx* ctx, const float* crops, int M, int beam_width, int top_paths, int32_t* labels, float* log_prob,
                   int on_device) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_TRY(beam_validate(ctx, "kocr_crnn_beam", beam_width, top_paths));
  if (M < 0 || (M > 0 && (!crops || !labels || !log_prob))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_crnn_beam: null buffer");
  if (crnn_classes(ctx) == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_crnn_beam: call kocr_load_crnn first");
  CrnnDecode rq;
  rq.bm = {beam_width, top_paths, labels, log_prob};
  CrnnExtras x;
  x.slots = 2;
  return crnn_call(ctx, "kocr_crnn_beam", {crops, false}, M, rq, on_device != 0, x);
}

// ---- lexicon (include/kocr.h, "Lexicon") --------------------------------------------------------------------------------
int kocr_set_lexicon(kocr_ctx* ctx, const int32_t* words, int stride, const int32_t* lengths, int V) {
  if (!ctx) return KOCR_EINVAL;
  if (V < 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_lexicon: V " + std::to_string(V) + " is negative");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  if (V == 0) {
    lexicon_unload(ctx, 0);
    return KOCR_OK;
  }
  if (!words || !lengths || stride < 1) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_lexicon: null buffer or stride < 1");
  const int C = crnn_classes(ctx);
  if (C == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_set_lexicon: call kocr_load_crnn first (the labels are checked against its classes)");
  int Lmax = 0;
  for (int v = 0; v < V; ++v) {
    const int L = lengths[v];
    if (L < 1 || L > KOCR_LEXICON_MAX_WORD || L > stride)
      KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_lexicon: lengths: word " + std::to_string(v) + " has length " + std::to_string(L) +
                                      " outside [1, min(KOCR_LEXICON_MAX_WORD = " + std::to_string(KOCR_LEXICON_MAX_WORD) +
                                      ", stride = " + std::to_string(stride) + ")]");
    for (int i = 0; i < L; ++i) {
      const int c = words[(size_t)v * stride + i];
      if (c < 0 || c > C - 2)
        KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_lexicon: words: word " + std::to_string(v) + ": label " + std::to_string(c) +
                                        " at position " + std::to_string(i) + " outside [0, " + std::to_string(C - 2) +
                                        "] (the blank is " + std::to_string(C - 1) + ")");
    }
    Lmax = std::max(Lmax, L);
  }
  // rows of Lmax labels; the words by ascending length (stable: equal lengths keep the caller's order)
  std::vector<int32_t> rows((size_t)V * Lmax, -1), order(V);
  for (int v = 0; v < V; ++v) {
    std::copy(words + (size_t)v * stride, words + (size_t)v * stride + lengths[v], rows.begin() + (size_t)v * Lmax);
    order[v] = v;
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return lengths[a] < lengths[b]; });
  lexicon_unload(ctx, 0);
  auto& lex = ctx->lex;
  auto put = [&](int** d, const int32_t* h, size_t n) -> int {
    KOCR_TRY(ctx->dev_alloc((void**)d, n * sizeof(int32_t)));
    KOCR_HIP(ctx, hipMemcpyAsync(*d, h, n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    return KOCR_OK;
  };
  int rc = put(&lex.d_words, rows.data(), rows.size());
  if (rc == KOCR_OK) rc = put(&lex.d_lens, lengths, V);
  if (rc == KOCR_OK) rc = put(&lex.d_order, order.data(), V);
  hipStreamSynchronize(ctx->stream);  // the host vectors go out of scope
  if (rc != KOCR_OK) {
    lexicon_unload(ctx, 0);
    return rc;
  }
  lex.V = V;
  lex.Lmax = Lmax;
  lex.classes = C;
  return KOCR_OK;
}

int kocr_lexicon_size(const kocr_ctx* ctx) { return ctx ? ctx->lex.V : KOCR_EINVAL; }

int kocr_set_lexicon_scratch(kocr_ctx* ctx, uint64_t bytes) {
  if (!ctx) return KOCR_EINVAL;
  ctx->lex_scratch = bytes ? (size_t)bytes : kocr_ctx::LEX_SCRATCH_DEFAULT;
  return KOCR_OK;
}

// The lexicon match of include/kocr.h ("Lexicon") alone: the forward up to fc_12, then the three lexicon launches
int kocr_crnn_lexicon(kocr_ctx* ctx, const float* crops, int M, int top_words, int32_t* index, float* log_prob, float* all_values,
                      int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (top_words < 1 || top_words > 64) KOCR_TRY(lexicon_validate(ctx, "kocr_crnn_lexicon", top_words));
  if (M < 0 || (M > 0 && (!crops || !index || !log_prob))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_crnn_lexicon: null buffer");
  if (crnn_classes(ctx) == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_crnn_lexicon: call kocr_load_crnn first");
  KOCR_TRY(lexicon_validate(ctx, "kocr_crnn_lexicon", top_words));
  CrnnDecode rq;
  rq.lx = {top_words, index, log_prob, all_values};
  CrnnExtras x;
  x.slots = 3;
  x.workspace = lexicon_workspace_bytes(ctx, crnn_batch(M), !all_values);
  return crnn_call(ctx, "kocr_crnn_lexicon", {crops, false}, M, rq, on_device != 0, x);
}

int kocr_ctc_batch_cost(kocr_ctx* ctx, const float* y_pred, int M, int T, int C, const int32_t* labels, int label_stride,
                        const int32_t* label_lengths, const int32_t* input_lengths, float* loss, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  const char* fn = "kocr_ctc_batch_cost";
  if (M < 0 || T < 1 || C < 1 || label_stride < 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_ctc_batch_cost: bad sizes");
  if (M > 0 && (!y_pred || !labels || !label_lengths || !input_lengths || !loss))
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_ctc_batch_cost: null buffer");
  CtcTargets tg{labels, label_stride, label_lengths, input_lengths, loss};
  KOCR_TRY(ctc_validate(ctx, fn, M, T, C, labels, label_stride, label_lengths, input_lengths, &tg.Lmax));
  if (M == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t yb = (size_t)M * T * C * sizeof(float), lb = (size_t)M * sizeof(float);
  Staging st{ctx, ctx->ws, fn, on_device != 0};
  KOCR_TRY(st.reserve(0, {yb, lb}, {tg.staged_bytes() * M}));
  CtcStaged staged;
  KOCR_TRY(ctc_stage_labels(st, tg, 0, M, staged));
  const float* d_y;
  float* d_loss;
  KOCR_TRY(st.in(y_pred, yb, d_y));
  KOCR_TRY(st.out(loss, lb, d_loss));
  const CtcLabels& lab = staged.dev;
  KOCR_TRY(launch_ctc_loss(ctx, /*logits=*/false, d_y, M, T, C, 0, lab.d_lab, lab.lstride, lab.d_len, lab.d_in_len, d_loss, lab.Lmax));
  KOCR_TRY(st.back(loss, d_loss, lb));
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `staged` goes out of scope
  return KOCR_OK;
}

int kocr_crnn_ctc_loss(kocr_ctx* ctx, const float* crops, int M, const int32_t* labels, int label_stride,
                       const int32_t* label_lengths, const int32_t* input_lengths, float* loss, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  const char* fn = "kocr_crnn_ctc_loss";
  if (M < 0 || label_stride < 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_crnn_ctc_loss: bad sizes");
  if (M > 0 && (!crops || !labels || !label_lengths || !input_lengths || !loss))
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_crnn_ctc_loss: null buffer");
  const int C = crnn_classes(ctx);
  if (C == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_crnn_ctc_loss: call kocr_load_crnn first");
  const int LW = crnn_label_width(ctx);
  CtcTargets tg{labels, label_stride, label_lengths, input_lengths, loss};
  KOCR_TRY(ctc_validate(ctx, fn, M, LW, C, labels, label_stride, label_lengths, input_lengths, &tg.Lmax));
  if (M == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int mb = crnn_batch(M);
  const size_t cb = CRNN_CROP_PIXELS * sizeof(float);
  Staging st{ctx, ctx->ws, fn, on_device != 0};
  KOCR_TRY(st.reserve(crnn_workspace_bytes(mb, C), {cb * mb, sizeof(float) * mb}, {tg.staged_bytes() * mb}));
  CtcStaged staged;
  return crnn_batches(ctx, M, [&](long s, int nb) -> int {
    KOCR_TRY(ctc_stage_labels(st, tg, s, nb, staged));
    const float* d_c;
    float* d_loss;
    KOCR_TRY(st.in(crops + s * CRNN_CROP_PIXELS, cb * nb, d_c));
    KOCR_TRY(st.out(loss + s, sizeof(float) * nb, d_loss));
    KOCR_TRY(crnn_ctc_loss(ctx, d_c, nb, staged.dev, d_loss));
    KOCR_TRY(st.back(loss + s, d_loss, sizeof(float) * nb));
    KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));  // `staged` is reused by the next batch
    return KOCR_OK;
  });
}

// ---- character sets (include/kocr.h, "Character sets") ------------------------------------------------------------------
int kocr_set_charsets(kocr_ctx* ctx, const uint8_t* allowed, int S, int classes) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  if (S == 0) {
    charsets_unload(ctx);
    return KOCR_OK;
  }
  const int C = crnn_classes(ctx);
  if (C == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_set_charsets: call kocr_load_crnn first (the sets are subsets of its classes)");
  if (S < 0 || S > KOCR_CHARSETS_MAX)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_charsets: S " + std::to_string(S) + " outside [0, KOCR_CHARSETS_MAX = " +
                                    std::to_string(KOCR_CHARSETS_MAX) + "]");
  if (classes != C)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_charsets: classes " + std::to_string(classes) + " is not the recogniser's " +
                                    std::to_string(C) + " (class count mismatch)");
  if (!allowed) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_charsets: null buffer");
  // the bit table: bit c of set s for an allowed class, the blank's bit always, the bits from C on clear
  const int nw = (C + 31) / 32;
  std::vector<uint32_t> bits((size_t)S * nw, 0u);
  for (int s = 0; s < S; ++s) {
    int n = 0;
    for (int c = 0; c < C - 1; ++c)
      if (allowed[(size_t)s * (C - 1) + c]) {
        bits[(size_t)s * nw + (c >> 5)] |= 1u << (c & 31);
        ++n;
      }
    if (n == 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_charsets: allowed: set " + std::to_string(s) + " is empty (a set needs at least one class)");
    bits[(size_t)s * nw + ((C - 1) >> 5)] |= 1u << ((C - 1) & 31);
  }
  charsets_unload(ctx);
  auto& cs = ctx->charsets;
  int rc = ctx->dev_alloc((void**)&cs.d_bits, bits.size() * sizeof(uint32_t));
  if (rc == KOCR_OK && hipMemcpyAsync(cs.d_bits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
    ctx->set_err("kocr_set_charsets: the copy of the table failed");
    rc = KOCR_EHIP;
  }
  hipStreamSynchronize(ctx->stream);  // the host vector goes out of scope
  if (rc != KOCR_OK) {
    charsets_unload(ctx);
    return rc;
  }
  cs.S = S;
  cs.classes = C;
  return KOCR_OK;
}

int kocr_charset_count(const kocr_ctx* ctx) { return ctx ? ctx->charsets.S : KOCR_EINVAL; }

int kocr_set_charset(kocr_ctx* ctx, int set) {
  if (!ctx) return KOCR_EINVAL;
  if (set < -1 || set >= ctx->charsets.S)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_charset: set " + std::to_string(set) + " outside [-1, " + std::to_string(ctx->charsets.S) +
                                    ") (" + std::to_string(ctx->charsets.S) + " sets are loaded: kocr_set_charsets)");
  ctx->charset = set;
  return KOCR_OK;
}

int kocr_get_charset(const kocr_ctx* ctx, int* set) {
  if (!ctx || !set) return KOCR_EINVAL;
  *set = ctx->charset;
  return KOCR_OK;
}

// ---- patterns (include/kocr.h, "Patterns") -------------------------------------------------------------------------------
int kocr_set_patterns(kocr_ctx* ctx, const int32_t* delta, const uint8_t* accept, const int32_t* n_states, int P, int classes) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  if (P == 0) {
    patterns_unload(ctx);
    return KOCR_OK;
  }
  const int C = crnn_classes(ctx);
  if (C == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_set_patterns: call kocr_load_crnn first (the transitions are over its classes)");
  if (P < 0 || P > KOCR_PATTERNS_MAX)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_patterns: P " + std::to_string(P) + " outside [0, KOCR_PATTERNS_MAX = " +
                                    std::to_string(KOCR_PATTERNS_MAX) + "]");
  if (classes != C)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_patterns: classes " + std::to_string(classes) + " is not the recogniser's " + std::to_string(C) +
                                    " (class count mismatch)");
  if (C - 1 >= 0xffff) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_patterns: more than 65535 classes");
  if (!delta || !accept || !n_states) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_patterns: null buffer");
  const int K = C - 1;
  std::vector<int32_t> hdr((size_t)P * 8, 0), pred;
  std::vector<int2> nodes, states;
  std::vector<int> Sv(P), NTv(P);
  size_t row0 = 0;
  for (int p = 0; p < P; ++p) {
    const std::string sp = "pattern " + std::to_string(p);
    const int S = n_states[p];
    if (S < 1 || S > KOCR_PATTERN_MAX_STATES)
      KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_patterns: n_states: " + sp + " has " + std::to_string(S) +
                                      " states, outside [1, KOCR_PATTERN_MAX_STATES = " + std::to_string(KOCR_PATTERN_MAX_STATES) + "]");
    const int32_t* d = delta + row0 * K;
    const uint8_t* a = accept + row0;
    // the transitions in range; the label nodes: (s, c) for every c that enters s
    std::vector<std::vector<int>> in((size_t)S * K);  // [s][c] -> the p with delta[p][c] == s, ascending
    for (int q = 0; q < S; ++q)
      for (int c = 0; c < K; ++c) {
        const int to = d[(size_t)q * K + c];
        if (to < -1 || to >= S)
          KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_patterns: delta: " + sp + ": state " + std::to_string(q) + ", class " + std::to_string(c) +
                                          " moves to " + std::to_string(to) + " outside [-1, " + std::to_string(S) + ")");
        if (to >= 0) in[(size_t)to * K + c].push_back(q);
      }
    // trimmed: every state reachable from state 0 and able to reach an accepting state
    std::vector<char> fwd(S, 0), bwd(S, 0);
    std::vector<int> stack{0};
    fwd[0] = 1;
    while (!stack.empty()) {
      const int q = stack.back();
      stack.pop_back();
      for (int c = 0; c < K; ++c) {
        const int to = d[(size_t)q * K + c];
        if (to >= 0 && !fwd[to]) {
          fwd[to] = 1;
          stack.push_back(to);
        }
      }
    }
    for (int q = 0; q < S; ++q)
      if (a[q]) {
        bwd[q] = 1;
        stack.push_back(q);
      }
    while (!stack.empty()) {
      const int q = stack.back();
      stack.pop_back();
      for (int c = 0; c < K; ++c)
        for (int from : in[(size_t)q * K + c])
          if (!bwd[from]) {
            bwd[from] = 1;
            stack.push_back(from);
          }
    }
    for (int q = 0; q < S; ++q)
      if (!fwd[q] || !bwd[q])
        KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_patterns: " + sp + " is not trimmed: state " + std::to_string(q) +
                                        (fwd[q] ? " reaches no accepting state" : " is not reachable from state 0"));
    hdr[(size_t)p * 8 + 2] = (int)nodes.size();
    hdr[(size_t)p * 8 + 3] = (int)states.size();
    hdr[(size_t)p * 8 + 4] = (int)pred.size();
    const int node0 = (int)nodes.size(), pred0 = (int)pred.size();
    int n_label = 0;
    for (int q = 0; q < S; ++q) {
      states.push_back(make_int2((int)nodes.size() - node0, a[q] ? 1 : 0));
      nodes.push_back(make_int2(0xffff | (q << 16), (int)pred.size() - pred0));
      for (int c = 0; c < K; ++c) {
        const auto& from = in[(size_t)q * K + c];
        if (from.empty()) continue;
        nodes.push_back(make_int2(c | (q << 16), (int)pred.size() - pred0));
        pred.insert(pred.end(), from.begin(), from.end());
        ++n_label;
      }
    }
    if (n_label > KOCR_PATTERN_MAX_NODES)
      KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_patterns: " + sp + " has " + std::to_string(n_label) +
                                      " label nodes, more than KOCR_PATTERN_MAX_NODES = " + std::to_string(KOCR_PATTERN_MAX_NODES));
    const int NT = (int)nodes.size() - node0;
    states.push_back(make_int2(NT, 0));
    nodes.push_back(make_int2(0xffff, (int)pred.size() - pred0));
    hdr[(size_t)p * 8 + 0] = Sv[p] = S;
    hdr[(size_t)p * 8 + 1] = NTv[p] = NT;
    row0 += S;
  }
  if (pred.empty()) pred.push_back(0);
  patterns_unload(ctx);
  auto& pats = ctx->patterns;
  auto put = [&](void** dptr, const void* h, size_t bytes) -> int {
    KOCR_TRY(ctx->dev_alloc(dptr, bytes));
    KOCR_HIP(ctx, hipMemcpyAsync(*dptr, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    return KOCR_OK;
  };
  int rc = put((void**)&pats.d_hdr, hdr.data(), hdr.size() * sizeof(int32_t));
  if (rc == KOCR_OK) rc = put((void**)&pats.d_nodes, nodes.data(), nodes.size() * sizeof(int2));
  if (rc == KOCR_OK) rc = put((void**)&pats.d_states, states.data(), states.size() * sizeof(int2));
  if (rc == KOCR_OK) rc = put((void**)&pats.d_pred, pred.data(), pred.size() * sizeof(int32_t));
  hipStreamSynchronize(ctx->stream);  // the host vectors go out of scope
  if (rc != KOCR_OK) {
    patterns_unload(ctx);
    return rc;
  }
  pats.P = P;
  pats.classes = C;
  pats.S = Sv;
  pats.NT = NTv;
  return KOCR_OK;
}

int kocr_pattern_count(const kocr_ctx* ctx) { return ctx ? ctx->patterns.P : KOCR_EINVAL; }

int kocr_set_pattern(kocr_ctx* ctx, int index) {
  if (!ctx) return KOCR_EINVAL;
  if (index < -1 || index >= ctx->patterns.P)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_pattern: index " + std::to_string(index) + " outside [-1, " + std::to_string(ctx->patterns.P) +
                                    ") (" + std::to_string(ctx->patterns.P) + " patterns are loaded: kocr_set_patterns)");
  ctx->pattern = index;
  return KOCR_OK;
}

int kocr_get_pattern(const kocr_ctx* ctx, int* index) {
  if (!ctx || !index) return KOCR_EINVAL;
  *index = ctx->pattern;
  return KOCR_OK;
}

// What the two entry points below share: pattern_of (HOST, nullable: the context's switch, which must then be on) checked
static int pattern_args(kocr_ctx* ctx, const char* fn, const void* in, int M, const int32_t* pattern_of, const void* labels,
                        const void* log_path, const void* log_prob) {
  const std::string f(fn);
  if (M < 0 || (M > 0 && (!in || !labels || !log_path || !log_prob))) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null buffer");
  if (crnn_classes(ctx) == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, f + ": call kocr_load_crnn first");
  if (ctx->patterns.P == 0) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": no patterns are loaded (kocr_set_patterns first)");
  if (pattern_of) KOCR_TRY(patterns_validate(ctx, fn, pattern_of, M, "crop"));
  else if (ctx->pattern < 0) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": pattern_of is null and no pattern is switched on (kocr_set_pattern)");
  if (ctx->charset >= 0)
    KOCR_FAIL(ctx, KOCR_EINVAL, f + ": a pattern cannot be combined with an active character set (kocr_set_charset): the pattern states "
                                    "the characters itself");
  return KOCR_OK;
}

// The pattern decode of include/kocr.h ("Patterns") alone: the forward up to fc_12, then the pattern launches
int kocr_crnn_pattern(kocr_ctx* ctx, const float* crops, int M, const int32_t* pattern_of, int32_t* labels, float* log_path,
                      float* log_prob, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_TRY(pattern_args(ctx, "kocr_crnn_pattern", crops, M, pattern_of, labels, log_path, log_prob));
  CrnnDecode rq;
  rq.pt = {true, pattern_of, nullptr, ctx->pattern, 0, labels, log_path, log_prob};
  CrnnExtras x;
  x.slots = 3;
  x.lists = 1;
  x.workspace = pattern_workspace_bytes(ctx, M, rq.pt);
  return crnn_call(ctx, "kocr_crnn_pattern", {crops, false}, M, rq, on_device != 0, x);
}

// KOCR_EINVAL unless the logits of a development entry fit one recogniser batch
static int one_batch(kocr_ctx* ctx, const char* fn, int M) {
  if (M > CRNN_BATCH)
    KOCR_FAIL(ctx, KOCR_EINVAL, std::string(fn) + ": M " + std::to_string(M) + " exceeds one recogniser batch of " + std::to_string(CRNN_BATCH));
  return KOCR_OK;
}

// Development entry (include/kocr.h): the pattern launches on the caller's logits (HOST)
int kocr_crnn_decode_logits_patterns(kocr_ctx* ctx, const float* logits, int M, const int32_t* pattern_of, int32_t* labels,
                                     float* log_path, float* log_prob) {
  if (!ctx) return KOCR_EINVAL;
  const char* fn = "kocr_crnn_decode_logits_patterns";
  KOCR_TRY(pattern_args(ctx, fn, logits, M, pattern_of, labels, log_path, log_prob));
  KOCR_TRY(one_batch(ctx, fn, M));
  CrnnDecode rq;
  rq.pt = {true, pattern_of, nullptr, ctx->pattern, 0, labels, log_path, log_prob};
  CrnnExtras x;
  x.slots = 3;
  x.lists = 1;
  x.workspace = pattern_workspace_bytes(ctx, M, rq.pt);
  return crnn_call(ctx, fn, {logits, true}, M, rq, false, x);
}

// What kocr_crnn_decode_logits and kocr_crnn_decode_logits_charsets (`fn`: the one that was called) share: crnn_forward's
// launches behind fc_12 on the caller's logits, as `rq` on the caller's buffers states them, then the loss where tg.labels is
// given; set_of (HOST, nullable): the crops' character sets in place of the context's switch
static int decode_logits_call(kocr_ctx* ctx, const char* fn, const float* logits, int M, const CrnnDecode& rq, CtcTargets tg,
                              const int32_t* set_of) {
  const std::string f(fn);
  if (M < 0 || (M > 0 && (!logits || !rq.d_labels))) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null buffer");
  if (!rq.sc.d_logw != !rq.sc.d_chars) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": log_word and char_scores go together");
  const int C = crnn_classes(ctx);
  if (C == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, f + ": call kocr_load_crnn first");
  KOCR_TRY(one_batch(ctx, fn, M));
  if (rq.bm.beam_width) {
    KOCR_TRY(beam_validate(ctx, fn, rq.bm.beam_width, rq.bm.top_paths));
    if (M > 0 && (!rq.bm.d_labels || !rq.bm.d_logp)) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null beam buffer");
  }
  if (rq.lx.top_words) {
    KOCR_TRY(lexicon_validate(ctx, fn, rq.lx.top_words));
    if (M > 0 && (!rq.lx.d_index || !rq.lx.d_logp)) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null lexicon buffer");
  }
  if (tg.labels) {
    if (tg.stride < 0) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": bad sizes");
    if (M > 0 && (!tg.lengths || !tg.input_lengths || !tg.loss)) KOCR_FAIL(ctx, KOCR_EINVAL, f + ": null loss buffer");
    KOCR_TRY(ctc_validate(ctx, fn, M, crnn_label_width(ctx), C, tg.labels, tg.stride, tg.lengths, tg.input_lengths, &tg.Lmax));
  }
  if (set_of) KOCR_TRY(charsets_validate(ctx, fn, set_of, M, "crop"));
  CrnnExtras x;
  x.slots = 10;
  x.lists = 2;
  x.workspace = rq.lx.top_words ? lexicon_workspace_bytes(ctx, M, !rq.lx.d_all) : 0;
  x.set_of = set_of;
  x.loss = tg.labels ? &tg : nullptr;
  return crnn_call(ctx, fn, {logits, true}, M, rq, false, x);
}

int kocr_crnn_decode_logits(kocr_ctx* ctx, const float* logits, int M, int32_t* labels, float* probs, float* log_word,
                            float* char_scores, int beam_width, int top_paths, int32_t* beam_labels, float* beam_log_prob,
                            int top_words, int32_t* lex_index, float* lex_log_prob, float* lex_values, const int32_t* loss_labels,
                            int label_stride, const int32_t* label_lengths, const int32_t* input_lengths, float* loss) {
  if (!ctx) return KOCR_EINVAL;
  CrnnDecode rq;
  rq.greedy = true;
  rq.d_labels = labels;
  rq.d_probs = probs;
  rq.sc = {log_word != nullptr, log_word, char_scores};
  rq.bm = {beam_width, top_paths, beam_labels, beam_log_prob};
  rq.lx = {top_words, lex_index, lex_log_prob, lex_values};
  const CtcTargets tg{loss_labels, label_stride, label_lengths, input_lengths, loss};
  return decode_logits_call(ctx, "kocr_crnn_decode_logits", logits, M, rq, tg, nullptr);
}

int kocr_crnn_decode_logits_charsets(kocr_ctx* ctx, const float* logits, int M, int32_t* labels, float* probs, float* log_word,
                                     float* char_scores, int beam_width, int top_paths, int32_t* beam_labels, float* beam_log_prob,
                                     int top_words, int32_t* lex_index, float* lex_log_prob, float* lex_values,
                                     const int32_t* loss_labels, int label_stride, const int32_t* label_lengths,
                                     const int32_t* input_lengths, float* loss, const int32_t* set_of) {
  if (!ctx) return KOCR_EINVAL;
  CrnnDecode rq;
  rq.greedy = true;
  rq.d_labels = labels;
  rq.d_probs = probs;
  rq.sc = {log_word != nullptr, log_word, char_scores};
  rq.bm = {beam_width, top_paths, beam_labels, beam_log_prob};
  rq.lx = {top_words, lex_index, lex_log_prob, lex_values};
  const CtcTargets tg{loss_labels, label_stride, label_lengths, input_lengths, loss};
  return decode_logits_call(ctx, "kocr_crnn_decode_logits_charsets", logits, M, rq, tg, set_of);
}

int kocr_crnn_features(kocr_ctx* ctx, const float* crops, int M, float* feats, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (M < 0 || (M > 0 && (!crops || !feats))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_crnn_features: null buffer");
  const int C = crnn_classes(ctx);
  if (C == 0) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_crnn_features: call kocr_load_crnn first");
  if (M == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int mb = crnn_batch(M);
  const size_t fpc = (size_t)CRNN_STEPS * CRNN_FEAT;  // features per crop
  const size_t cb = CRNN_CROP_PIXELS * sizeof(float), fb = fpc * sizeof(float);
  Staging st{ctx, ctx->ws, "kocr_crnn_features", on_device != 0};
  KOCR_TRY(st.reserve(crnn_workspace_bytes(mb, C), {cb * mb, fb * mb}));
  return crnn_batches(ctx, M, [&](long s, int nb) -> int {
    const float* d_c;
    float* d_f;
    KOCR_TRY(st.in(crops + s * CRNN_CROP_PIXELS, cb * nb, d_c));
    KOCR_TRY(st.out(feats + s * fpc, fb * nb, d_f));
    KOCR_TRY(crnn_features(ctx, d_c, nb, d_f));
    KOCR_TRY(st.back(feats + s * fpc, d_f, fb * nb));
    return st.finish();
  });
}

int kocr_compute_maps(kocr_ctx* ctx, const uint8_t* heatmap, int hh, int hw, int N, int H, int W, int n_chars,
                      const float* char_quads, const uint8_t* is_space, int n_lines, const int32_t* line_offsets,
                      const int32_t* image_line_offsets, float* maps, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  const char* fn = "kocr_compute_maps";
  if (H % 2 != 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_compute_maps: Height must be an even number");
  if (W % 2 != 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_compute_maps: Width must be an even number");
  if (N < 0 || H < 0 || W < 0 || hh < 1 || hw < 1 || n_chars < 0 || n_lines < 0)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_compute_maps: bad sizes");
  if (N > 0 && (!heatmap || !line_offsets || !image_line_offsets || !maps || (n_chars > 0 && (!char_quads || !is_space))))
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_compute_maps: null buffer");
  if (!on_device && N > 0) {
    bool ok = line_offsets[0] == 0 && line_offsets[n_lines] == n_chars && image_line_offsets[0] == 0 &&
              image_line_offsets[N] == n_lines;
    for (int l = 0; ok && l < n_lines; ++l) ok = line_offsets[l] < line_offsets[l + 1];
    for (int i = 0; ok && i < N; ++i) ok = image_line_offsets[i] <= image_line_offsets[i + 1];
    if (!ok) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_compute_maps: offsets must run from 0 to n_chars / n_lines, lines non-empty");
  }
  const int h = H / 2, w = W / 2;
  if (N == 0 || (long)h * w == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t n = (size_t)n_chars, px = (size_t)N * h * w;
  const size_t heat_b = (size_t)hh * hw, quad_b = n * 8 * sizeof(float), line_b = ((size_t)n_lines + 1) * sizeof(int32_t);
  const size_t img_b = ((size_t)N + 1) * sizeof(int32_t), maps_b = px * 2 * sizeof(float);
  const size_t slot_b = 2 * n * sizeof(MapSlot), plane_b = px * 2 * sizeof(int32_t);
  Staging st{ctx, ctx->io, fn, on_device != 0};
  KOCR_TRY(st.reserve(0, {heat_b, quad_b, n, line_b, img_b, maps_b},
                      {quad_b, n * 2 * sizeof(float), n * sizeof(int), n * sizeof(int), slot_b, plane_b}));
  const uint8_t *d_heat, *d_space;
  const float* d_quads;
  const int32_t *d_loff, *d_ioff;
  float* d_maps;
  KOCR_TRY(st.in(heatmap, heat_b, d_heat));
  KOCR_TRY(st.in(char_quads, quad_b, d_quads));
  KOCR_TRY(st.in(is_space, n, d_space));
  KOCR_TRY(st.in(line_offsets, line_b, d_loff));
  KOCR_TRY(st.in(image_line_offsets, img_b, d_ioff));
  KOCR_TRY(st.out(maps, maps_b, d_maps));
  MapsWork wk;
  KOCR_TRY(st.scratch(quad_b, wk.rbox));
  KOCR_TRY(st.scratch(n * 2 * sizeof(float), wk.ctr));
  KOCR_TRY(st.scratch(n * sizeof(int), wk.permx));
  KOCR_TRY(st.scratch(n * sizeof(int), wk.permy));
  KOCR_TRY(st.scratch(slot_b, wk.slots));
  KOCR_TRY(st.scratch(plane_b, wk.planes));
  // numpy's float32 v / 255 (detection.py:197): IEEE division on the host, so the device's division rule never matters.  The
  // table stays resident on the context (a blocking upload by the first call), so a device-pointer call copies nothing from
  // host memory and stays asynchronous
  if (!ctx->d_div255) {
    std::vector<float> table(256);
    for (int v = 0; v < 256; ++v) table[v] = (float)v / 255.0f;
    KOCR_TRY(ctx->upload(&ctx->d_div255, table));
  }
  wk.table = ctx->d_div255;
  KOCR_TRY(launch_compute_maps(ctx, d_heat, hh, hw, N, h, w, n_chars, d_quads, d_space, n_lines, d_loff, d_ioff, wk, d_maps));
  KOCR_TRY(st.back(maps, d_maps, maps_b));
  return st.finish();
}

int kocr_heat_mse(kocr_ctx* ctx, const float* y_true, const float* y_pred, int N, int h, int w, double* sums, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || h < 0 || w < 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_heat_mse: bad sizes");
  if (N > 0 && (!y_true || !y_pred || !sums)) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_heat_mse: null buffer");
  if (N == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t yb = (size_t)N * h * w * 2 * sizeof(float), sb = (size_t)N * sizeof(double);
  Staging st{ctx, ctx->io, "kocr_heat_mse", on_device != 0};
  KOCR_TRY(st.reserve(0, {yb, yb, sb}));
  const float *d_t, *d_p;
  double* d_s;
  KOCR_TRY(st.in(y_true, yb, d_t));
  KOCR_TRY(st.in(y_pred, yb, d_p));
  KOCR_TRY(st.out(sums, sb, d_s));
  KOCR_TRY(launch_heat_mse(ctx, d_t, d_p, N, h * w, d_s));
  KOCR_TRY(st.back(sums, d_s, sb));
  return st.finish();
}

int kocr_craft_mse(kocr_ctx* ctx, const void* img, int dtype, int N, int H, int W, const float* y_true, int micro_batch,
                   double* sums, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || (N > 0 && (!img || !y_true || !sums))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_craft_mse: null buffer");
  if (dtype != KOCR_U8 && dtype != KOCR_F32) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_craft_mse: bad dtype");
  if (N == 0) return KOCR_OK;
  if (!craft_loaded(ctx)) KOCR_FAIL(ctx, KOCR_ENOWEIGHTS, "kocr_craft_mse: call kocr_load_craft first");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const int mb = craft_micro_batch(micro_batch, N, H, W);
  const size_t in_img = (size_t)H * W * 3 * (dtype == KOCR_U8 ? 1 : 4);
  const size_t out_img = (size_t)(H / 2) * (W / 2) * 2 * sizeof(float);
  Staging st{ctx, ctx->ws, "kocr_craft_mse", on_device != 0};
  KOCR_TRY(st.reserve(craft_workspace_bytes(mb, H, W), {in_img * mb, out_img * mb, sizeof(double) * mb}, {out_img * mb}));
  return craft_batches(ctx, micro_batch, N, H, W, [&](int s, int nb) -> int {
    const void* d_in;
    const float* d_y;
    float* d_heat;
    double* d_s;
    KOCR_TRY(st.in((const void*)((const char*)img + (size_t)s * in_img), in_img * nb, d_in));
    KOCR_TRY(st.in((const float*)((const char*)y_true + (size_t)s * out_img), out_img * nb, d_y));
    KOCR_TRY(st.out(sums + s, sizeof(double) * nb, d_s));
    KOCR_TRY(st.scratch(out_img * nb, d_heat));
    KOCR_TRY(craft_forward(ctx, d_in, dtype, nb, H, W, d_heat));
    KOCR_TRY(launch_heat_mse(ctx, d_y, d_heat, nb, (H / 2) * (W / 2), d_s));
    KOCR_TRY(st.back(sums + s, d_s, sizeof(double) * nb));
    return st.finish();
  });
}

int kocr_get_boxes(kocr_ctx* ctx, const float* heat, int N, int h, int w, float detection_threshold,
                   float text_threshold, float link_threshold, int size_threshold, float* boxes,
                   int32_t* counts, int cap, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || (N > 0 && (!heat || !boxes || !counts))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_get_boxes: null buffer");
  if (N == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t hb = (size_t)N * h * w * 2 * sizeof(float), bb = (size_t)N * cap * 8 * sizeof(float);
  Staging st{ctx, ctx->io, "kocr_get_boxes", on_device != 0};
  KOCR_TRY(st.reserve(0, {hb, bb}));
  const float* d_heat;
  float* d_boxes;
  KOCR_TRY(st.in(heat, hb, d_heat));
  KOCR_TRY(st.out(boxes, bb, d_boxes));
  int n_empty = 0;
  const float* d_scores = nullptr;
  const int rc = postproc_get_boxes(ctx, d_heat, N, h, w, detection_threshold, text_threshold, link_threshold,
                                    size_threshold, d_boxes, cap, counts, &n_empty, nullptr, &d_scores);
  if (rc != KOCR_OK) return rc;
  KOCR_TRY(chars_resident(ctx, "kocr_get_boxes", d_heat, N, h, w, d_boxes, cap, counts));
  KOCR_TRY(st.back(boxes, d_boxes, bb));
  KOCR_TRY(st.finish());
  ctx->keep_det_scores(d_scores, N, cap);
  if (n_empty > 0)
    KOCR_FAIL(ctx, KOCR_EEMPTYCONTOUR,
              "kocr_get_boxes: a component has no pixels left after removing text&link overlap "
              "(the reference raises IndexError at detection.py:272)");
  return KOCR_OK;
}

int kocr_warp_crops(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, const float* boxes,
                    const int32_t* counts, int target_h, int target_w, float* crops, int on_device) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || target_h <= 0 || target_w <= 0 || (N > 0 && (!img_rgb || !counts)))
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_warp_crops: bad argument");
  std::vector<WarpParam> prm;
  const long M = prepare_box_warps(ctx, "kocr_warp_crops", N, boxes, counts, crops, target_h, target_w, prm);
  if (M <= 0) return (int)M;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ib = (size_t)N * H * W * 3, cb = (size_t)M * target_h * target_w * sizeof(float);
  const size_t pb = (size_t)M * sizeof(WarpParam);
  Staging st{ctx, ctx->io, "kocr_warp_crops", on_device != 0};
  KOCR_TRY(st.reserve(0, {ib, cb}, {pb}));
  const WarpParam* d_prm;
  const uint8_t* d_img;
  float* d_crops;
  KOCR_TRY(st.upload(prm.data(), pb, d_prm));
  KOCR_TRY(st.in(img_rgb, ib, d_img));
  KOCR_TRY(st.out(crops, cb, d_crops));
  KOCR_TRY(launch_warp(ctx, d_img, H, W, d_prm, (int)M, target_h, target_w, d_crops));
  KOCR_TRY(st.back(crops, d_crops, cb));
  // prm is host memory about to go out of scope: the H2D copy must have completed
  KOCR_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return KOCR_OK;
}

// float images (round 5): the same two image operations in float, see imgproc.hip / warp.hip.  Host pointers.
int kocr_resize_pad_f32(kocr_ctx* ctx, const float* src, int n, int sh, int sw, int channels, int dh, int dw, int Hmax, int Wmax,
                        float cval, float* dst) {
  if (!ctx) return KOCR_EINVAL;
  if (n < 0 || channels <= 0 || (n > 0 && (!src || !dst))) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_resize_pad_f32: bad argument");
  if (n == 0) return KOCR_OK;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t sb = (size_t)n * sh * sw * channels * sizeof(float), db = (size_t)n * Hmax * Wmax * channels * sizeof(float);
  const size_t tb = (size_t)(3 * (Wmax + Hmax) + 64) * sizeof(int);
  Staging st{ctx, ctx->io, "kocr_resize_pad_f32"};
  KOCR_TRY(st.reserve(tb, {sb, db}));
  const float* ds;
  float* dd;
  KOCR_TRY(st.in(src, sb, ds));
  KOCR_TRY(st.out(dst, db, dd));
  KOCR_TRY(launch_resize_pad_f32(ctx, ds, n, sh, sw, channels, dd, dh, dw, Hmax, Wmax, cval, ctx->io));
  KOCR_TRY(st.back(dst, dd, db));
  return st.finish();
}

int kocr_warp_crops_f32(kocr_ctx* ctx, const float* img, int N, int H, int W, int channels, const float* boxes, const int32_t* counts,
                        int target_h, int target_w, float* crops) {
  if (!ctx) return KOCR_EINVAL;
  if (N < 0 || target_h <= 0 || target_w <= 0 || (channels != 1 && channels != 3) || (N > 0 && (!img || !counts)))
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_warp_crops_f32: bad argument");
  std::vector<WarpParam> prm;
  const long M = prepare_box_warps(ctx, "kocr_warp_crops_f32", N, boxes, counts, crops, target_h, target_w, prm);
  if (M <= 0) return (int)M;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ib = (size_t)N * H * W * channels * sizeof(float), cb = (size_t)M * target_h * target_w * sizeof(float);
  const size_t pb = (size_t)M * sizeof(WarpParam);
  Staging st{ctx, ctx->io, "kocr_warp_crops_f32"};
  KOCR_TRY(st.reserve(0, {ib, cb}, {pb}));
  const WarpParam* d_prm;
  const float* di;
  float* d_crops;
  KOCR_TRY(st.upload(prm.data(), pb, d_prm));
  KOCR_TRY(st.in(img, ib, di));
  KOCR_TRY(st.out(crops, cb, d_crops));
  KOCR_TRY(launch_warp_f32(ctx, di, H, W, channels, d_prm, (int)M, target_h, target_w, d_crops));
  KOCR_TRY(st.back(crops, d_crops, cb));
  return st.finish();
}

int kocr_warp_quads(kocr_ctx* ctx, const uint8_t* img_rgb, int N, int H, int W, int M, const float* src_quads,
                    const float* dst_quads, const int32_t* image_index, const int32_t* crop_w, const int32_t* crop_h,
                    int target_h, int target_w, float* crops, double* transforms) {
  if (!ctx) return KOCR_EINVAL;
  if (N <= 0 || M < 0 || target_h <= 0 || target_w <= 0 || !img_rgb)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_warp_quads: bad argument");
  if (M == 0) return KOCR_OK;
  if (!src_quads || !dst_quads || !image_index || !crop_w || !crop_h || !crops)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_warp_quads: null buffer");
  for (int m = 0; m < M; ++m)
    if (image_index[m] < 0 || image_index[m] >= N || crop_w[m] < 0 || crop_h[m] < 0 || crop_w[m] > target_w ||
        crop_h[m] > target_h)
      KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_warp_quads: image index or crop size out of range");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  const size_t ib = (size_t)N * H * W * 3, cb = (size_t)M * target_h * target_w * sizeof(float);
  const size_t qb = (size_t)M * 8 * sizeof(float), nb = (size_t)M * sizeof(int), tb = (size_t)M * 9 * sizeof(double);
  const size_t pb = (size_t)M * sizeof(WarpParam);
  Staging st{ctx, ctx->io, "kocr_warp_quads"};
  KOCR_TRY(st.reserve(0, {ib, cb, qb, qb, nb, nb, nb, tb, pb, 256}));
  const uint8_t* d_img;
  const float *d_src, *d_dst;
  const int32_t *d_idx, *d_cw, *d_ch;
  float* d_crops;
  double* d_tf;
  WarpParam* d_prm;
  int* d_status;
  KOCR_TRY(st.in(img_rgb, ib, d_img));
  KOCR_TRY(st.out(crops, cb, d_crops));
  KOCR_TRY(st.in(src_quads, qb, d_src));
  KOCR_TRY(st.in(dst_quads, qb, d_dst));
  KOCR_TRY(st.in(image_index, nb, d_idx));
  KOCR_TRY(st.in(crop_w, nb, d_cw));
  KOCR_TRY(st.in(crop_h, nb, d_ch));
  KOCR_TRY(st.scratch(tb, d_tf));
  KOCR_TRY(st.scratch(pb, d_prm));
  KOCR_TRY(st.scratch(256, d_status));
  KOCR_HIP(ctx, hipMemsetAsync(d_status, 0, sizeof(int), ctx->stream));
  KOCR_TRY(launch_warp_quads(ctx, d_src, d_dst, d_idx, d_cw, d_ch, M, d_prm, d_tf, d_status));
  KOCR_TRY(launch_warp(ctx, d_img, H, W, d_prm, M, target_h, target_w, d_crops));
  int status = 0;
  KOCR_TRY(st.back(crops, d_crops, cb));
  if (transforms) KOCR_TRY(st.back(transforms, d_tf, tb));
  KOCR_TRY(st.download(&status, d_status, sizeof(int)));
  KOCR_TRY(st.finish());
  if (status != 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_warp_quads: singular perspective transform");
  return KOCR_OK;
}

int kocr_conv2d_nhwc(kocr_ctx* ctx, const float* in, int N, int H, int W, int Cin, const float* w_hwio,
                     int KH, int KW, int dilation, int Cout, const float* pre_a, const float* pre_b,
                     int relu, const float* post_a, const float* post_b, float* out) {
  if (!ctx || !in || !w_hwio || !out) return KOCR_EINVAL;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || KH <= 0 || KW <= 0 || dilation <= 0 ||
      !(KH & 1) || !(KW & 1))
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_conv2d_nhwc: bad shape (odd kernels, positive sizes)");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  KOCR_TRY(ctx->amax_begin());  // allocates the slot pool BEFORE the layer's mark: it outlives this call
  TempLayer layer(ctx);
  ConvLayer L;
  L.name = "kocr_conv2d_nhwc";
  KOCR_TRY(prepare_conv(ctx, L, w_hwio, /*oihw=*/false, Cin, Cout, KH, KW, dilation, pre_a, pre_b, relu, post_a, post_b));
  const size_t nin = (size_t)N * H * W * Cin * sizeof(float), nout = (size_t)N * H * W * Cout * sizeof(float);
  Staging st{ctx, ctx->ws, "kocr_conv2d_nhwc"};
  KOCR_TRY(st.reserve(0, {nin, nout}));
  Tensor ti, to;
  ti.N = to.N = N;
  ti.H = to.H = H;
  ti.W = to.W = W;
  ti.C = ti.cs = Cin;
  to.C = to.cs = Cout;
  const float* d_in;
  KOCR_TRY(st.in(in, nin, d_in));
  KOCR_TRY(st.out(out, nout, to.p));
  ti.p = (float*)d_in;
  KOCR_TRY(launch_conv(ctx, L, ti, nullptr, nullptr, to));
  KOCR_TRY(st.back(out, to.p, nout));
  return st.finish();
}

int kocr_conv2d_cells(kocr_ctx* ctx, const float* in, int N, int H, int W, int Cin, const float* w_hwio, int Cout,
                      const float* pre_a, const float* pre_b, int relu, const float* post_a, const float* post_b,
                      int cellW, int cellWv, int pool, float* out, float* pool_out, float* amax_out) {
  if (!ctx || !in || !w_hwio || (!out && !pool) || (pool && !pool_out)) return KOCR_EINVAL;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || cellW <= 0 || cellWv <= 0 || W % cellW)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_conv2d_cells: bad shape");
  // the constraints include/kocr.h documents, checked here with their own messages: the columns behind cellWv are
  // the 'same' padding between neighbouring crops -- without at least one of them a crop would read its neighbour's edge
  if (cellWv >= cellW)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_conv2d_cells: cellWv must be smaller than cellW (at least one zero gutter column per cell)");
  if (cellW % 4 != 0) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_conv2d_cells: cellW must be a multiple of 4 (F(4,3) quads)");
  if (pool && (cellWv % 2 != 0 || cellW % 8 != 0 || H % 2 != 0))
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_conv2d_cells: pooling needs an even cellWv, cellW % 8 == 0 and an even H");
  if (Cin % 32 != 0 || Cout <= 64)
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_conv2d_cells: the cell-grid kernel takes Cin % 32 == 0 and Cout > 64");
  if (!((H % 4 == 0 && W % 64 == 0) || (H % 8 == 0 && W % 32 == 0)))
    KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_conv2d_cells: the grid must tile as 4 x 64 (H % 4 == 0, W % 64 == 0) or 8 x 32");
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  KOCR_TRY(ctx->amax_begin());
  TempLayer layer(ctx);
  ConvLayer L;
  L.name = "kocr_conv2d_cells";
  KOCR_TRY(prepare_conv(ctx, L, w_hwio, /*oihw=*/false, Cin, Cout, 3, 3, 1, pre_a, pre_b, relu, post_a, post_b));
  const int cn = W / cellW;
  const size_t nin = (size_t)N * H * W * Cin * sizeof(float), nout = (size_t)N * H * W * Cout * sizeof(float), npool = nout / 4;
  Staging st{ctx, ctx->ws, "kocr_conv2d_cells"};
  KOCR_TRY(st.reserve(0, {nin, out ? nout : 0, pool ? npool : 0}));
  Tensor ti, to, tp;
  ti.N = to.N = tp.N = N;
  ti.H = to.H = H;
  ti.W = to.W = W;
  tp.H = H / 2;
  tp.W = W / 2;
  ti.C = ti.cs = Cin;
  to.C = to.cs = tp.C = tp.cs = Cout;
  ti.cellW = to.cellW = cellW;
  ti.cellWv = to.cellWv = cellWv;
  tp.cellW = cellW / 2;
  tp.cellWv = cellWv / 2;
  ti.amax = ctx->amax_slots(N * cn);
  to.amax = ctx->amax_slots(N * cn);
  tp.amax = ctx->amax_slots(N * cn);
  if (!ti.amax || !to.amax || !tp.amax) KOCR_FAIL(ctx, KOCR_ECAPACITY, "kocr_conv2d_cells: out of max-|x| slots");
  const float* d_in;
  KOCR_TRY(st.in(in, nin, d_in));
  ti.p = (float*)d_in;
  if (out) KOCR_TRY(st.out(out, nout, to.p));
  if (pool) KOCR_TRY(st.out(pool_out, npool, tp.p));
  // the input's per-cell max |x| (its producer's job in the recogniser): computed here on the host
  std::vector<float> am((size_t)N * cn, 0.f);
  for (int n = 0; n < N; ++n)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const float* px = in + (((size_t)n * H + y) * W + x) * Cin;
        float m = 0.f;
        for (int c = 0; c < Cin; ++c) m = std::max(m, std::fabs(px[c]));
        float& a = am[(size_t)n * cn + x / cellW];
        a = std::max(a, m);
      }
  KOCR_TRY(st.put((float*)ti.amax, am.data(), am.size() * sizeof(float)));
  KOCR_TRY(launch_conv_pool(ctx, L, ti, nullptr, nullptr, to, pool ? &tp : nullptr, /*need_full=*/out != nullptr));
  if (out) KOCR_TRY(st.back(out, to.p, nout));
  if (pool) KOCR_TRY(st.back(pool_out, tp.p, npool));
  if (amax_out) KOCR_TRY(st.download(amax_out, (const float*)(pool && !out ? tp.amax : to.amax), am.size() * sizeof(float)));
  return st.finish();
}

int kocr_set_split_mode(kocr_ctx* ctx, int mode) {
  if (!ctx) return KOCR_EINVAL;
  if (mode != KOCR_SPLIT_BF16X3 && mode != KOCR_SPLIT_F16X2 && mode != KOCR_SPLIT_F16X1) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_split_mode: unknown mode");
  ctx->split_mode = mode;
  return KOCR_OK;
}

int kocr_get_split_mode(const kocr_ctx* ctx) { return ctx ? ctx->split_mode : KOCR_EINVAL; }

int kocr_set_schedule(kocr_ctx* ctx, int fold_linear_chain, int fold_upsample) {
  if (!ctx) return KOCR_EINVAL;
  ctx->opt_linfold = fold_linear_chain != 0;
  ctx->opt_upfold = fold_upsample != 0;
  return KOCR_OK;
}

int kocr_get_schedule(kocr_ctx* ctx, int* fold_linear_chain, int* fold_upsample) {
  if (!ctx || !fold_linear_chain || !fold_upsample) return KOCR_EINVAL;
  *fold_linear_chain = ctx->opt_linfold ? 1 : 0;
  *fold_upsample = ctx->opt_upfold ? 1 : 0;
  return KOCR_OK;
}

int kocr_set_min_area_rect(kocr_ctx* ctx, int rule) {
  if (!ctx) return KOCR_EINVAL;
  if (rule != KOCR_RECT_EXACT && rule != KOCR_RECT_OPENCV) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_min_area_rect: unknown rule");
  ctx->min_area_rect = rule;
  return KOCR_OK;
}

int kocr_get_min_area_rect(const kocr_ctx* ctx) { return ctx ? ctx->min_area_rect : KOCR_EINVAL; }

int kocr_set_scores(kocr_ctx* ctx, int on) {
  if (!ctx) return KOCR_EINVAL;
  if (on != 0 && on != 1) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_set_scores: on must be 0 or 1");
  ctx->scores_on = on != 0;
  return KOCR_OK;
}

int kocr_get_scores(const kocr_ctx* ctx) { return ctx ? (ctx->scores_on ? 1 : 0) : KOCR_EINVAL; }

int kocr_set_beam(kocr_ctx* ctx, int beam_width, int top_paths) {
  if (!ctx) return KOCR_EINVAL;
  if (beam_width == 0) {
    ctx->beam_width = 0;
    ctx->beam_top_paths = 1;
    return KOCR_OK;
  }
  KOCR_TRY(beam_validate(ctx, "kocr_set_beam", beam_width, top_paths));
  ctx->beam_width = beam_width;
  ctx->beam_top_paths = top_paths;
  return KOCR_OK;
}

int kocr_get_beam(const kocr_ctx* ctx, int* beam_width, int* top_paths) {
  if (!ctx) return KOCR_EINVAL;
  if (beam_width) *beam_width = ctx->beam_width;
  if (top_paths) *top_paths = ctx->beam_top_paths;
  return KOCR_OK;
}

int kocr_set_lexicon_match(kocr_ctx* ctx, int top_words) {
  if (!ctx) return KOCR_EINVAL;
  if (top_words != 0) KOCR_TRY(lexicon_validate(ctx, "kocr_set_lexicon_match", top_words));
  ctx->lex_top = top_words;
  return KOCR_OK;
}

int kocr_get_lexicon_match(const kocr_ctx* ctx, int* top_words) {
  if (!ctx) return KOCR_EINVAL;
  if (top_words) *top_words = ctx->lex_top;
  return KOCR_OK;
}

int kocr_profile_enable(kocr_ctx* ctx, int on) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_TRY(ctx->prof_flush());
  ctx->prof_on = on != 0;
  return KOCR_OK;
}

int kocr_profile_reset(kocr_ctx* ctx) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_TRY(ctx->prof_flush());
  ctx->prof.clear();
  return KOCR_OK;
}

int kocr_profile_report(kocr_ctx* ctx, int cap, char* names, int64_t* launches, double* total_ms,
                        double* flops, double* bytes) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_TRY(ctx->prof_flush());
  int i = 0;
  for (auto& kv : ctx->prof) {
    if (i < cap && names && launches && total_ms && flops && bytes) {
      snprintf(names + (size_t)i * 64, 64, "%s", kv.first.c_str());
      launches[i] = kv.second.launches;
      total_ms[i] = kv.second.ms;
      flops[i] = kv.second.flops;
      bytes[i] = kv.second.bytes;
    }
    ++i;
  }
  return i;
}

int kocr_range_stats_enable(kocr_ctx* ctx, int on) {
  if (!ctx) return KOCR_EINVAL;
  if (on && !ctx->d_range) {  // allocated here, not at first use: kocr_conv2d_nhwc frees what a call allocates
    KOCR_HIP(ctx, hipSetDevice(ctx->device));
    void* d = nullptr;
    KOCR_TRY(ctx->dev_alloc(&d, 64));
    ctx->d_range = d;
  }
  ctx->range_on = on != 0;
  if (on) ctx->range.clear();
  return KOCR_OK;
}

int kocr_range_stats_report(kocr_ctx* ctx, int cap, char* names, double* values) {
  if (!ctx) return KOCR_EINVAL;
  int i = 0;
  for (auto& kv : ctx->range) {
    if (i < cap && names && values) {
      snprintf(names + (size_t)i * 64, 64, "%s", kv.first.c_str());
      const RangeRow& r = kv.second;
      const double v[7] = {r.launches, r.elements, r.nonzero, r.below_m4, r.below_m14, r.sum_abs, r.sum_abs_below_m4};
      for (int k = 0; k < 7; ++k) values[(size_t)i * 7 + k] = v[k];
    }
    ++i;
  }
  return i;
}

// ---- workspace arenas: for tests (include/kocr.h) ----
int kocr_debug_arena_count(void) { return kocr_ctx::N_ARENAS; }

const char* kocr_debug_arena_name(int i) { return kocr_ctx::arena_name(i); }

int kocr_debug_arena_stats(kocr_ctx* ctx, int i, uint64_t* cap, uint64_t* requested, uint64_t* peak, uint64_t* excess) {
  if (!ctx) return KOCR_EINVAL;
  const Arena* a = ctx->arena_at(i);
  if (!a) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_debug_arena_stats: no arena " + std::to_string(i));
  if (cap) *cap = a->cap;
  if (requested) *requested = a->requested;
  if (peak) *peak = a->peak;
  if (excess) *excess = a->excess;
  return KOCR_OK;
}

int kocr_debug_release_arenas(kocr_ctx* ctx) {
  if (!ctx) return KOCR_EINVAL;
  KOCR_HIP(ctx, hipSetDevice(ctx->device));
  KOCR_TRY(release_arenas(ctx));
  ctx->guard_damage = kocr_ctx::GuardDamage{};
  return KOCR_OK;
}

int kocr_debug_memory_stats(kocr_ctx* ctx, uint64_t* persistent_count, uint64_t* persistent_bytes, uint64_t* arena_bytes,
                            uint64_t* process_count, uint64_t* process_bytes) {
  uint64_t pc = 0, pb = 0, ab = 0;
  if (ctx) {
    pc = ctx->owned.size();
    for (const kocr_ctx::Owned& o : ctx->owned) pb += o.bytes;
    for (int i = 0; i < kocr_ctx::N_ARENAS; ++i) ab += ctx->arena_at(i)->cap;
  }
  if (persistent_count) *persistent_count = pc;
  if (persistent_bytes) *persistent_bytes = pb;
  if (arena_bytes) *arena_bytes = ab;
  if (process_count) *process_count = g_mem_count.load();
  if (process_bytes) *process_bytes = g_mem_bytes.load();
  return KOCR_OK;
}

int kocr_debug_set_arena_guards(kocr_ctx* ctx, int on) {
  if (!ctx) return KOCR_EINVAL;
  for (int i = 0; i < kocr_ctx::N_ARENAS; ++i) {
    Arena& a = *ctx->arena_at(i);
    if (!a.guards.empty()) arena_guard_check(a);
    // the next allocation of an arena comes behind a reset of it; until then its offsets stay what they are
    a.gctx = on ? ctx : nullptr;
  }
  return KOCR_OK;
}

int kocr_debug_set_arena_poison(kocr_ctx* ctx, int byte) {
  if (!ctx) return KOCR_EINVAL;
  if (byte < -1 || byte > 255) KOCR_FAIL(ctx, KOCR_EINVAL, "kocr_debug_set_arena_poison: byte must be -1 (off) or in [0, 255]");
  for (int i = 0; i < kocr_ctx::N_ARENAS; ++i) {
    Arena& a = *ctx->arena_at(i);
    a.pctx = byte >= 0 ? ctx : nullptr;
    a.pbyte = (unsigned char)(byte >= 0 ? byte : 0);
  }
  return KOCR_OK;
}

int kocr_debug_check_arena_guards(kocr_ctx* ctx, int* arena, uint64_t* offset, uint64_t* byte) {
  if (!ctx) return KOCR_EINVAL;
  for (int i = 0; i < kocr_ctx::N_ARENAS; ++i) arena_guard_check(*ctx->arena_at(i));
  const kocr_ctx::GuardDamage d = ctx->guard_damage;
  ctx->guard_damage = kocr_ctx::GuardDamage{};
  if (arena) *arena = d.arena;
  if (offset) *offset = d.offset;
  if (byte) *byte = d.byte;
  return d.count;
}

}  // extern "C"
