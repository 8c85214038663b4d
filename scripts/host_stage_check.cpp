// Developer check on the host alone (no GPU, nothing of the library linked): the decode request of common.h (CrnnDecode with
// each / from), the recogniser stage of abi.h (RecStage with staging_bytes / staging_take) and the resident-result states of
// kocr_ctx, over arenas of HOST memory, with a crnn_forward that fills every row it is handed with that buffer's own byte.
// Under the address and undefined-behaviour sanitizers a row past its buffer or past the arena is reported; rows of two
// buffers that overlap fail the pattern check.
//   hipcc -std=c++17 -x hip --cuda-host-only -Xarch_host -fsanitize=address,undefined -Wno-unused-value -I keras_ocr_amd/csrc \
//         scripts/host_stage_check.cpp -o host_stage_check && ./host_stage_check
#include "abi.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "line %d: %s\n", __LINE__, #c);                 \
      exit(1);                                                        \
    }                                                                 \
  } while (0)

// ---- what the helpers call in the library, restated on host memory ----
static int LW = 48;
static const int C = 37, V = 11;
int arena_reserve(kocr_ctx* ctx, Arena& a, size_t bytes) {
  ctx->invalidate_results();
  if (bytes <= a.cap) return KOCR_OK;
  free(a.base);
  a.base = (char*)malloc(bytes);  // exactly what was asked for: one byte more is the sanitizer's
  a.cap = bytes;
  a.off = 0;
  return KOCR_OK;
}
int kocr_ctx::ws_reserve(size_t bytes) { return arena_reserve(this, ws, bytes); }
void arena_guard_fill(Arena&, size_t, size_t) {}  // guard mode stays off here (scripts/host_arena_check.cpp drives it)
void arena_guard_check(Arena&) {}
void arena_poison_fill(Arena&, void*, size_t) {}  // ... and so does poison mode
int crnn_label_width(kocr_ctx*) { return LW; }
int crnn_classes(kocr_ctx*) { return C; }
size_t crnn_workspace_bytes(int M, int) { return (size_t)M * 64; }
size_t lexicon_workspace_bytes(kocr_ctx*, int M, bool) { return (size_t)M * 16; }
size_t pattern_workspace_bytes(kocr_ctx*, int M, const CrnnPattern&) { return (size_t)M * 8; }
int craft_micro_batch(int micro_batch, int N, int, int) { return std::min(micro_batch > 0 ? micro_batch : 32, N); }

// a buffer's own byte: the place of its pointer in the request, the same for the caller's request and every batch's
template <class P> static int byte_of(const CrnnDecode& r, const P& member) {
  return 1 + (int)(((const char*)&member - (const char*)&r) / sizeof(void*));
}

static long crops_seen;
static int outputs_seen;
int crnn_forward(kocr_ctx*, const float* d_crops, int M, const CrnnDecode& rq) {
  const size_t m = (size_t)M;
  for (size_t i = 0; i < m * CRNN_CROP_PIXELS; ++i) CHECK(d_crops[i] == 0.f);
  CHECK(rq.cm.first == crops_seen && (!rq.pt.on || rq.pt.first == crops_seen));  // the batch's place in the call
  CrnnDecode r = rq;
  outputs_seen = 0;
  r.each(LW, C, V, [&](auto*& p, size_t b) {
    memset(p, byte_of(r, p), m * b);
    ++outputs_seen;
    return KOCR_OK;
  });
  crops_seen += M;
  return KOCR_OK;
}

static void filled(const void* p, int byte, size_t n) {
  for (size_t i = 0; i < n; ++i) CHECK(((const unsigned char*)p)[i] == byte);
}

// the device buffers of one batch of a request as a buffer list (abi.h)
struct Rows {
  CrnnDecode d;
  int nb;
  template <class F> int each(F f) {
    return d.each(LW, C, V, [&](auto*& p, size_t b) { return f(p, (size_t)nb * b); });
  }
};

// The request on its own, as a staged call of api.cpp drives it: every output on (the probabilities and the lexicon's values
// too), the caller's buffers exactly sized, each batch's device buffers from an arena of exactly the bytes that each() states.
static void check_request(kocr_ctx& ctx, long M) {
  CrnnDecode host;
  host.greedy = host.sc.on = host.pt.on = true;
  host.bm.beam_width = 4;
  host.bm.top_paths = 3;
  host.lx.top_words = 5;
  int* const want_i = (int*)8;  // "given": each() lists the probabilities and the values only where the caller has a buffer
  host.d_probs = host.lx.d_all = (float*)want_i;
  int n_out = 0;
  CHECK(host.each(LW, C, V, [&](auto*& p, size_t b) {
    p = (std::remove_reference_t<decltype(p)>)calloc((size_t)M, b);
    ++n_out;
    return KOCR_OK;
  }) == KOCR_OK && n_out == CrnnDecode::MAX_OUTPUTS);
  crops_seen = 0;
  for (long s = 0; s < M; s += CRNN_BATCH) {
    const int nb = crnn_batch(M - s);
    const CrnnDecode h = host.from(s, LW, C, V);
    CHECK(h.cm.first == s && h.pt.first == s && (char*)h.d_probs == (char*)host.d_probs + (size_t)s * LW * C * 4 &&
          (char*)h.lx.d_all == (char*)host.lx.d_all + (size_t)s * V * 4 && (char*)h.bm.d_logp == (char*)host.bm.d_logp + (size_t)s * 3 * 4);
    Rows rows{h, nb};
    size_t exact = 0, counted = 0;  // as arena_alloc places them; as Staging::reserve counts them
    rows.each([&](auto*&, size_t b) {
      exact = ((exact + 255) & ~(size_t)255) + b;
      counted += b + 256;
      return KOCR_OK;
    });
    CHECK(staging_bytes(rows) == counted && exact <= counted);
    free(ctx.io.base);
    ctx.io = Arena{};
    CHECK(arena_reserve(&ctx, ctx.io, exact) == KOCR_OK);
    Staging st{&ctx, ctx.io, "host_stage_check"};
    CHECK(staging_take(st, rows) == KOCR_OK && ctx.io.off == exact && ctx.io.peak == exact);
    float* crops = (float*)calloc((size_t)nb, CRNN_CROP_PIXELS * sizeof(float));
    CHECK(crnn_forward(&ctx, crops, nb, rows.d) == KOCR_OK && outputs_seen == n_out);
    free(crops);
    // every output back to the caller's rows, pairing the two requests as the staged call does
    void* dev[CrnnDecode::MAX_OUTPUTS];
    int n = 0;
    rows.d.each(LW, C, V, [&](auto*& p, size_t) {
      dev[n++] = p;
      return KOCR_OK;
    });
    n = 0;
    CrnnDecode(h).each(LW, C, V, [&](auto*& p, size_t b) {
      memcpy(p, dev[n++], (size_t)nb * b);
      return KOCR_OK;
    });
  }
  CHECK(crops_seen == M);
  host.each(LW, C, V, [&](auto*& p, size_t b) {
    filled(p, byte_of(host, p), (size_t)M * b);
    free(p);
    return KOCR_OK;
  });
}

int main() {
  kocr_ctx ctx;
  int stages = 0, requests = 0;
  for (int lw : {48, 50, 45}) {  // rnn_steps_to_discard 2 (the default), 0 and 5
    LW = lw;
    for (long M : {2049L, 1L}) check_request(ctx, M), ++requests;
    for (long M : {1L, 7L, 1023L, 1024L, 1025L, 2500L})
      for (int sw = 0; sw < 32; ++sw) {
        ctx.scores_on = sw & 1;
        ctx.beam_width = sw & 2 ? 4 : 0;
        ctx.beam_top_paths = sw & 2 ? 3 : 1;
        ctx.lex_top = sw & 4 ? 5 : 0;
        const bool force = sw & 8;
        ctx.pattern = sw & 16 ? 0 : -1;
        RecStage rec(&ctx, M, force);
        const size_t m = (size_t)M, crop_b = m * CRNN_CROP_PIXELS * sizeof(float);
        Staging st{&ctx, ctx.io, "host_stage_check"};
        CHECK(st.reserve(0, {}, {crop_b, rec.bytes()}) == KOCR_OK);
        float* crops;
        CHECK(st.scratch(crop_b, crops) == KOCR_OK);
        memset(crops, 0, crop_b);
        CHECK(rec.take(st) == KOCR_OK && ctx.io.off <= ctx.io.cap);
        crops_seen = 0;
        CHECK(rec.run(crops) == KOCR_OK && crops_seen == M);
        const bool scores = ctx.scores_on || force, pat = ctx.pattern >= 0;
        const CrnnDecode& r = rec.req;
        filled(r.d_labels, byte_of(r, r.d_labels), m * LW * 4);
        if (scores) filled(r.sc.d_logw, byte_of(r, r.sc.d_logw), m * 4), filled(r.sc.d_chars, byte_of(r, r.sc.d_chars), m * LW * 4);
        if (ctx.beam_width)
          filled(r.bm.d_labels, byte_of(r, r.bm.d_labels), m * 3 * LW * 4), filled(r.bm.d_logp, byte_of(r, r.bm.d_logp), m * 3 * 4);
        if (ctx.lex_top) filled(r.lx.d_index, byte_of(r, r.lx.d_index), m * 5 * 4), filled(r.lx.d_logp, byte_of(r, r.lx.d_logp), m * 5 * 4);
        if (pat) {
          filled(r.pt.d_labels, byte_of(r, r.pt.d_labels), m * LW * 4);
          filled(r.pt.d_logpath, byte_of(r, r.pt.d_logpath), m * 4);
          filled(r.pt.d_logp, byte_of(r, r.pt.d_logp), m * 4);
        }
        CHECK(outputs_seen == 1 + 2 * scores + 2 * (ctx.beam_width > 0) + 2 * (ctx.lex_top > 0) + 3 * pat);
        CHECK(scores || (!r.sc.d_logw && !r.sc.d_chars));
        CHECK(pat || (!r.pt.d_labels && !r.pt.d_logpath && !r.pt.d_logp));
        CHECK(!r.d_probs && !r.lx.d_all);
        // what stays resident: every record with the state of its switch, and all of them forgotten by the next sizing
        rec.keep();
        CHECK(ctx.last_sc.rec == resident(ctx.scores_on) && ctx.last_sc.M == M && ctx.last_sc.lw == LW);
        CHECK(ctx.last_beam.state == resident(ctx.beam_width > 0) && ctx.last_beam.K == ctx.beam_top_paths);
        CHECK(ctx.last_lex.state == resident(ctx.lex_top > 0) && ctx.last_or.state == Resident::OFF);
        CHECK(ctx.last_pat.state == resident(pat));
        ctx.orient_mode = KOCR_ORIENT_ANY;
        OrientWinners won;
        won.words = M / 2;
        rec.keep(&won);
        CHECK(ctx.last_or.state == Resident::VALID && ctx.last_or.M == M / 2 && ctx.last_sc.M == M / 2);
        ctx.orient_mode = KOCR_ORIENT_OFF;
        CHECK(arena_reserve(&ctx, ctx.pl, 1) == KOCR_OK);
        CHECK(ctx.last_sc.rec == Resident::NONE && ctx.last_sc.det == Resident::NONE && ctx.last_beam.state == Resident::NONE &&
              ctx.last_lex.state == Resident::NONE && ctx.last_or.state == Resident::NONE && ctx.last_ch.state == Resident::NONE &&
              ctx.last_pl.state == Resident::NONE && ctx.last_pat.state == Resident::NONE);
        ++stages;
      }
  }
  // no crops: nothing taken, nothing run, "nothing resident, M = 0"
  ctx.scores_on = true;
  ctx.beam_width = 0;
  RecStage(&ctx, 0).keep();
  CHECK(ctx.last_sc.rec == Resident::VALID && ctx.last_sc.M == 0 && !ctx.last_sc.d_logw && ctx.last_beam.state == Resident::OFF);
  // the detector's batch loop covers [0, N) once, in order
  int next = 0;
  CHECK(craft_batches(&ctx, 3, 10, 0, 0, [&](int s, int nb) {
          CHECK(s == next && nb >= 1 && nb <= 3 && ctx.ws.off == 0);
          next += nb;
          return KOCR_OK;
        }) == KOCR_OK && next == 10);
  for (Arena* a : {&ctx.ws, &ctx.io, &ctx.pl}) free(a->base);
  printf("host_stage_check ok: %d stages, %d requests\n", stages, requests);
  return 0;
}
